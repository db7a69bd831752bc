"""A Conv2d + BatchNorm2d + ReLU chain (what baselines.make_layers(batch_norm=True) emits) through
plans2.ChainPlan on the GPU, against the same nn.Sequential in torch float64 on the CPU:

    Conv(3,64,3) BN ReLU, Conv(64,64,3) BN ReLU, MaxPool2d(2), Conv(64,128,3, dilation 2) BN ReLU, Conv(128,1,1)

in training mode (fp32) at 2x3x16x24 and at 2x3x16x64 (a width that is a multiple of 64, which the
fused first-layer form may take), the running statistics after the step, the eval forward, and bf16.

Bounds: max(3 x torch's own fp32 error against float64, floor), torch's error computed here on the same
inputs (measured: 3.6e-7..8.8e-7 on outputs, <= 5.5e-7 on gradients, normwise over all parameters).
Floors: outputs 1e-4; gradients GRAD_FLOOR.  The biases of the three convolutions that feed a training
BatchNorm have an exactly zero true gradient (the batch mean removes them), so they stay out of the
relative norms and are checked against the size of their layer's weight gradient instead.
"""
import copy

import pytest
import torch
import torch.nn as nn

from oracle import dg_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 24), (2, 16, 64)]
OUT_FLOOR = 1e-4
# tests/test_dilation_gpu.py::test_dilated_layer_batchnorm_train's bar for one batch-statistic layer.
# Measured on the MI355X for the three stacked ones (normwise over all parameters but the BN-fed biases):
#   2x3x16x24  outputs 4.9e-7, gradients 6.3e-7 (worst single tensor 1.8e-6), BN-fed biases 4.9e-9 of dW
#   2x3x16x64  outputs 6.8e-7, gradients 6.6e-7 (worst single tensor 2.5e-6), BN-fed biases 4.7e-9 of dW
# so the floor stays at that bar.
GRAD_FLOOR = 1e-4
BN_FED_BIASES = ("0.bias", "3.bias", "7.bias")


def _chain():
    seq = nn.Sequential(nn.Conv2d(3, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
                        nn.Conv2d(64, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
                        nn.MaxPool2d(2, 2),
                        nn.Conv2d(64, 128, 3, padding=2, dilation=2), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
                        nn.Conv2d(128, 1, 1))
    seq.load_state_dict(O.seeded_state_dict(seq.state_dict()))
    return seq


def _inputs(shape):
    B, H, W = shape
    up = lambda v: -(-v // 16) * 16  # noqa: E731  (O.synthetic_batch makes multiples of 16)
    x = O.synthetic_batch(B, up(H), up(W), seed=2112, with_dmap=False)[0][..., :H, :W].contiguous()
    r =torch.randn((B, 1, H // 2, W // 2), generator=torch.Generator().manual_seed(99), dtype=torch.float64)
    return x, r


_REF = {}


def _reference(shape):
    """The float64 training step of the chain on the CPU and torch's own fp32 error against it:
    (output, {name: grad}, state after the step, eval output of that state, fp32 output error, fp32
    gradient error, fp32 worst BN-fed bias ratio).  Computed once per shape."""
    if shape in _REF:
        return _REF[shape]
    x, r = _inputs(shape)
    res = {}
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(_chain()).to(dt).train()
        o = m(x.to(dt))
        (o * r.to(dt)).sum().backward()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        with torch.no_grad():
            ev = m.eval()(x.to(dt))
        res[dt] = (o.detach(), grads, state, ev)
    o64, g64, st64, ev64 = res[torch.float64]
    o32, g32, _, _ = res[torch.float32]
    _REF[shape] = (o64, g64, st64, ev64, _out_err(o32, o64), _grad_err(g32, g64), _bias_ratio(g32))
    return _REF[shape]


def _out_err(a, ref):
    return ((a.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _grad_err(grads, ref):
    keys = [k for k in ref if k not in BN_FED_BIASES]
    num = sum(float((grads[k].double().cpu() - ref[k]).norm() ** 2) for k in keys)
    den = sum(float(ref[k].norm() ** 2) for k in keys)
    return (num / den) ** 0.5


def _bias_ratio(grads):
    return max((grads[k].double().norm() / grads[k.replace("bias", "weight")].double().norm()).item()
               for k in BN_FED_BIASES)


def _plan(seq, dev):
    from dgvcc_amd.models import plans2 as P2
    seq = seq.to(dev)
    return seq, P2.ChainPlan(seq, image_input=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_bn_chain_train_step_matches_float64(dev, shape):
    from dgvcc_amd import engine as E
    from dgvcc_amd.models import plans2 as P2
    o64, g64, st64, ev64, o32_err, g32_err, b32 = _reference(shape)
    x, r = _inputs(shape)
    seq, plan = _plan(_chain().train(), dev)
    layers = [op[1] for op in plan.ops if op[0] == "conv"]
    assert [type(l) for l in layers] == [E.ConvLayer] * 3 and all(l.bn is not None for l in layers)
    out = P2.run_chain(plan, (x.to(dev),), True, torch.float32)
    assert tuple(out.shape) == tuple(o64.shape) and out.dtype == torch.float32
    (out * r.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    tol = max(3 * o32_err, OUT_FLOOR)
    err = _out_err(out.detach(), o64)
    print(f"Conv-BN chain {shape} out: err {err:.3e} tol {tol:.3e} (torch fp32 {o32_err:.3e})")
    assert err < tol, (err, tol)
    grads = {k: p.grad for k, p in seq.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    gtol = max(3 * g32_err, GRAD_FLOOR)
    gerr = _grad_err(grads, g64)
    worst = max(((grads[k].double().cpu() - g64[k]).norm() / g64[k].norm()).item()
                for k in g64 if k not in BN_FED_BIASES)
    bias = _bias_ratio(grads)
    print(f"Conv-BN chain {shape} grads: normwise {gerr:.3e} (worst tensor {worst:.3e}) tol {gtol:.3e} "
          f"(torch fp32 {g32_err:.3e}); BN-fed bias / weight gradient {bias:.3e} (torch fp32 {b32:.3e})")
    assert gerr < gtol, (gerr, gtol)
    assert bias < 1e-4, bias
    # running statistics after the step
    sd = seq.state_dict()
    for k in st64:
        if "running" in k:
            e = ((sd[k].double().cpu() - st64[k]).abs().max() / st64[k].abs().max()).item()
            assert e < 1e-5, (k, e)
        elif "num_batches_tracked" in k:
            assert int(sd[k]) == int(st64[k])
    # eval forward of the stepped statistics
    with torch.no_grad():
        ev = P2.run_chain(plan, (x.to(dev),), False, torch.float32)
    e = _out_err(ev, ev64)
    print(f"Conv-BN chain {shape} eval out: err {e:.3e} tol {tol:.3e}")
    assert e < tol, (e, tol)


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_bn_chain_bf16_runs_finite(dev, shape):
    from dgvcc_amd.models import plans2 as P2
    x, r = _inputs(shape)
    seq, plan = _plan(_chain().train(), dev)
    out = P2.run_chain(plan, (x.to(dev),), True, torch.bfloat16)
    (out.float() * r.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == (shape[0], 1, shape[1] // 2, shape[2] // 2) and bool(torch.isfinite(out).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in seq.parameters())
    assert all(bool(torch.isfinite(v).all()) for v in seq.state_dict().values())


def test_dilated_bn_layer_on_a_ragged_input_still_raises(dev):
    """Batch statistics over a ragged phase batch would count its zero fill: 2x3x18x24 pools to 9x12."""
    from dgvcc_amd.models import plans2 as P2
    seq, plan = _plan(_chain().train(), dev)
    x = O.synthetic_batch(2, 32, 32, seed=2112, with_dmap=False)[0][..., :18, :24].contiguous()
    with pytest.raises(ValueError, match="divisible"):
        P2.run_chain(plan, (x.to(dev),), True, torch.float32)
