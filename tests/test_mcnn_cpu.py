"""MCNN and the small-channel convolution family without a GPU: the drop-in surface (state_dict
keys and shapes of the reference, its inverted load_weights flag), the size guard, how ChainPlan
routes convolutions between the dense and the small-channel layer, and the C-ABI's argument
checks (invalid and out-of-family calls return before any launch)."""
import json
import os

import pytest
import torch
import torch.nn as nn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_state_dict_keys_and_shapes_are_the_references():
    from dgvcc_amd.models.baselines import MCNN
    want = json.load(open(os.path.join(GOLD, "mcnn_keys.json")))
    got = [[k, list(v.shape)] for k, v in MCNN().state_dict().items()]
    assert len(want) == 26
    assert got == want


def test_initialize_weights_runs_exactly_when_load_weights_is_false(monkeypatch):
    from dgvcc_amd.models.baselines import MCNN
    ran = []
    real = MCNN._initialize_weights
    monkeypatch.setattr(MCNN, "_initialize_weights", lambda self: (ran.append(1), real(self))[1])
    m = MCNN()
    assert ran == [1]
    convs = [c for c in m.modules() if isinstance(c, nn.Conv2d)]
    assert len(convs) == 13 and all(bool((c.bias == 0).all()) for c in convs)
    w = m.branch1[3].weight  # 32 x 16 x 7 x 7: kaiming_normal_, std = sqrt(2 / fan_in)
    assert abs(w.std().item() / (2.0 / (16 * 49)) ** 0.5 - 1) < 0.05
    MCNN(load_weights=False)
    assert ran == [1, 1]
    m = MCNN(load_weights=True)
    assert ran == [1, 1]
    assert not all(bool((c.bias == 0).all()) for c in m.modules() if isinstance(c, nn.Conv2d))


@pytest.mark.parametrize("hw", [(30, 32), (32, 34), (33, 33)])
def test_sizes_that_are_no_multiple_of_4_raise(hw):
    from dgvcc_amd.models.baselines import MCNN
    with pytest.raises(ValueError, match="multiples of 4"):
        MCNN()(torch.zeros(1, 3, *hw))


def test_chainplan_routes_mcnn_branches_to_small_layers():
    from dgvcc_amd import engine as E
    from dgvcc_amd.models import plans2 as P2
    from dgvcc_amd.models.baselines import MCNN
    m = MCNN()
    for branch, forms in ((m.branch1, [(3, 16, 9), (16, 32, 7), (32, 16, 7), (16, 8, 7)]),
                          (m.branch2, [(3, 20, 7), (20, 40, 5), (40, 20, 5), (20, 10, 5)]),
                          (m.branch3, [(3, 24, 5), (24, 48, 3), (48, 24, 3), (24, 12, 3)])):
        for kw in ({}, {"image_input": True}):
            plan = P2.ChainPlan(branch, **kw)
            assert [op[0] for op in plan.ops] == ["conv", "pool", "conv", "pool", "conv", "conv"]
            layers = [op[1] for op in plan.ops if op[0] == "conv"]
            assert all(type(l) is E.SmallConvLayer and l.act == E.ACT_RELU for l in layers)
            assert [(l.Cin, l.Cout, l.R) for l in layers] == forms
            assert [(l.Cp_in, l.Cp_out) for l in layers] == [(-(-a // 8) * 8, -(-b // 8) * 8) for a, b, _ in forms]
            assert plan.params() == [p for c in branch if isinstance(c, nn.Conv2d) for p in (c.weight, c.bias)]


def test_chainplan_keeps_the_dense_layers_of_csrnet_and_models2():
    """Every convolution the dense path takes keeps its layer class: CSRNet's plan is sixteen
    engine.ConvLayer (the first the im2col stem) and the 1x1 head, as before the small-channel family."""
    from dgvcc_amd import engine as E
    from dgvcc_amd.models import plans2 as P2
    from dgvcc_amd.models.baselines import CSRNet
    m = CSRNet()
    plan = P2.ChainPlan(list(m.frontend) + list(m.backend) + [m.output_layer], image_input=True)
    kinds = [op[0] for op in plan.ops]
    assert kinds == (["conv"] * 2 + ["pool"] + ["conv"] * 2 + ["pool"] + ["conv"] * 3 + ["pool"] + ["conv"] * 9
                     + ["head"])
    layers = [op[1] for op in plan.ops if op[0] == "conv"]
    assert all(type(l) is E.ConvLayer for l in layers)
    assert [l.first for l in layers] == [True] + [False] * 15
    assert [l.dil for l in layers] == [1] * 10 + [2] * 6
    # a dense 1x1 / 3x3 chain and the decoder-concatenation first layer are untouched too
    plan = P2.ChainPlan([nn.Conv2d(64, 128, 3, padding=1), nn.ReLU(), nn.Conv2d(128, 64, 1), nn.ReLU()])
    assert [type(op[1]) for op in plan.ops] == [E.ConvLayer, E.ConvLayer]
    assert not P2.ChainPlan.is_small(nn.Conv2d(3, 64, 3, padding=1), True)
    assert P2.ChainPlan.is_small(nn.Conv2d(3, 64, 3, padding=1), False)
    assert P2.ChainPlan.is_small(nn.Conv2d(3, 64, 5, padding=2), True)


@pytest.mark.parametrize("conv, what", [
    (nn.Conv2d(3, 8, 11, padding=5), "kernel_size=(11, 11)"),
    (nn.Conv2d(65, 8, 3, padding=1), "in_channels=65"),
    (nn.Conv2d(8, 8, 3, stride=2, padding=1), "stride=(2, 2)"),
    (nn.Conv2d(8, 8, 3, padding=0), "padding=(0, 0)"),
    (nn.Conv2d(8, 8, 3, padding=2, dilation=2), "dilation=(2, 2)"),
    (nn.Conv2d(8, 8, 3, padding=1, groups=2), "groups=2"),
])
def test_unsupported_forms_raise_with_their_parameters(conv, what):
    from dgvcc_amd import engine as E
    from dgvcc_amd.models import plans2 as P2
    with pytest.raises(ValueError) as e:
        P2.ChainPlan([conv, nn.ReLU()])
    assert what in str(e.value)
    with pytest.raises(ValueError) as e:
        E.SmallConvLayer(conv, None)
    assert what in str(e.value)


def test_batchnorm_and_dropout_on_small_layers_raise():
    from dgvcc_amd import engine as E
    from dgvcc_amd.models import plans2 as P2
    from dgvcc_amd.models.models import ConvBlock
    with pytest.raises(ValueError, match="BatchNorm on a small-channel layer"):
        E.SmallConvLayer(nn.Conv2d(3, 16, 9, padding=4), nn.BatchNorm2d(16))
    with pytest.raises(ValueError, match="Dropout2d after a small-channel"):
        P2.ChainPlan([ConvBlock(16, 8, 3, padding=1), nn.Dropout2d(0.5), ConvBlock(8, 8, 3, padding=1)])
    with pytest.raises(ValueError, match="BatchNorm on a small-channel layer"):
        P2.ChainPlan([ConvBlock(16, 8, 3, padding=1, bn=True), ConvBlock(8, 8, 3, padding=1)])


def test_smallconv_abi_rejects_without_a_device():
    """Null pointers -> DG_ERR_INVALID (-1); out-of-family shapes -> DG_ERR_UNSUPPORTED (-2); both
    before any launch, so the fake non-null addresses below are never touched."""
    from dgvcc_amd import _capi
    L = _capi.lib()
    P = 4096  # a non-null, 16-byte aligned stand-in address
    fwd = lambda *, x=P, wp=P, y=P, dt=0, C=16, Cout=32, R=7, S=7, stride=1, pad=3, dil=1: L.dg_smallconv_fwd(  # noqa: E731
        dt, x, 16, 2, 8, 8, C, wp, Cout, R, S, stride, pad, dil, None, 1, y, 32, None)
    assert fwd(x=None) == -1 and fwd(wp=None) == -1 and fwd(y=None) == -1 and fwd(dt=7) == -1
    for kw in (dict(R=11, S=11, pad=5), dict(C=65), dict(Cout=65), dict(C=0), dict(stride=2), dict(dil=2),
               dict(pad=2), dict(R=7, S=5), dict(R=4, S=4, pad=1)):
        assert fwd(**kw) == -2, kw
    wg = lambda *, x=P, dy=P, dw=P, work=P, C=16, Cout=32, R=7, stride=1: L.dg_smallconv_wgrad(  # noqa: E731
        1, x, 16, dy, 32, 2, 8, 8, C, Cout, R, R, stride, (R - 1) // 2, 1, dw, None, work, 1 << 30, None)
    assert wg(x=None) == -1 and wg(dy=None) == -1 and wg(dw=None) == -1 and wg(work=None) == -1
    assert wg(R=11) == -2 and wg(C=65) == -2 and wg(stride=2) == -2
    assert L.dg_smallconv_pack(0, None, 32, 16, 7, 7, 0, P, None) == -1
    assert L.dg_smallconv_pack(0, P, 32, 16, 11, 11, 0, P, None) == -2
    assert L.dg_smallconv_pack_elems(0, 32, 16, 11, 11, 0) == -2 and L.dg_smallconv_pack_elems(9, 32, 16, 7, 7, 0) == -1
    assert L.dg_image_nhwc_pad(0, None, 2, 3, 8, 8, P, 8, 8, None) == -1
    assert L.dg_image_nhwc_pad(0, P, 2, 3, 8, 8, P, 8, 4, None) == -2  # Cp is no multiple of 8


def test_smallconv_workspace_and_pack_sizes():
    from dgvcc_amd import _capi
    L = _capi.lib()
    # rows of K = taps x channels of a stage, rounded up to the MFMA step group (32 16-bit / 16 f32 elements)
    assert L.dg_smallconv_pack_elems(1, 32, 16, 7, 7, 0) == 32 * 800           # 49*16 = 784 -> 800
    assert L.dg_smallconv_pack_elems(1, 32, 16, 7, 7, 1) == 16 * 49 * 32       # flipped: 32 -> 16
    assert L.dg_smallconv_pack_elems(0, 16, 3, 9, 9, 0) == 16 * 336            # f32: Cin 3 packs 4 per tap, 324 -> 336
    assert L.dg_smallconv_pack_elems(1, 16, 3, 9, 9, 0) == 16 * 672            # 16-bit: 8 per tap, 648 -> 672
    assert L.dg_smallconv_pack_elems(0, 64, 40, 5, 5, 0) == 64 * (800 + 208)   # two stages: 32 + 8 channels
    ws = L.dg_smallconv_wgrad_workspace(1, 2, 19, 69, 16, 32, 7, 7)
    assert ws > 0 and ws % (32 * 4) == 0
    assert L.dg_smallconv_wgrad_workspace(1, 0, 19, 69, 16, 32, 7, 7) == -1
    assert L.dg_smallconv_wgrad_workspace(1, 2, 19, 69, 16, 32, 11, 11) == -2
