"""Host side of the dilated convolution / CSRNet support (no GPU): the model's state_dict
against the reference's (tests/golden/make_golden_csrnet.py), which dilated forms
engine.ConvLayer takes, how ChainPlan parses the network, and the argument checks of the two
layout entry points (they return before any launch)."""
import json
import os

import pytest
import torch
import torch.nn as nn

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_csrnet_state_dict_keys_match_reference():
    from dgvcc_amd.models.baselines import CSRNet
    keys = json.load(open(os.path.join(G, "csrnet_keys.json")))
    mine = [[k, list(v.shape)] for k, v in CSRNet().state_dict().items()]
    assert mine == keys
    assert len(mine) == 34 and mine[0][0] == "frontend.0.weight" and mine[-1][0] == "output_layer.bias"


def test_csrnet_initialize_weights():
    from dgvcc_amd.models.baselines import CSRNet
    torch.manual_seed(0)
    m = CSRNet(load_weights=True)
    convs = [c for c in m.modules() if isinstance(c, nn.Conv2d)]
    assert len(convs) == 17
    assert all(float(c.bias.detach().abs().max()) == 0.0 for c in convs)
    w = torch.cat([c.weight.detach().reshape(-1) for c in convs[1:]])
    assert abs(float(w.std()) - 0.01) < 2e-4 and abs(float(w.mean())) < 1e-4
    assert [c.dilation for c in m.backend if isinstance(c, nn.Conv2d)] == [(2, 2)] * 6
    assert [c.out_channels for c in m.backend if isinstance(c, nn.Conv2d)] == [512, 512, 512, 256, 128, 64]


def test_convlayer_takes_dilation():
    from dgvcc_amd import engine as E
    layer = E.ConvLayer(nn.Conv2d(64, 64, 3, padding=2, dilation=2), None)
    assert (layer.dil, layer.R, layer.pad, layer.resident) == (2, 3, 1, False)
    assert E.ConvLayer(nn.Conv2d(64, 128, 3, padding=3, dilation=3), nn.BatchNorm2d(128)).dil == 3
    plain = E.ConvLayer(nn.Conv2d(64, 64, 3, padding=1), None)
    assert (plain.dil, plain.R, plain.pad) == (1, 3, 1)


@pytest.mark.parametrize("kw", [
    dict(kernel_size=3, padding=1, dilation=2),             # padding != dilation
    dict(kernel_size=3, padding=2, dilation=2, stride=2),   # strided
    dict(kernel_size=3, padding=(2, 3), dilation=(2, 3)),   # asymmetric
    dict(kernel_size=5, padding=4, dilation=2),             # 5x5
    dict(kernel_size=1, padding=0, dilation=2),             # 1x1
])
def test_convlayer_other_dilated_forms_raise(kw):
    from dgvcc_amd import engine as E
    with pytest.raises(ValueError, match="dilat"):
        E.ConvLayer(nn.Conv2d(64, 64, **kw), None)


def test_convlayer_dilated_first_layer_raises():
    from dgvcc_amd import engine as E
    with pytest.raises(ValueError, match="dilat"):
        E.ConvLayer(nn.Conv2d(3, 64, 3, padding=2, dilation=2), None, first=True)


def test_convblock_dilation_constructs_a_layer():
    from dgvcc_amd import engine as E
    from dgvcc_amd.models.models import ConvBlock
    cb = ConvBlock(64, 64, padding=2, dilation=2, bn=True)
    assert E.ConvLayer(cb.conv, cb.bn).dil == 2


def test_phase_mask_repeats_each_image_row():
    from dgvcc_amd import engine as E
    m = torch.arange(6.0).reshape(2, 3)
    assert E.phase_mask(None, 2) is None and E.phase_mask(m, 1) is m
    assert torch.equal(E.phase_mask(m, 2), torch.stack([m[0]] * 4 + [m[1]] * 4))


def test_chainplan_parses_csrnet():
    from dgvcc_amd.models import plans2 as P2
    from dgvcc_amd.models.baselines import CSRNet
    m = CSRNet()
    plan = P2.ChainPlan(list(m.frontend) + list(m.backend) + [m.output_layer], image_input=True)
    kinds = [op[0] for op in plan.ops]
    assert kinds == ["conv"] * 2 + ["pool"] + ["conv"] * 2 + ["pool"] + ["conv"] * 3 + ["pool"] + ["conv"] * 9 + ["head"]
    assert [op[1].dil for op in plan.ops if op[0] == "conv"] == [1] * 10 + [2] * 6
    assert plan.ops[-1][1] is m.output_layer and plan.ops[-1][2] == 0 and plan.ops[-1][3] is False
    assert plan._run_end(13) == 18 and plan._run_end(10) == 12
    assert [tuple(p.shape) for p in plan.params()] == [tuple(p.shape) for p in m.parameters()]


def test_chainplan_bare_conv_stays_a_layer_when_not_terminal():
    """The op list of the chains that parsed before is unchanged: a bare 3x3 Conv2d, or a 1x1 one
    followed by further convs, is a conv op; only a terminal 1x1 with <= 4 channels is a head."""
    from dgvcc_amd.models import plans2 as P2
    mods = [nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 1), nn.ReLU(),
            nn.Conv2d(64, 64, 3, padding=1)]
    assert [op[0] for op in P2.ChainPlan(mods).ops] == ["conv", "conv", "conv"]
    from dgvcc_amd.models.models2 import Generator
    g = Generator()
    kinds = [op[0] for op in P2.ChainPlan(list(g.enc) + list(g.dec), image_input=True).ops]
    assert kinds.count("head") == 1 and kinds[-1] == "head" and kinds.count("conv") == 21


def test_layout_entry_points_check_arguments():
    from dgvcc_amd import _capi
    L = _capi.lib()
    p = 1 << 20  # a non-null, 16-byte aligned address: every case returns before a launch
    for f in (L.dg_space_to_batch, L.dg_batch_to_space):
        assert f(0, None, 64, 1, 4, 4, 64, 2, p, 64, 0, None) == -1      # null source
        assert f(0, p, 64, 1, 4, 4, 64, 2, None, 64, 0, None) == -1      # null destination
        assert f(0, p, 64, 1, 4, 4, 64, 0, p, 64, 0, None) == -1         # d < 1
        assert f(0, p, 64, 0, 4, 4, 64, 2, p, 64, 0, None) == -1         # N <= 0
        assert f(0, p, 64, 1, 4, -1, 64, 2, p, 64, 0, None) == -1        # W <= 0
        assert f(0, p, 32, 1, 4, 4, 64, 2, p, 64, 0, None) == -1         # ldx < C
        assert f(0, p, 64, 1, 4, 4, 64, 2, p, 60, 0, None) == -1         # ldy < C
        assert f(7, p, 64, 1, 4, 4, 64, 2, p, 64, 0, None) == -1         # unknown dtype
        assert f(0, p, 64, 1, 4, 4, 6, 2, p, 64, 0, None) == -2          # 24-byte f32 rows
        assert f(1, p, 64, 1, 4, 4, 12, 2, p, 64, 0, None) == -2         # 24-byte bf16 rows
        assert f(2, p, 64, 1, 4, 4, 16, 2, p, 68, 0, None) == -2         # pixel stride not 16 bytes


def test_layout_wrappers_guard_shapes():
    from dgvcc_amd import kernels as K
    x = K.Act(torch.zeros(2, 7, 9, 64))
    assert K.phase_shape(2, 7, 9, 2) == (8, 4, 5) and K.phase_shape(2, 8, 12, 3) == (18, 3, 4)
    with pytest.raises(K.DGError, match="phase batch"):
        K.space_to_batch(x, 2, K.Act(torch.zeros(8, 4, 4, 64)))
    with pytest.raises(K.DGError, match="phase batch"):
        K.batch_to_space(K.Act(torch.zeros(8, 4, 5, 32)), 2, x)
    with pytest.raises(K.DGError, match="dtypes"):
        K.space_to_batch(x, 2, K.Act(torch.zeros(8, 4, 5, 64, dtype=torch.bfloat16)))


def test_mse_count_loss_rejects_other_mismatches():
    from dgvcc_amd.losses import MSELoss
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    tr = DGTrainer.__new__(DGTrainer)
    tr.device, tr.log_para = "cpu", 1000
    for shape in [(2, 1, 8, 4), (2, 1, 5, 5), (2, 1, 128, 128), (1, 1, 8, 8)]:
        with pytest.raises(ValueError, match="MSELoss"):
            tr.compute_count_loss(MSELoss(), torch.zeros(shape), (None, torch.zeros(2, 1, 64, 64), None))
