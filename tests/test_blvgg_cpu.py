"""BL's VGG19 counter without a GPU: the drop-in surface (state_dict keys and shapes of the reference),
its plan (op kinds, layer classes, the align-corners upsampling, the abs head), the size guard, what
ChainPlan now parses (Conv2d + BatchNorm2d chains, align-corners upsampling, head_abs) and what it
still refuses, main_base's model table, and the C-ABI's two new entry points."""
import json
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_state_dict_keys_and_shapes_are_the_references():
    from dgvcc_amd.models.baselines import BL_VGG, VGG
    want = json.load(open(os.path.join(GOLD, "blvgg_keys.json")))
    m = BL_VGG()
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(want) == 38
    assert got == want
    assert isinstance(m, VGG)
    assert sorted({k.split(".")[0] for k, _ in got}) == ["features", "reg_layer"]
    assert [k for k, _ in got if k.startswith("reg_layer")] == [f"reg_layer.{i}.{p}" for i in (0, 2, 4)
                                                                for p in ("weight", "bias")]


def test_reference_make_layers_call_shape():
    from dgvcc_amd.models import baselines as B
    seq = B.make_layers(B.cfg["E"], batch_norm=False)
    assert sum(isinstance(m, nn.Conv2d) for m in seq) == 16 and sum(isinstance(m, nn.MaxPool2d) for m in seq) == 4
    assert not any(isinstance(m, nn.BatchNorm2d) for m in seq)
    assert {"VGG", "BL_VGG"} <= set(B.__all__)


def _plan(m):
    from dgvcc_amd.models import plans2 as P2
    up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
    return P2.ChainPlan(list(m.features) + [up] + list(m.reg_layer), image_input=True, head_abs=True)


def test_plan_ops_layers_upsampling_and_abs_head():
    from dgvcc_amd import engine as E
    from dgvcc_amd import kernels as K
    from dgvcc_amd.models.baselines import BL_VGG
    m = BL_VGG()
    plan = _plan(m)
    kinds = [op[0] for op in plan.ops]
    assert kinds == (["conv"] * 2 + ["pool"] + ["conv"] * 2 + ["pool"] + ["conv"] * 4 + ["pool"] + ["conv"] * 4
                     + ["pool"] + ["conv"] * 4 + ["up"] + ["conv"] * 2 + ["head"])
    layers = [op[1] for op in plan.ops if op[0] == "conv"]
    assert len(layers) == 16 + 2 and all(type(l) is E.ConvLayer for l in layers)
    assert [l.first for l in layers] == [True] + [False] * 17
    assert all(l.bn is None and l.act == E.ACT_RELU and l.dil == 1 for l in layers)
    up = plan.ops[kinds.index("up")]
    assert up[1] == 2 and up[2] == K.UP_BILINEAR_AC
    head = plan.ops[-1]
    assert head[1] is m.reg_layer[4] and head[2] == K.ACT_NONE and head[3] is False and head[4] is True
    assert len(plan.params()) == 38 and {id(p) for p in plan.params()} == {id(p) for p in m.parameters()}


def test_pickled_model_drops_its_plan():
    import pickle
    from dgvcc_amd.models.baselines import BL_VGG
    m = BL_VGG()
    m._plans = {"net": _plan(m)}
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._plans is None and m._plans is not None
    assert [k for k in m2.state_dict()] == [k for k in m.state_dict()]


@pytest.mark.parametrize("hw", [(24, 32), (32, 40), (33, 33)])
def test_sizes_that_are_no_multiple_of_16_raise(hw):
    from dgvcc_amd.models.baselines import BL_VGG
    with pytest.raises(ValueError, match=f"multiples of 16.*{hw[0]}x{hw[1]}"):
        BL_VGG()(torch.zeros(1, 3, *hw))


def test_pretrained_never_downloads(monkeypatch, tmp_path):
    """pretrained=True reads the local hub cache only; with none it warns and keeps the random init."""
    import torch.hub
    import torch.utils.model_zoo as zoo
    from dgvcc_amd.models.baselines import BL_VGG

    def boom(*a, **k):
        raise AssertionError("a download was attempted")

    monkeypatch.setattr(zoo, "load_url", boom)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", boom)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    with pytest.warns(UserWarning, match="VGG19 weights unavailable offline"):
        m = BL_VGG(pretrained=True)
    assert len(m.state_dict()) == 38


# ---------------------------------------------------------------- ChainPlan parsing --
def test_chainplan_parses_conv_batchnorm_chains():
    from dgvcc_amd import engine as E
    from dgvcc_amd.models import plans2 as P2
    from dgvcc_amd.models.baselines import make_layers
    seq = make_layers([64, "M", 128], batch_norm=True)
    plan = P2.ChainPlan(seq, image_input=True)
    assert [op[0] for op in plan.ops] == ["conv", "pool", "conv"]
    l0, l1 = plan.ops[0][1], plan.ops[2][1]
    assert type(l0) is E.ConvLayer and type(l1) is E.ConvLayer
    assert l0.bn is seq[1] and l1.bn is seq[5] and l0.conv is seq[0] and l1.conv is seq[4]
    assert l0.act == E.ACT_RELU and l1.act == E.ACT_RELU and l0.first and not l1.first
    assert {id(p) for p in plan.params()} == {id(p) for p in seq.parameters()}
    # dilated, and without a ReLU behind the BatchNorm
    conv, bn = nn.Conv2d(64, 128, 3, padding=2, dilation=2), nn.BatchNorm2d(128)
    plan = P2.ChainPlan([conv, bn, nn.Conv2d(128, 64, 3, padding=1), nn.ReLU()])
    a, b = plan.ops[0][1], plan.ops[1][1]
    assert a.bn is bn and a.dil == 2 and a.act == E.ACT_NONE
    assert b.bn is None and b.act == E.ACT_RELU


def test_chainplan_batchnorm_refusals():
    from dgvcc_amd.models import plans2 as P2
    with pytest.raises(ValueError, match="BatchNorm on a small-channel layer"):
        P2.ChainPlan([nn.Conv2d(16, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU()])
    for mods in ([nn.BatchNorm2d(64), nn.Conv2d(64, 64, 3, padding=1)],
                 [nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(), nn.BatchNorm2d(64)],
                 [nn.Conv2d(64, 64, 3, padding=1), nn.MaxPool2d(2), nn.BatchNorm2d(64)]):
        with pytest.raises(ValueError, match="unsupported module BatchNorm2d"):
            P2.ChainPlan(mods)


def test_chainplan_upsampling_modes():
    from dgvcc_amd import kernels as K
    from dgvcc_amd.models import plans2 as P2
    conv = lambda: nn.Conv2d(64, 64, 3, padding=1)  # noqa: E731
    for up, s, mode in ((nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True), 2, K.UP_BILINEAR_AC),
                        (nn.UpsamplingBilinear2d(scale_factor=4), 4, K.UP_BILINEAR_AC),
                        (nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False), 2, K.UP_BILINEAR),
                        (nn.Upsample(scale_factor=2, mode="bilinear"), 2, K.UP_BILINEAR)):
        plan = P2.ChainPlan([conv(), up, conv()])
        assert plan.ops[1] == ["up", s, mode]
    for up in (nn.Upsample(scale_factor=2, mode="nearest"), nn.Upsample(scale_factor=2, mode="bicubic"),
               nn.Upsample(scale_factor=1.5, mode="bilinear", align_corners=True),
               nn.Upsample(size=(8, 8), mode="bilinear", align_corners=True)):
        with pytest.raises(ValueError, match="upsampling"):
            P2.ChainPlan([conv(), up, conv()])


def test_head_abs_needs_an_activation_free_head():
    from dgvcc_amd.models import plans2 as P2
    body = lambda: [nn.Conv2d(64, 64, 3, padding=1), nn.ReLU()]  # noqa: E731
    plan = P2.ChainPlan(body() + [nn.Conv2d(64, 1, 1)], head_abs=True)
    assert plan.ops[-1][0] == "head" and plan.ops[-1][4] is True
    assert P2.ChainPlan(body() + [nn.Conv2d(64, 1, 1)]).ops[-1][4] is False
    for tail in ([nn.Conv2d(64, 1, 1), nn.ReLU()], [nn.Conv2d(64, 1, 1), nn.Sigmoid()],
                 [nn.Conv2d(64, 3, 1), nn.Tanh()], []):
        with pytest.raises(ValueError, match="head_abs"):
            P2.ChainPlan(body() + tail, head_abs=True)


def test_existing_error_texts_stay():
    from dgvcc_amd.models import plans2 as P2
    with pytest.raises(ValueError, match="only MaxPool2d\\(2, 2\\)"):
        P2.ChainPlan([nn.Conv2d(64, 64, 3, padding=1), nn.MaxPool2d(3, 2)])
    with pytest.raises(ValueError, match="unsupported module Linear"):
        P2.ChainPlan([nn.Conv2d(64, 64, 3, padding=1), nn.Linear(4, 4)])


# ---------------------------------------------------------------- entry points --
def test_main_base_get_model():
    from dgvcc_amd import main as Mn
    from dgvcc_amd import main_base as Mb
    from dgvcc_amd.models import baselines as B
    from dgvcc_amd.models.models2 import DensityRegressorBase
    assert type(Mb.get_model("csrnet", {"load_weights": False})) is B.CSRNet
    assert type(Mb.get_model("mcnn", {})) is B.MCNN
    bl = Mb.get_model("bl", {"pretrained": False})
    assert type(bl) is B.VGG and len(bl.state_dict()) == 38
    assert type(Mb.get_model("dgnet", {"pretrained": False})) is DensityRegressorBase
    for name in ("sasnet", "dssinet", "cctrans"):
        with pytest.raises(NotImplementedError, match="DESIGN.md §7"):
            Mb.get_model(name, {})
    with pytest.raises(ValueError, match="Unknown model: vgg"):
        Mb.get_model("vgg", {})
    # main's own table is unchanged
    assert Mn.get_model("bl", {}) is None and Mn.get_model("csrnet", {}) is None
    with pytest.raises(NotImplementedError):
        Mn.get_dataset("bay", {}, "train")
    assert (Mb.get_loss, Mb.get_dataset, Mb.get_optimizer, Mb.get_scheduler) == \
        (Mn.get_loss, Mn.get_dataset, Mn.get_optimizer, Mn.get_scheduler)


def test_main_base_load_config_runs_simple_mode(monkeypatch, tmp_path):
    """main_base.load_config: main's, with main_base's model table, 'simple' mode whatever the config
    says and its patch_size or 10000; the `loss: bl` crop check applies before any data is read."""
    import yaml
    from dgvcc_amd import main as Mn
    from dgvcc_amd import main_base as Mb
    seen = []

    def no_data(name, params, method):
        seen.append((name, method, dict(params)))
        raise RuntimeError("stop before the data")

    monkeypatch.setattr(Mn, "get_dataset", no_data)
    cfg = {"seed": 1, "version": "t", "device": "cpu", "log_para": 1000, "mode": "final",
           "model": {"name": "bl", "params": {"pretrained": False}}, "checkpoint": None,
           "loss": {"name": "bl", "params": {"sigma": 8, "c_size": 64, "stride": 8, "background_ratio": 1,
                                            "use_background": True, "device": "cpu"}},
           "train_dataset": {"name": "den_cls", "params": {"crop_size": 32}}}
    path = tmp_path / "bl.yml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="c_size 64 must equal"):
        Mb.load_config(str(path), "train")
    assert seen == []
    cfg["train_dataset"]["params"]["crop_size"] = 64
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(RuntimeError, match="stop before the data"):
        Mb.load_config(str(path), "train")
    assert seen == [("den_cls", "train", {"crop_size": 64, "bl_targets": True})]


def test_main_base_init_params(monkeypatch, tmp_path):
    import yaml
    from dgvcc_amd import main as Mn
    from dgvcc_amd import main_base as Mb
    monkeypatch.setattr(Mn, "get_dataset", lambda n, p, m: (torch.utils.data.TensorDataset(torch.zeros(2, 1)), None))
    base = {"seed": 1, "version": "t", "device": "cpu", "log_para": 1000, "mode": "final",
            "model": {"name": "mcnn", "params": {}}, "checkpoint": None,
            "test_dataset": {"name": "den_cls", "params": {}}, "test_loader": {"batch_size": 1}}
    for extra, want in (({}, 10000), ({"patch_size": 512}, 512)):
        path = tmp_path / "c.yml"
        path.write_text(yaml.safe_dump(dict(base, **extra)))
        init, task = Mb.load_config(str(path), "test")
        assert init == {"seed": 1, "version": "t", "device": "cpu", "log_para": 1000, "patch_size": want,
                        "mode": "simple"}
        assert type(task["model"]).__name__ == "MCNN" and "test_dataloader" in task
    # main itself still has no such model
    init, task = Mn.load_config(str(path), "test")
    assert task["model"] is None


def test_main_base_runs_as_a_module():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "dgvcc_amd.main_base", "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "--config" in r.stdout and "train_test" in r.stdout


# ---------------------------------------------------------------- C-ABI --
def test_abi_declares_and_exports_abs():
    from dgvcc_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "dgvcc.h")).read()
    assert re.search(r"int dg_abs_fwd\(const float\* z, int64_t n, float\* y, void\* stream\);", hdr)
    assert re.search(r"int dg_abs_bwd\(const float\* z, const float\* gy, int64_t n, float\* gz, int accumulate, "
                     r"void\* stream\);", hdr)
    syms = set(_capi.exported_symbols())
    assert {"dg_abs_fwd", "dg_abs_bwd", "dg_tanh_fwd", "dg_tanh_bwd"} <= syms
    assert _capi.lib().dg_version() == 8 and _capi.header_abi_version() == 8


def test_abs_abi_rejects_without_a_device():
    """Null pointers and n <= 0 -> DG_ERR_INVALID (-1) before any launch."""
    from dgvcc_amd import _capi
    L = _capi.lib()
    P = 4096
    assert L.dg_abs_fwd(None, 4, P, None) == -1 and L.dg_abs_fwd(P, 4, None, None) == -1
    assert L.dg_abs_fwd(P, 0, P, None) == -1
    assert L.dg_abs_bwd(None, P, 4, P, 0, None) == -1 and L.dg_abs_bwd(P, None, 4, P, 0, None) == -1
    assert L.dg_abs_bwd(P, P, 4, None, 0, None) == -1 and L.dg_abs_bwd(P, P, -1, P, 0, None) == -1
