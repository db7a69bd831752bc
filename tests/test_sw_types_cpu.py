"""CPU-only checks of SwitchWhiten2d beyond the SW counter's own configuration (sw_type 3 and 5,
tied mixing weights, no affine): the float64 restatement tests/sw_ref.py against the reference
operator's float64 results (tests/golden/sw_types.npz, written by
tests/golden/make_golden_sw_types.py), the modules' construction and state_dict keys, the counter's
sw_cfg, and the new C entry points' argument validation (invalid calls return before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sw_ref as R

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "sw_types.npz"))
ALL12 = [(t, tie, aff) for t in (2, 3, 5) for tie in (False, True) for aff in (True, False)]


def rel(a, b):
    b = torch.as_tensor(b, dtype=torch.float64)
    return ((a.double() - b.reshape(a.shape)).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def test_fixture_holds_the_eleven_variants():
    names = {k.split("__")[0] for k in GOLD.files}
    assert names == {R.variant_name(*v) for v in R.VARIANTS} and len(names) == 11


@pytest.mark.parametrize("variant", R.VARIANTS, ids=lambda v: R.variant_name(*v))
def test_sw_ref_matches_reference_float64(variant):
    """Both sides float64, differing in summation order only: 1e-10 relative on y, gx, every
    parameter gradient, the updated running statistics and the eval-mode output."""
    sw_type, tie, affine = variant
    name = R.variant_name(*variant)
    x, gy, params = R.fixture_case(*variant)
    out = R.run(x, gy, params, sw_type)
    out["y_eval"] = R.run_eval(x, params, sw_type)
    want = {k[len(name) + 2:] for k in GOLD.files if k.startswith(name + "__")} - {"keys"}
    assert want == set(out), (sorted(want), sorted(out))
    for k in sorted(want):
        e = rel(out[k], GOLD[f"{name}__{k}"])
        assert e < 1e-10, (k, e)


@pytest.mark.parametrize("variant", R.VARIANTS, ids=lambda v: R.variant_name(*v))
@pytest.mark.parametrize("cls", ["SwitchWhiten2d", "SyncSwitchWhiten2d"])
def test_state_dict_keys_match_reference(cls, variant):
    from dgvcc_amd.models import trunks
    sw_type, tie, affine = variant
    m = getattr(trunks, cls)(32, sw_type=sw_type, tie_weight=tie, affine=affine)
    keys = [str(k) for k in GOLD[R.variant_name(*variant) + "__keys"]]
    assert list(m.state_dict()) == keys == R.state_keys(tie, affine)
    assert m.sw_mean_weight.shape == (sw_type,)
    assert (m.sw_var_weight is None) == tie and (m.weight is None) == (m.bias is None) == (not affine)
    if not tie:
        assert m.sw_var_weight.shape == (sw_type,)


@pytest.mark.parametrize("variant", ALL12, ids=lambda v: R.variant_name(*v))
@pytest.mark.parametrize("cls", ["SwitchWhiten2d", "SyncSwitchWhiten2d"])
def test_all_variants_construct(cls, variant):
    from dgvcc_amd.models import trunks
    sw_type, tie, affine = variant
    m = getattr(trunks, cls)(64, num_pergroup=16, sw_type=sw_type, T=5, tie_weight=tie, eps=1e-5, momentum=0.9,
                             affine=affine)
    assert (m.sw_type, m.tie_weight, m.affine, m.num_groups) == (sw_type, tie, affine, 4)
    assert m.running_mean.shape == (4, 16, 1) and m.running_cov.shape == (4, 16, 16)
    assert len(list(m.parameters())) == 1 + (not tie) + 2 * affine
    assert callable(m.forward) and "sw_type={}".format(sw_type) in repr(m)


def test_unsupported_configurations_still_raise():
    from dgvcc_amd.models.trunks import SwitchWhiten2d, SyncSwitchWhiten2d
    for cls in (SwitchWhiten2d, SyncSwitchWhiten2d):
        with pytest.raises(NotImplementedError):
            cls(32, num_pergroup=8)
        with pytest.raises(NotImplementedError):
            cls(32, num_pergroup=8, sw_type=5)
        with pytest.raises(ValueError):
            cls(32, sw_type=4)


def test_sw_counter_takes_sw_cfg():
    from dgvcc_amd import main
    from dgvcc_amd.models.trunks import SW_CFG, SWCounter_ResNet, SwitchWhiten2d
    model = SWCounter_ResNet(pretrained=False, sw_cfg={"sw_type": 5})
    layers = [m for m in model.modules() if isinstance(m, SwitchWhiten2d)]
    assert len(layers) == 7  # the stem and layer1-3's odd blocks
    for m in layers:
        assert m.sw_type == 5 and m.sw_mean_weight.shape == (5,) and m.sw_var_weight.shape == (5,)
        assert (m.momentum, m.T, m.tie_weight, m.affine) == (0.9, 5, False, True)
    via_main = main.get_model("sw", {"pretrained": False, "sw_cfg": {"sw_type": 5, "tie_weight": True}})
    assert all(m.sw_type == 5 and m.sw_var_weight is None
               for m in via_main.modules() if isinstance(m, SwitchWhiten2d))
    assert SW_CFG["sw_type"] == 2  # merged over, not written
    base = SWCounter_ResNet(pretrained=False)
    same = SWCounter_ResNet(pretrained=False, sw_cfg=None)
    assert list(base.state_dict()) == list(same.state_dict())
    assert all(m.sw_type == 2 for m in base.modules() if isinstance(m, SwitchWhiten2d))


NEW_SYMBOLS = ("dg_swx_save_size", "dg_swx_fwd", "dg_swx_fwd_stats", "dg_swx_fwd_finish", "dg_swx_bwd",
               "dg_swx_bwd_stats", "dg_swx_bwd_finish")


def test_new_entry_points_exported():
    from dgvcc_amd import _capi
    syms = _capi.exported_symbols()
    for name in NEW_SYMBOLS:
        assert name in syms and hasattr(_capi.lib(), name)
    assert _capi.lib().dg_version() == 8  # additive: the ABI version stays


def test_save_size_by_type():
    from dgvcc_amd import _capi
    L = _capi.lib()
    base = L.dg_sw_save_size(3, 64)
    assert L.dg_swx_save_size(3, 64, 2) == base
    assert L.dg_swx_save_size(3, 64, 3) == L.dg_swx_save_size(3, 64, 5) == base + 3 * 2 * 4
    assert L.dg_swx_save_size(3, 64, 4) == -1 and L.dg_swx_save_size(3, 60, 3) == -1
    assert L.dg_swx_save_size(0, 64, 3) == -1


def test_invalid_arguments_rejected_without_gpu():
    """Null pointers and sw_type 4 return DG_ERR_INVALID before any launch (no GPU here)."""
    from dgvcc_amd import _capi
    L = _capi.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; nothing may be launched or read
    p = ctypes.addressof(buf)
    N, HW, C, ld = 2, 15, 32, 32

    def holes(fn, args, idx):
        for t in (2, 3, 5):
            for i in idx:
                a = list(args(t, 0))
                a[i] = None
                assert fn(*a) == -1, (fn.__name__, t, i)
        assert fn(*args(4, 0)) == -1, fn.__name__
        assert fn(*args(0, 0)) == -1, fn.__name__

    # dg_swx_fwd_stats(dtype, x, ldx, N, HW, C, sw_type, save, moments, workspace, stream)
    holes(L.dg_swx_fwd_stats, lambda t, tie: (0, p, ld, N, HW, C, t, p, p, p, None), [1, 7, 8, 9])
    # dg_swx_fwd_finish(dtype, x, ldx, N, HW, C, sw_type, tie, T, eps, momentum, mean_w, var_w, gamma, beta,
    #                   running_mean, running_cov, training, act, count, moments, save, y, ldy, stream)
    fin = lambda t, tie: (0, p, ld, N, HW, C, t, tie, 5, 1e-5, 0.9, p, p, p, p, p, p, 1, 0, N, p, p, p, ld, None)  # noqa: E731
    holes(L.dg_swx_fwd_finish, fin, [1, 11, 12, 15, 16, 20, 21, 22])
    a = list(fin(3, 0))
    a[14] = None  # gamma without beta
    assert L.dg_swx_fwd_finish(*a) == -1
    a = list(fin(3, 0))
    a[19] = 0  # count
    assert L.dg_swx_fwd_finish(*a) == -1
    # dg_swx_fwd(dtype, x, ldx, N, HW, C, sw_type, tie, T, eps, momentum, mean_w, var_w, gamma, beta,
    #            running_mean, running_cov, training, act, save, y, ldy, workspace, stream)
    fwd = lambda t, tie: (0, p, ld, N, HW, C, t, tie, 5, 1e-5, 0.9, p, p, p, p, p, p, 1, 0, p, p, ld, p, None)  # noqa: E731
    holes(L.dg_swx_fwd, fwd, [1, 11, 12, 15, 16, 19, 20, 22])
    assert L.dg_swx_fwd(*[7 if i == 0 else v for i, v in enumerate(fwd(5, 0))]) == -1      # dtype
    assert L.dg_swx_fwd(*[40 if i == 5 else v for i, v in enumerate(fwd(5, 0))]) == -1      # C % 16
    assert L.dg_swx_fwd(*[512 if i == 5 else v for i, v in enumerate(fwd(5, 0))]) == -2     # C > 256
    assert L.dg_swx_fwd(*[9 if i == 8 else v for i, v in enumerate(fwd(5, 0))]) == -2       # T > 8
    # dg_swx_bwd_stats(dtype, gy, ldg, y, ldy, x, ldx, N, HW, C, sw_type, tie, T, eps, mean_w, var_w, gamma, act,
    #                  save, bmoments, dgamma, dbeta, workspace, stream)
    bst = lambda t, tie: (0, p, ld, p, ld, p, ld, N, HW, C, t, tie, 5, 1e-5, p, p, p, 1, p, p, p, p, p, None)  # noqa: E731
    holes(L.dg_swx_bwd_stats, bst, [1, 3, 5, 14, 15, 18, 19, 22])
    # dg_swx_bwd_finish(dtype, gy, ldg, y, ldy, x, ldx, N, HW, C, sw_type, tie, act, mean_w, var_w, save, count,
    #                   bmoments, dx, lddx, accumulate, dmean_w, dvar_w, workspace, stream)
    bfi = lambda t, tie: (0, p, ld, p, ld, p, ld, N, HW, C, t, tie, 1, p, p, p, N, p, p, ld, 0, p, p, p, None)  # noqa: E731
    holes(L.dg_swx_bwd_finish, bfi, [1, 3, 5, 13, 14, 15, 17, 18, 23])
    # dg_swx_bwd(dtype, gy, ldg, y, ldy, x, ldx, N, HW, C, sw_type, tie, T, eps, mean_w, var_w, gamma, act, save,
    #            dx, lddx, accumulate, dgamma, dbeta, dmean_w, dvar_w, workspace, stream)
    bwd = lambda t, tie: (0, p, ld, p, ld, p, ld, N, HW, C, t, tie, 5, 1e-5, p, p, p, 1, p, p, ld, 0, p, p, p, p, p,  # noqa: E731
                          None)
    holes(L.dg_swx_bwd, bwd, [1, 3, 5, 14, 15, 18, 19, 26])

    # tie_weight: a NULL var_w (and dvar_w) passes the pointer checks -- the call gets as far as the shape
    # check (C = 512 > 256: DG_ERR_UNSUPPORTED, still before any launch); untied, the same call is invalid
    C2 = 512
    for t in (2, 3, 5):
        for fn, args, iv, idv in ((L.dg_swx_fwd, fwd, 12, None), (L.dg_swx_fwd_finish, fin, 12, None),
                                  (L.dg_swx_bwd_stats, bst, 15, None), (L.dg_swx_bwd_finish, bfi, 14, 22),
                                  (L.dg_swx_bwd, bwd, 15, 25)):
            for tie, want in ((1, -2), (0, -1)):
                a = [C2 if v == C else v for v in args(t, tie)]  # C and the row strides
                a[iv] = None
                if idv is not None:
                    a[idv] = None
                assert fn(*a) == want, (fn.__name__, t, tie)


def test_kernels_wrapper_rejects_other_types():
    from dgvcc_amd import kernels as K
    with pytest.raises(K.DGError):
        K._sw_plain(4, False, None)
    assert K._sw_plain(2, False, object()) and not K._sw_plain(2, True, object())
    assert not K._sw_plain(2, False, None) and not K._sw_plain(5, False, object())
