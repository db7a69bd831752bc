"""DensityMapDataset / JHUDomainDataset, host half (no GPU): a sample's tap tables applied to its
source windows (tests/resize_ref.py arithmetic), then zero outside, block sum and flip, equal the
whole-frame path with the same Python-`random` draws (PIL `resize` of the full image, restatement
(b) of the full density map, renormalise, pad, crop, block sum, flip): the image bit for bit, the
density map within 1e-12 in float64.  Plus the entry points, file naming, signatures and the ABI."""
import inspect
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as R
from dgvcc_amd.utils.misc import get_padding

H, W = 60, 80
CROP = (32, 48)
DS = 2


def _frame(seed, n_points):
    rng = np.random.default_rng(seed)
    img = R.test_image(H, W, seed)
    pts = np.stack([rng.uniform(0, W - 1, n_points), rng.uniform(0, H - 1, n_points)], 1)
    d = np.zeros((H, W), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for x, y in pts:
        g = np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / 8.0)
        d += (g / g.sum()).astype(np.float32)
    return img, pts, d


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    """<root>/train: f001.jpg, f002.png (points), f003.png (no people), with `_dmap2` and `_dmap` maps, and the
    JHU domain lists."""
    root = str(tmp_path_factory.mktemp("den"))
    os.makedirs(os.path.join(root, "train"))
    os.makedirs(os.path.join(root, "domains"))
    names = []
    for name, ext, seed, n in (("f001", ".jpg", 1, 7), ("f002", ".png", 2, 12), ("f003", ".png", 3, 0)):
        img, pts, d = _frame(seed, n)
        fn = os.path.join(root, "train", name + ext)
        Image.fromarray(img).save(fn, quality=95)
        np.save(os.path.join(root, "train", name + ".npy"), pts.reshape(-1, 2))
        np.save(os.path.join(root, "train", name + "_dmap2.npy"), d)
        np.save(os.path.join(root, "train", name + "_dmap.npy"), d)
        names.append(fn)
    for phase in ("train", "val"):
        with open(os.path.join(root, "domains", f"fog_{phase}.txt"), "w") as f:
            f.write("\n".join(sorted(names)) + "\n")
    return root


def _den(root, pre_resize=1, ds=DS, **kw):
    from dgvcc_amd.datasets import DensityMapDataset
    d = DensityMapDataset(root, CROP, ds, "train", False, 1, pre_resize=pre_resize, **kw)
    d.img_fns = sorted(d.img_fns)
    return d


def _draws(seed, pre_resize):
    """The draws of one _train_transform call on an H x W frame, or None where the crop does not fit."""
    rnd = random.Random(seed)
    grey = rnd.random() > 0.88
    factor = pre_resize * (rnd.random() * 0.5 + 0.75)
    nh, nw = (int(H * factor), int(W * factor)) if factor != 1.0 else (H, W)
    padded = min(nw, nh) < min(CROP)
    ph, pw = (max(nh, CROP[0]), max(nw, CROP[1])) if padded else (nh, nw)
    if nh <= 0 or nw <= 0 or ph < CROP[0] or pw < CROP[1]:
        return None
    i, j = rnd.randint(0, ph - CROP[0]), rnd.randint(0, pw - CROP[1])
    return dict(grey=grey, factor=factor, nh=nh, nw=nw, padded=padded, i=i, j=j, ph=ph, pw=pw, flip=rnd.random() > 0.5)


def _seed_for(pred, pre_resize=1):
    for seed in range(5000):
        d = _draws(seed, pre_resize)
        if d is not None and pred(d):
            return seed
    raise AssertionError("no seed gives the case")


def _whole_frame(img, gt, dmap, pre_resize, ds):
    """The reference's _train_transform on whole frames (den_dataset.py:55-128), torchvision's tensor
    resize restated by R.aa_bilinear_resize; an empty map stays zero."""
    h, w = img.shape[:2]
    ch, cw = CROP
    pil = Image.fromarray(img)
    d = np.asarray(dmap, dtype=np.float64)
    if random.random() > 0.88:
        pil = pil.convert("L").convert("RGB")
    factor = pre_resize * (random.random() * 0.5 + 0.75)
    if factor != 1.0:
        w, h = int(w * factor), int(h * factor)
        pil = pil.resize((w, h))
        s = d.sum()
        d = R.aa_bilinear_resize(d, h, w)
        ns = d.sum()
        d = d * s / ns if ns != 0 else d
        gt = gt * factor
    arr = np.asarray(pil)
    if 1.0 * min(w, h) < min(ch, cw):
        (left, top, right, bottom), h, w = get_padding(h, w, ch, cw)
        arr = np.pad(arr, ((top, bottom), (left, right), (0, 0)))
        d = np.pad(d, ((top, bottom), (left, right)))
        if len(gt) > 0:
            gt = gt + [left, top]
    i, j = random.randint(0, h - ch), random.randint(0, w - cw)
    arr, d = arr[i:i + ch, j:j + cw], d[i:i + ch, j:j + cw]
    if len(gt) > 0:
        gt = gt - [j, i]
        gt = gt[(gt[:, 0] >= 0) * (gt[:, 0] <= cw) * (gt[:, 1] >= 0) * (gt[:, 1] <= ch)]
    else:
        gt = np.empty([0, 2])
    d = d.reshape(ch // ds, ds, cw // ds, ds).sum(axis=(1, 3))
    if len(gt) > 0:
        gt = gt / ds
    if random.random() > 0.5:
        arr, d = arr[:, ::-1], d[:, ::-1]
        if len(gt) > 0:
            gt[:, 0] = cw - gt[:, 0]
    return np.ascontiguousarray(arr), np.ascontiguousarray(d), torch.from_numpy(gt.copy()).float()


def _from_sample(s, ds):
    """What the device computes from a sample, in numpy: (uint8 crop [ch,cw,3], float64 map)."""
    r0, c0, oh, ow, grey, flip, ch, cw, down = s.geom.tolist()
    assert (ch, cw, down) == (*CROP, ds)
    inner = R.apply_u8(s.img_win.numpy(), s.img_hb.numpy(), s.img_hw.numpy(), s.img_vb.numpy(), s.img_vw.numpy(),
                       grey=bool(grey))
    assert inner.shape[:2] == (oh, ow)
    img = R.place(inner, r0, c0, ch, cw)
    img = img[:, ::-1] if flip else img
    m = R.apply_f64(s.map_win.numpy(), s.map_hb.numpy(), s.map_hw.numpy(), s.map_vb.numpy(), s.map_vw.numpy())
    m = R.block_sum_flip(R.place(m * s.scale, r0, c0, ch, cw), ds, bool(flip))
    return np.ascontiguousarray(img), m


CASES = {
    "padded": (0.4, lambda d: d["padded"] and d["nh"] < CROP[0] and d["nw"] < CROP[1]),
    "top_edge": (1, lambda d: not d["padded"] and d["i"] == 0 and d["factor"] < 1),
    "bottom_edge": (1, lambda d: not d["padded"] and d["i"] == d["nh"] - CROP[0] and d["factor"] > 1),
    "left_edge": (1, lambda d: not d["padded"] and d["j"] == 0 and d["factor"] > 1),
    "right_edge": (1, lambda d: not d["padded"] and d["j"] == d["nw"] - CROP[1] and d["factor"] < 1),
    "grey": (1, lambda d: d["grey"]),
    "flip": (1, lambda d: d["flip"] and not d["grey"]),
    "no_flip": (1, lambda d: not d["flip"]),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("index", [0, 1, 2])
def test_sample_equals_whole_frame(root, case, index):
    pre, pred = CASES[case]
    seed = _seed_for(pred, pre)
    ds = _den(root, pre_resize=pre)
    fn = ds.img_fns[index]
    img = np.asarray(Image.open(fn).convert("RGB"))
    gt = np.load(fn[:-4] + ".npy")
    dmap = np.load(fn[:-4] + "_dmap2.npy")
    random.seed(seed)
    want_img, want_map, want_gt = _whole_frame(img, gt, dmap, pre, DS)
    state = random.getstate()
    random.seed(seed)
    s = ds[index]
    assert random.getstate() == state  # the same number of draws
    got_img, got_map = _from_sample(s, DS)
    assert np.array_equal(got_img, want_img)
    assert np.isfinite(got_map).all() and np.abs(got_map - want_map).max() <= 1e-12
    assert torch.equal(s.points, want_gt)
    if index == 2:  # no people: empty points, an all-zero map that stays zero and finite
        assert s.points.shape == (0, 2) and not got_map.any() and np.isfinite(s.scale)
    # O(window): the windows hold only what the taps touch
    assert s.img_win.shape[0] <= H and s.img_win.shape[1] <= W


def test_collate_packs_descriptors(root):
    from dgvcc_amd.datasets import RawDenBatch
    from dgvcc_amd.datasets.augment import RESIZE_DESC
    ds = _den(root)
    random.seed(_seed_for(CASES["flip"][1]))
    samples = [ds[0], ds[1], ds[2]]
    raw = ds.collate(samples)
    assert isinstance(raw, RawDenBatch) and raw.crop_size == CROP and raw.downsample == DS
    D = {k: n for n, k in enumerate(RESIZE_DESC)}
    for src, desc, bounds, weights, pre in ((raw.img_src, raw.img_desc, raw.img_bounds, raw.img_weights, "img"),
                                            (raw.map_src, raw.map_desc, raw.map_bounds, raw.map_weights, "map")):
        assert not any(t.is_cuda for t in (src, desc, bounds, weights)) and desc.dtype == torch.int32
        for n, s in enumerate(samples):
            r = desc[n].tolist()
            win = getattr(s, pre + "_win")
            sh, sw = win.shape[:2]
            assert (r[D["sh"]], r[D["sw"]]) == (sh, sw)
            got = src[r[D["src"]]:r[D["src"]] + sh * sw].reshape(win.shape)
            assert torch.equal(got, win.to(got.dtype))
            for b0, w0, k, nrows, tb, tw in ((r[D["hb"]], r[D["hw"]], r[D["kh"]], r[D["ow"]], "_hb", "_hw"),
                                             (r[D["vb"]], r[D["vw"]], r[D["kv"]], r[D["oh"]], "_vb", "_vw")):
                assert torch.equal(bounds[b0:b0 + nrows], getattr(s, pre + tb))
                tw = getattr(s, pre + tw)
                assert torch.equal(weights[w0:w0 + nrows * k].reshape(nrows, k), tw.to(weights.dtype))
    assert raw.img_src.dtype == torch.uint8 and raw.img_weights.dtype == torch.int32
    assert raw.map_src.dtype == torch.float32 and raw.map_weights.dtype == torch.float32
    assert raw.scales.dtype == torch.float32 and raw.scales.shape == (3,) and len(raw.points) == 3


def test_get_dataset_entry_points(root):
    from dgvcc_amd import main as Mn
    from dgvcc_amd import main_base as Mb
    from dgvcc_amd.datasets import DensityMapDataset, JHUDomainDataset
    ds, collate = Mn.get_dataset("den", dict(root=root, crop_size=CROP, downsample=DS, is_grey=False, unit_size=1), "train")
    assert type(ds) is DensityMapDataset and len(ds) == 3
    assert collate is DensityMapDataset.collate
    ds, collate = Mb.get_dataset("jhu_domain", dict(root=root, domain_label="fog", crop_size=32, domain_type="weather",
                                                    domain=3, downsample=DS), "train")
    assert type(ds) is JHUDomainDataset and len(ds) == 3 and ds.crop_size == (32, 32)
    assert collate is JHUDomainDataset.collate
    with pytest.raises(NotImplementedError):
        Mn.get_dataset("bay", {}, "train")


def test_jhu_domain_sample_and_val(root):
    from dgvcc_amd.datasets import JHUDomainDataset
    ds = JHUDomainDataset(root, "fog", CROP, "weather", 3, DS, "train")
    random.seed(5)
    raw = ds.collate([ds[0], ds[1]])
    assert raw.img_desc.shape == (2, 16)
    val = JHUDomainDataset(root, "fog", CROP, "weather", 3, DS, "test", unit_size=16)
    img, rec, gt, name, padding = val[0]  # DenClsDataset._val_transform's sample
    assert img.dtype == torch.uint8 and img.shape[0] % 16 == 0 and img.shape[1] % 16 == 0 and name == "f001"


def test_file_naming(root, tmp_path):
    from dgvcc_amd.datasets import JHUDomainDataset
    train = os.path.join(root, "train")
    ds = _den(root)
    assert ds._paths(os.path.join(train, "f001.jpg"), ".jpg") == ("f001", os.path.join(train, "f001.npy"),
                                                               os.path.join(train, "f001_dmap2.npy"))
    # `_aug` copies share the original's points file, as in DenClsDataset
    assert ds._paths(os.path.join(train, "f001_aug.jpg"), ".jpg")[1] == os.path.join(train, "f001.npy")
    gt_dir = str(tmp_path / "gt")
    ds = _den(root, gt_dir=gt_dir, gen_root=str(tmp_path / "gen"))
    assert ds._paths(os.path.join(train, "f002.png"), ".png")[2] == os.path.join(gt_dir, "f002.npy")
    # a generated image <name>_<k>.png outside the root belongs to <root>/train/<name>
    assert ds._paths(str(tmp_path / "gen" / "f002_1.png"), ".png") == ("f002", os.path.join(train, "f002.npy"),
                                                                    os.path.join(gt_dir, "f002.npy"))
    ds = _den(root, gen_root=str(tmp_path / "gen"))
    assert ds._paths(str(tmp_path / "gen" / "f002_1.png"), ".png")[2] == os.path.join(train, "f002_dmap2.npy")
    jhu = JHUDomainDataset(root, "fog", CROP, "weather", 3, DS, "train")
    assert jhu._paths(os.path.join(train, "f003.png"), ".png")[2] == os.path.join(train, "f003_dmap.npy")
    assert jhu.img_fns == sorted(jhu.img_fns) and len(jhu) == 3


def test_constructor_signatures():
    from dgvcc_amd.datasets import DensityMapDataset, JHUDomainDataset

    def sig(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]

    E = inspect.Parameter.empty
    assert sig(DensityMapDataset) == [("root", E), ("crop_size", E), ("downsample", E), ("method", E), ("is_grey", E),
                                      ("unit_size", E), ("pre_resize", 1), ("roi_map_path", None), ("gt_dir", None),
                                      ("gen_root", None)]
    assert sig(JHUDomainDataset) == [("root", E), ("domain_label", E), ("crop_size", E), ("domain_type", E),
                                     ("domain", E), ("downsample", E), ("method", E), ("is_grey", False),
                                     ("unit_size", 0), ("pre_resize", 1)]


def test_crop_must_tile_downsample(root):
    from dgvcc_amd.datasets import DensityMapDataset
    with pytest.raises(ValueError, match="downsample"):
        DensityMapDataset(root, (32, 50), 4, "train", False, 1)


def test_abi_declares_and_exports():
    from dgvcc_amd import _capi
    protos = _capi.parse_header()
    assert _capi.header_abi_version() == 8
    assert len(protos["dg_resize_crop_u8"][1]) == 14 and len(protos["dg_resize_crop_f32"][1]) == 16
    assert len(protos["dg_resize_crop_workspace"][1]) == 3
    syms = set(_capi.exported_symbols())
    assert {"dg_resize_crop_u8", "dg_resize_crop_f32", "dg_resize_crop_workspace"} <= syms
    lib = _capi.lib()
    for name in ("dg_resize_crop_u8", "dg_resize_crop_f32", "dg_resize_crop_workspace"):
        assert getattr(lib, name) is not None
