"""Plain restatements of the two resamplers behind DensityMapDataset's random rescale, written
per output sample with Python loops and independent of dgvcc_amd/datasets/den_dataset.py:

(a) PIL `Image.resize` (bicubic) on 8-bit images (Resample.c): a = -0.5, scale = in / out,
    support = 2 * max(scale, 1); window xmin = max(int(c - support + .5), 0) to
    min(int(c + support + .5), in); weights normalised in double, rounded half away from zero to
    22 fractional bits; accumulator seeded with 1 << 21, arithmetic shift by 22, clip to 0..255;
    horizontal pass into a uint8 image, then vertical pass; a pass whose axis keeps its size is
    skipped.
(b) ATen's antialiased bilinear (`interpolate(mode='bilinear', align_corners=False,
    antialias=True)`): the same windows with the triangle filter and support max(scale, 1), in
    float64.

Also the arithmetic of (a) / (b) applied with given tap tables to a source window (what the
device kernels do with a sample's tables), and the tail of the pipeline (zero outside, block sum,
flip).
"""
import numpy as np

BITS = 22


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def triangle(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def coeffs(n_in, n_out, filt, base_support):
    """[(xmin, [normalised double weights])] for every output sample."""
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = base_support * fscale
    ss = 1.0 / fscale
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        k = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        out.append((xmin, k))
    return out


def to_fixed(w):
    return int(-0.5 + w * (1 << BITS)) if w < 0 else int(0.5 + w * (1 << BITS))


def _pass_u8(img, table):
    """Resample axis 1 of uint8 [H, W, C] with [(xmin, int weights)]."""
    H, _, C = img.shape
    out = np.empty((H, len(table), C), dtype=np.uint8)
    src = img.astype(np.int64)
    for x, (xmin, k) in enumerate(table):
        acc = np.full((H, C), 1 << (BITS - 1), dtype=np.int64)
        for j, w in enumerate(k):
            acc += src[:, xmin + j, :] * w
        out[:, x, :] = np.clip(acc >> BITS, 0, 255)
    return out


def pil_bicubic_resize(img, out_h, out_w):
    """uint8 [H, W, 3] -> uint8 [out_h, out_w, 3] as Image.resize((out_w, out_h))."""
    H, W = img.shape[:2]
    if out_w != W:
        img = _pass_u8(img, [(m, [to_fixed(w) for w in k]) for m, k in coeffs(W, out_w, bicubic, 2.0)])
    if out_h != H:
        t = _pass_u8(img.transpose(1, 0, 2), [(m, [to_fixed(w) for w in k]) for m, k in coeffs(H, out_h, bicubic, 2.0)])
        img = t.transpose(1, 0, 2)
    return np.ascontiguousarray(img)


def _pass_f64(d, table):
    out = np.zeros((d.shape[0], len(table)), dtype=np.float64)
    for x, (xmin, k) in enumerate(table):
        for j, w in enumerate(k):
            out[:, x] += d[:, xmin + j] * w
    return out


def aa_bilinear_resize(d, out_h, out_w):
    """float64 [H, W] -> [out_h, out_w]; horizontal pass, then vertical."""
    d = np.asarray(d, dtype=np.float64)
    H, W = d.shape
    if out_w != W:
        d = _pass_f64(d, coeffs(W, out_w, triangle, 1.0))
    if out_h != H:
        d = _pass_f64(d.T, coeffs(H, out_h, triangle, 1.0)).T
    return np.ascontiguousarray(d)


def axis_sums(n_in, n_out):
    """[n_in]: the total weight each input sample has over all outputs of (b)."""
    s = np.zeros(n_in, dtype=np.float64)
    if n_in == n_out:
        return s + 1.0
    for xmin, k in coeffs(n_in, n_out, triangle, 1.0):
        for j, w in enumerate(k):
            s[xmin + j] += w
    return s


# ---- a sample's tables applied to its window ---------------------------------------------------
def _table(bounds, weights):
    bounds, weights = np.asarray(bounds), np.asarray(weights)
    return [(int(s), [weights[n, j].item() for j in range(int(c))]) for n, (s, c) in enumerate(bounds)]


def apply_u8(win, hb, hw, vb, vw, grey=False):
    """uint8 window [sh, sw, 3] -> uint8 [oh, ow, 3] in the arithmetic of (a)."""
    win = np.asarray(win)
    if grey:  # PIL convert('L').convert('RGB')
        w64 = win.astype(np.int64)
        L = (19595 * w64[..., 0] + 38470 * w64[..., 1] + 7471 * w64[..., 2] + 0x8000) >> 16
        win = np.repeat(L[..., None], 3, axis=2).astype(np.uint8)
    t = _pass_u8(win, _table(hb, hw))
    return np.ascontiguousarray(_pass_u8(t.transpose(1, 0, 2), _table(vb, vw)).transpose(1, 0, 2))


def apply_f64(win, hb, hw, vb, vw):
    """window [mh, mw] -> float64 [oh, ow] in the arithmetic of (b) with the given weights."""
    t = _pass_f64(np.asarray(win, dtype=np.float64), _table(hb, np.asarray(hw, dtype=np.float64)))
    return np.ascontiguousarray(_pass_f64(t.T, _table(vb, np.asarray(vw, dtype=np.float64))).T)


def place(inner, r0, c0, ch, cw):
    """[oh, ow, ...] set into a zero [ch, cw, ...] crop at (r0, c0)."""
    out = np.zeros((ch, cw) + inner.shape[2:], dtype=inner.dtype)
    out[r0:r0 + inner.shape[0], c0:c0 + inner.shape[1]] = inner
    return out


def block_sum_flip(d, ds, flip):
    h, w = d.shape
    d = d.reshape(h // ds, ds, w // ds, ds).sum(axis=(1, 3))
    return d[:, ::-1].copy() if flip else d


def normalise(img_u8):
    """ToTensor + Normalize(0.5, 0.5) of uint8 [H, W, 3] -> torch f32 [3, H, W]."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(img_u8)).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)


def test_image(H, W, seed):
    """uint8 [H, W, 3] noise with saturated 0 / 255 blocks (the clip of (a) is exercised)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    img[H // 5:H // 2, W // 6:W // 2] = 255
    img[H // 2:H - 2, W // 2:W - 3] = 0
    img[2:6, W - 8:W - 2] = 255
    return img


test_image.__test__ = False  # a helper, not a pytest test

CASES = [(37, 53, 0.75), (37, 53, 1.2499), (64, 48, 0.6), (41, 33, 1.4), (50, 70, 1.0003), (23, 19, 0.31),
         (30, 30, 2.5)]
