"""float64 restatements of the first layer of stem.hip (3x3 pad-1 convolution 3 -> 64 channels, its weight
gradient, the segment walk and the launch rule of the statistics partials), written from the comment blocks of
stem.hip and include/dgvcc.h.  Plain torch on the CPU; the BatchNorm side is tests/bn_ref.py.
tests/test_stem_ref_cpu.py checks them against F.conv2d / torch.nn.grad.conv2d_weight and asserts the input
conditions of every case; tests/test_stem_kernels_gpu.py checks the kernels against them.

Images are NCHW f32 [N, 3, H, W], filters torch layout [64, 3, 3, 3], activations NHWC [N, H, W, 64].
"""
import collections
import functools

import torch
import torch.nn.functional as F

import bn_ref as R

F32, BF16 = R.F32, R.BF16
CO = 64
EPS = 1e-5

# the planted channels of every case
CH_ZERO, CH_BIAS100, CH_NOBIAS, CH_NEGGAMMA = 5, 17, 30, 44
PLANTED = (CH_ZERO, CH_BIAS100, CH_NOBIAS, CH_NEGGAMMA)

SMALL = ((1, 1, 64), (3, 2, 64), (2, 3, 128), (1, 5, 192))
BWD_ONLY = ((2, 3, 32), (1, 4, 96), (1, 2, 160))
LONG = (2, 33, 4096)
FWD_SHAPES = SMALL + (LONG,)
BWD_SHAPES = SMALL + BWD_ONLY + (LONG,)


def _d(t):
    return t.detach().double().cpu()


def rounded(t, dt):
    """t as the kernels of storage type dt read it (bf16: rounded to nearest even), in float64."""
    return _d(t) if dt == F32 else _d(t.float().to(dt))


# ---------------------------------------------------------------- convolution --
def _taps(img):
    """The 9 shifted views [N, 3, H, W] of the zero-padded image: tap (r, s) of pixel (p, q) is
    img[p + r - 1, q + s - 1]."""
    N, _, H, W = img.shape
    xp = F.pad(img, (1, 1, 1, 1))
    return [((r, s), xp[:, :, r:r + H, s:s + W]) for r in range(3) for s in range(3)]


def conv(img, w, bias=None):
    """z[n, p, q, co] = sum over the 27 taps of img[n, c, p + r - 1, q + s - 1] w[co, c, r, s] + bias[co]
    (zero padding), NHWC, and the per-element sum of the absolute terms sum |x w| + |b|."""
    img, w = _d(img), _d(w)
    N, _, H, W = img.shape
    z = torch.zeros(N, H, W, CO, dtype=torch.float64)
    a = torch.zeros_like(z)
    for (r, s), x in _taps(img):
        for c in range(3):
            xc = x[:, c, :, :, None]
            z.addcmul_(xc, w[:, c, r, s])
            a.addcmul_(xc.abs(), w[:, c, r, s].abs())
    if bias is not None:
        z += _d(bias)
        a += _d(bias).abs()
    return z, a


def wgrad(img, dz):
    """dw[co, c, r, s] = sum over the pixels of dz[n, p, q, co] img[n, c, p + r - 1, q + s - 1], and the sum
    of the absolute terms sum |dz x| per element of dw."""
    img, dz = _d(img), _d(dz)
    dw = torch.zeros(CO, 3, 3, 3, dtype=torch.float64)
    a = torch.zeros_like(dw)
    d2 = dz.reshape(-1, CO)
    for (r, s), x in _taps(img):
        x2 = x.permute(0, 2, 3, 1).reshape(-1, 3)
        dw[:, :, r, s] = d2.T @ x2
        a[:, :, r, s] = d2.abs().T @ x2.abs()
    return dw, a


def wgrad_pixels(img, pix, dz_rows):
    """wgrad() of a dz that is dz_rows [P, 64] on the flat pixels pix [P] and zero elsewhere."""
    img, dz_rows = _d(img), _d(dz_rows)
    N, _, H, W = img.shape
    dw = torch.zeros(CO, 3, 3, 3, dtype=torch.float64)
    a = torch.zeros_like(dw)
    for (r, s), x in _taps(img):
        x2 = x.permute(0, 2, 3, 1).reshape(-1, 3)[pix]
        dw[:, :, r, s] = dz_rows.T @ x2
        a[:, :, r, s] = dz_rows.abs().T @ x2.abs()
    return dw, a


# ---------------------------------------------------------------- segments -----
def segment_pixels(N, H, W, seg, width):
    """Flat pixel indices (n H + p) W + q of segment `seg`: `width` consecutive pixels of one image row
    (width 64 in the forward kernels, 32 in the backward ones), rows walked in order."""
    spr = W // width
    assert W % width == 0 and 0 <= seg < N * H * spr
    row_id, k = divmod(seg, spr)
    return row_id * W + k * width + torch.arange(width)


def fwd_grid(nseg):
    return max(1, min(512, -(-nseg // 4)))


def part_counts(N, H, W):
    """The pixel count n of every statistics part row: 64 x the number of forward segments of block b, grid =
    max(1, min(512, ceil(nseg / 4))) blocks of 4 waves, wave w of block b taking the segments
    4 b + w + k 4 grid (k = 0, 1, ...) below nseg."""
    nseg = N * H * (W // 64)
    grid = fwd_grid(nseg)
    out = torch.zeros(grid, dtype=torch.float64)
    for b in range(grid):
        for w in range(4):
            first = 4 * b + w
            if first < nseg:
                out[b] += 64 * (1 + (nseg - 1 - first) // (4 * grid))
    return out


def wave_segments(nseg, block, wave, grid=None):
    """The segments one wave walks, in order."""
    grid = fwd_grid(nseg) if grid is None else grid
    return list(range(4 * block + wave, nseg, 4 * grid))


# ---------------------------------------------------------------- ReLU margin --
def uncertain(z, scale, shift):
    """Mask [M, 64] of the elements whose float64 pre-activation z scale + shift is within 2^-23 (|z scale| +
    |shift|) of zero: an f32 evaluation may put them on either side."""
    zs, sf = R.pre(z, scale, shift)
    return (zs + sf).abs() <= 2.0 ** -23 * (zs.abs() + sf.abs())


def margin_ok(z, scale, shift):
    """The condition of every case: at most 1 in 10^5 of the elements uncertain, the constant zero-filter
    channel left out when (and only when) its pre-activation is at least 0.5 from zero.  Returns (ok,
    number of uncertain elements counted, elements)."""
    u = uncertain(z, scale, shift)
    zs, sf = R.pre(z, scale, shift)
    far = bool(((zs + sf)[:, CH_ZERO].abs() >= 0.5).all())
    if far:
        u = u.clone()
        u[:, CH_ZERO] = False
    n = int(u.sum())
    return n * 100000 <= u.numel(), n, u.numel()


# ---------------------------------------------------------------- cases --------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def plant_borders(img):
    """Distinct large values in the first / last rows and columns of every image and channel: 3 .. 8.25 in
    magnitude against an interior in [-1, 1], so a halo read from the wrong row, column or image moves z by
    units, thousands of times the f32 bound and tens of times a bf16 ulp, while a channel's deviation stays
    comparable with its mean (bias ~ 2) and the relative bounds on the statistics keep their meaning."""
    N, C, H, W = img.shape
    n = torch.arange(N, dtype=torch.float32).view(N, 1, 1)
    c = torch.arange(C, dtype=torch.float32).view(1, C, 1)
    wob_w = 0.1 * torch.cos(torch.arange(W, dtype=torch.float32) * 0.7).view(1, 1, W)
    wob_h = 0.1 * torch.cos(torch.arange(H, dtype=torch.float32) * 0.9).view(1, 1, H)
    img[:, :, 0, :] = 3.0 + 0.5 * n + 0.25 * c + wob_w
    img[:, :, H - 1, :] = -(4.25 + 0.5 * n + 0.25 * c) + wob_w
    img[:, :, :, 0] = 5.5 + 0.5 * n + 0.25 * c + wob_h
    img[:, :, :, W - 1] = -(6.75 + 0.5 * n + 0.25 * c) + wob_h
    return img


@functools.lru_cache(maxsize=None)
def make_case(N, H, W, seed=0):
    """Seeded inputs of one shape: img (borders planted), filter w, bias ~ 2 +- 0.1, gamma, beta, running rows
    and the upstream gradient g [N, H, W, 64] (f32; the bf16 route rounds img, w and g).  Planted channels:
    CH_ZERO a zero filter (z = bias everywhere; beta 0.75 keeps its constant pre-activation away from zero),
    CH_BIAS100 a bias of 100 with a filter of scale 1e-3 (beta 25 keeps it active everywhere: with |z scale| and
    |shift| in the thousands its pre-activation would otherwise pass within 2^-23 of them near zero in about
    one element in a thousand, and in bf16 its z is constant),
    CH_NOBIAS zero bias with an ordinary filter, CH_NEGGAMMA a negative gamma."""
    g = _gen(seed or 1000 + 7 * N * H * W)
    img = plant_borders((torch.randn(N, 3, H, W, generator=g) * 0.5).clamp(-1, 1))
    w = torch.randn(CO, 3, 3, 3, generator=g) / 27 ** 0.5
    b = torch.randn(CO, generator=g) * 0.1 + 2.0
    gamma = torch.rand(CO, generator=g) + 0.5
    beta = torch.randn(CO, generator=g) * 0.1
    w[CH_ZERO] = 0.0
    w[CH_BIAS100] = torch.randn(3, 3, 3, generator=g) * 1e-3
    b[CH_BIAS100] = 100.0
    b[CH_NOBIAS] = 0.0
    gamma[CH_NEGGAMMA] = -gamma[CH_NEGGAMMA]
    beta[CH_ZERO], beta[CH_BIAS100] = 0.75, 25.0
    return dict(img=img, w=w, bias=b, gamma=gamma, beta=beta, eps=EPS,
                rm0=torch.randn(CO, generator=g), rv0=0.5 + torch.rand(CO, generator=g),
                g=0.3 + torch.randn(N, H, W, CO, generator=g))


@functools.lru_cache(maxsize=4)
def ref_conv(shape, dt):
    """(z, sum |terms|) of the case's bias-free convolution on the operands as dt reads them (shared, not
    modified); with_bias() adds the bias."""
    i = make_case(*shape)
    return conv(rounded(i["img"], dt), rounded(i["w"], dt), None)


def with_bias(shape, dt, use_bias=True):
    z, a = ref_conv(shape, dt)
    if not use_bias:
        return z, a
    b = _d(make_case(*shape)["bias"])
    return z + b, a + b.abs()


def stored_z(shape, dt):
    """The float64 z (with bias) rounded to the storage type: what a correct forward stores, up to its bound."""
    return with_bias(shape, dt)[0].float().to(dt)


def ref_stats(shape, dt):
    """float64 statistics of stored_z, scale / shift rounded to the f32 rows the kernels keep."""
    i = make_case(*shape)
    z = stored_z(shape, dt)
    st = R.stats(z, i["gamma"], i["beta"], i["eps"])
    return z, st, st["scale"].float(), st["shift"].float()


Variant = collections.namedtuple("Variant", "name img rows cols")


def wrong_halo_variants(img):
    """Images a wrong halo rule would effectively read, with the pixels (rows / columns) whose z it moves: a
    border row or column taken for padding, and the rows of the neighbouring image read in place of the
    padding above and below."""
    N, _, H, W = img.shape
    out = []
    if H > 1:
        for name, row, hit in (("row 0 as padding", 0, 1), ("last row as padding", H - 1, H - 2)):
            v = img.clone()
            v[:, :, row, :] = 0.0
            out.append(Variant(name, v, [hit], None))
    for name, col, hit in (("column 0 as padding", 0, 1), ("last column as padding", W - 1, W - 2)):
        v = img.clone()
        v[:, :, :, col] = 0.0
        out.append(Variant(name, v, None, [hit]))
    return out
