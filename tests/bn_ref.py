"""float64 restatements of the BatchNorm passes of norm.hip (statistics, apply, backward, the forms fused
with the 2x2 max pool, the SyncBatchNorm phases), written from the formulas in include/dgvcc.h and the
comment blocks of norm.hip.  Plain torch on the CPU, no project imports: tests/test_bn_ref_cpu.py checks
them against float64 autograd of F.batch_norm -> ReLU -> channel dropout -> F.max_pool2d,
tests/test_bn_kernels_gpu.py checks the kernels against them.

Activations are NHWC [N, H, W, C] (any leading shape: the last dimension is the channel, everything before
it pixels); per-channel rows are [C]; a Dropout2d mask is [N, C] (0 or 1 / (1 - p)) over HW pixels per
image.  Every function takes the stored inputs (already rounded to the storage type) and, where the
kernel takes them, the kernel's own stored f32 statistics rows, and computes in float64.  NaNs are not
modelled.
"""
import collections
import functools

import torch

# ulp(1) of the storage types
EPS_T = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


def _d(t):
    return None if t is None else t.detach().double().cpu()


def _rows(t):
    return _d(t).reshape(-1, t.shape[-1])


def drop_rows(drop, HW):
    """[N, C] -> [N * HW, C]: the mask of pixel p is drop[p // HW]."""
    return None if drop is None else _d(drop).repeat_interleave(HW, 0)


def _one(v, like):
    return torch.ones_like(like) if v is None else _d(v)


def _zero(v, like):
    return torch.zeros_like(like) if v is None else _d(v)


# ---------------------------------------------------------------- statistics --
def stats(z, gamma, beta, eps):
    """Training statistics per channel: mean, biased var, invstd = 1 / sqrt(var + eps), scale = gamma invstd,
    shift = beta - mean scale; `unbiased` = var M / (M - 1) feeds the running update (M = 1: the biased
    value, as bn_stats_finalize)."""
    x = _rows(z)
    M = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = _one(gamma, mean) * invstd
    shift = _zero(beta, mean) - mean * scale
    return dict(M=M, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift,
                unbiased=var * M / (M - 1) if M > 1 else var)


def running(old, new, momentum):
    return (1.0 - momentum) * _d(old) + momentum * _d(new)


# ---------------------------------------------------------------- apply -------
def pre(z, scale, shift):
    """(z scale, shift) as rows: the two terms of the pre-activation (NULL rows: identity)."""
    x = _rows(z)
    return x * _one(scale, x[0]), _zero(shift, x[0]).expand_as(x)


def apply(z, scale, shift, act, drop=None, HW=None):
    """y = act(z scale + shift) drop[n, c]."""
    zs, sf = pre(z, scale, shift)
    y = zs + sf
    if act == 1:
        y = y.clamp_min(0.0)
    if drop is not None:
        y = y * drop_rows(drop, HW)
    return y.reshape(z.shape)


def masked(g, z, scale, shift, act, drop=None, HW=None):
    """g' rows: g drop, zeroed where z scale + shift <= 0 when act = 1."""
    gp = _rows(g).clone()
    if drop is not None:
        gp = gp * drop_rows(drop, HW)
    if act == 1:
        zs, sf = pre(z, scale, shift)
        gp[(zs + sf) <= 0] = 0.0
    return gp


def xhat(z, mean, invstd):
    x = _rows(z)
    return (x - _zero(mean, x[0])) * _one(invstd, x[0])


def sums3(g, z, mean, invstd, scale, shift, act, drop=None, HW=None):
    """(sum g', sum g' xhat, sum xhat) [3][C], and the sums of the absolute terms [3][C] that bound their
    rounding."""
    gp, xh = masked(g, z, scale, shift, act, drop, HW), xhat(z, mean, invstd)
    return (torch.stack([gp.sum(0), (gp * xh).sum(0), xh.sum(0)]),
            torch.stack([gp.abs().sum(0), (gp * xh).abs().sum(0), xh.abs().sum(0)]))


def apply_coef(g, z, mean, invstd, scale, shift, act, k1, k2, k3, drop=None, HW=None):
    """dz = k1 g' - k2 xhat - k3, and the per-element sum of the absolute terms."""
    gp, xh = masked(g, z, scale, shift, act, drop, HW), xhat(z, mean, invstd)
    k1, k2, k3 = _d(k1), _d(k2), _d(k3)
    dz = k1 * gp - k2 * xh - k3
    terms = (k1 * gp).abs() + (k2 * xh).abs() + k3.abs()
    return dz.reshape(z.shape), terms.reshape(z.shape)


def bwd(g, z, gamma, mean, invstd, scale, shift, act, drop=None, HW=None):
    """The BN(+ReLU, +dropout) backward of bn_bwd_partial / bn_bwd_finalize / bn_bwd_apply.
    k1 = gamma invstd, k2 = k1 sum g' xhat / M, k3 = k1 sum g' / M, dz = k1 g' - k2 xhat - k3,
    dgamma = sum g' xhat, dbeta = sum g', dbias = -k2 sum xhat (sum dz less its dbeta term: bn_bwd_finalize).
    mean = invstd = None: no normalisation, dz = g', dbeta = dbias = sum g', dgamma = 0."""
    s, a = sums3(g, z, mean, invstd, scale, shift, act, drop, HW)
    M = _rows(z).shape[0]
    out = dict(M=M, sums=s, abs_sums=a)
    if invstd is None:
        gp = masked(g, z, scale, shift, act, drop, HW)
        out.update(dz=gp.reshape(z.shape), terms=gp.abs().reshape(z.shape), dgamma=torch.zeros_like(s[0]),
                   dbeta=s[0], dbias=s[0], k1=torch.ones_like(s[0]), k2=torch.zeros_like(s[0]),
                   k3=torch.zeros_like(s[0]), xhat=xhat(z, None, None))
        return out
    k1 = _one(gamma, s[0]) * _d(invstd)
    k2, k3 = k1 * s[1] / M, k1 * s[0] / M
    dz, terms = apply_coef(g, z, mean, invstd, scale, shift, act, k1, k2, k3, drop, HW)
    out.update(dz=dz, terms=terms, dgamma=s[1], dbeta=s[0], dbias=-k2 * s[2], k1=k1, k2=k2, k3=k3,
               xhat=xhat(z, mean, invstd))
    return out


# ---------------------------------------------------------------- 2x2 pool ----
def windows(t):
    """[N, H, W, C] -> [N, H/2, W/2, 4, C]: the four values of each 2x2 window in scan order
    ((0,0), (0,1), (1,0), (1,1))."""
    N, H, W, C = t.shape
    return t.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def unwindows(w):
    N, Ho, Wo, _, C = w.shape
    return w.reshape(N, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)


def first_max(w):
    """Index [N, Ho, Wo, C] of the first maximum, in scan order, of the four window values."""
    m = w[..., 0, :].clone()
    k = torch.zeros(m.shape, dtype=torch.long)
    for j in range(1, 4):
        up = w[..., j, :] > m
        m = torch.where(up, w[..., j, :], m)
        k = torch.where(up, torch.full_like(k, j), k)
    return k


def pool_fwd(y):
    """yp = the first max of the four stored y of each window (y: the stored activation)."""
    w = windows(_d(y))
    return torch.gather(w, 3, first_max(w).unsqueeze(3)).squeeze(3)


def pool_route(gp, gd, y):
    """Upstream gradient of y [N, H, W, C]: gp routed to the first max of the stored y (+ gd)."""
    w = windows(_d(y))
    g = torch.zeros_like(w)
    g.scatter_(3, first_max(w).unsqueeze(3), _d(gp).unsqueeze(3))
    g = unwindows(g)
    return g if gd is None else g + _d(gd)


def pool_bwd(gp, gd, y, z, gamma, mean, invstd, scale, shift, act, drop=None):
    """Pooled backward: bwd() of the routed gradient (times drop, ReLU-masked, inside bwd)."""
    return bwd(pool_route(gp, gd, y), z, gamma, mean, invstd, scale, shift, act, drop, z.shape[1] * z.shape[2])


# ---------------------------------------------------------------- sync phases -
def row(z):
    """A rank's (n, mean, M2) row [3][C]."""
    x = _rows(z)
    mean = x.mean(0)
    return torch.stack([torch.full_like(mean, float(x.shape[0])), mean, ((x - mean) ** 2).sum(0)])


def merge(rows):
    """Chan et al. merge of (n, mean, M2) rows [R][3][C] in order (rows with n = 0 are skipped)."""
    rows = _d(rows)
    n, mean, m2 = rows[0, 0].clone(), rows[0, 1].clone(), rows[0, 2].clone()
    for r in rows[1:]:
        nb = r[0]
        if float(nb.max()) == 0.0:
            continue
        nt = n + nb
        d = r[1] - mean
        mean = mean + d * nb / nt
        m2 = m2 + r[2] + d * d * n * nb / nt
        n = nt
    return torch.stack([n, mean, m2])


def stats_from_rows(rows, gamma, beta, eps):
    """Global statistics from the ranks' rows: the same quantities as stats()."""
    n, mean, m2 = merge(rows)
    M = int(n[0])
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = _one(gamma, mean) * invstd
    return dict(M=M, mean=mean, var=var, invstd=invstd, scale=scale, shift=_zero(beta, mean) - mean * scale,
                unbiased=var * M / (M - 1) if M > 1 else var)


def count_row(M, C):
    """The fourth row of a rank's sums: its pixel count as hi + lo parts, each exact in f32."""
    r = torch.zeros(C, dtype=torch.float64)
    r[0], r[1] = float(M - M % 4096), float(M % 4096)
    return r


def sums4(g, z, mean, invstd, scale, shift, act, drop=None, HW=None):
    """A rank's backward sums [4][C] (and the absolute-term sums [3][C])."""
    s, a = sums3(g, z, mean, invstd, scale, shift, act, drop, HW)
    return torch.cat([s, count_row(_rows(z).shape[0], s.shape[1])[None]]), a


def finalize_sync(loc, glob, M_local, M_global, gamma, invstd):
    """k1 / k2 / k3 from the global sums over the global count (M_global None: glob[3][0] + glob[3][1]),
    dgamma / dbeta from the local sums, dbias = k1 sum g'_l - k2 sum xhat_l - M_l k3; `terms` the sum of
    the absolute terms of dbias."""
    loc, glob = _d(loc), _d(glob)
    Mg = float(glob[3, 0] + glob[3, 1]) if M_global is None else float(M_global)
    k1 = _one(gamma, loc[0]) * _d(invstd)
    k2, k3 = k1 * glob[1] / Mg, k1 * glob[0] / Mg
    return dict(k1=k1, k2=k2, k3=k3, dgamma=loc[1], dbeta=loc[0],
                dbias=k1 * loc[0] - k2 * loc[2] - M_local * k3,
                terms=(k1 * loc[0]).abs() + (k2 * loc[2]).abs() + (M_local * k3).abs())


# ---------------------------------------------------------------- conditions --
def relu_margin(z, scale, shift):
    """min over the elements of |z scale + shift| / (|z scale| + |shift|): the ReLU cases need >= 1e-3, so
    that no f32 evaluation of the pre-activation can disagree with the reference about its sign."""
    zs, sf = pre(z, scale, shift)
    return float(((zs + sf).abs() / (zs.abs() + sf.abs())).min())


def _near(w, zw, dt, ulps):
    """[N, Ho, Wo, C]: some pair of the window's four values is neither exactly equal (duplicated z, or
    both zero) nor more than `ulps` ulp of the storage type apart."""
    bad = torch.zeros(w[..., 0, :].shape, dtype=torch.bool)
    tiny = 2.0 ** -24 if dt == torch.float16 else 0.0
    for i in range(4):
        for j in range(i + 1, 4):
            a, b = w[..., i, :], w[..., j, :]
            eq = (zw[..., i, :] == zw[..., j, :]) | (a == b)
            bad |= ~eq & ((a - b).abs() <= ulps * (EPS_T[dt] * torch.maximum(a.abs(), b.abs()) + tiny))
    return bad


def pool_gaps(z, y, dt):
    """(windows with a pair neither exactly equal nor > 4 ulp of the storage type apart, fraction of
    (window, channel) entries whose maximal z is duplicated) of a pooled case; y: the float64 reference."""
    zw = windows(_d(z))
    bad = _near(windows(_d(y)), zw, dt, 4.0)
    tied = (zw == zw.max(3, keepdim=True).values).sum(3) >= 2
    return int(bad.sum()), float(tied.double().mean())


def drop_ok(drop, p):
    """Zeros and 1 / (1 - p) only, and every image holds a dropped and a kept channel."""
    d = _d(drop)
    keep = 1.0 / (1.0 - p)
    vals = bool(((d == 0) | ((d - keep).abs() <= 1e-6 * keep)).all())
    return vals and bool(((d == 0).any(1) & (d != 0).any(1)).all())


# ---------------------------------------------------------------- input makers -
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_drop(N, C, p, g):
    d = (torch.rand(N, C, generator=g) >= p).float() / (1.0 - p)
    for n in range(N):  # one dropped and one kept channel in every image
        i, j = torch.randperm(C, generator=g)[:2].tolist()
        d[n, i], d[n, j] = 0.0, 1.0 / (1.0 - p)
    return d


def make_case(N, H, W, C, dt, seed, act=0, p=None, pooled=False, mean0=5.0, std0=3.0, small_gamma=True,
              tie_frac=0.4, eps=1e-5):
    """Seeded stored inputs of one case: z [N, H, W, C] (storage type dt), gamma / beta / running rows
    (f32), the upstream gradients g (and gp for a pooled case), a Dropout2d mask for p.

    Channel c is centred at s_c mean0 (s_c = +-1) and beta_c = -s_c U(0.25, 1.5), so shift = beta - mean
    scale does not cancel and a relative bound on it is meaningful; every fourth gamma is 100 times
    smaller (not in pooled cases, where it would put the window values within the storage type's
    rounding of each other).  ReLU cases: elements with |z scale + shift| < 2e-3 (|z scale| + |shift|) are
    resampled until none is left.  Pooled cases: in tie_frac of the (window, channel) entries the
    window's largest z is duplicated into another position (the first-max rule's test), and entries with
    two values neither equal nor 8 ulp apart are resampled."""
    g = _gen(seed)
    sgn = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)

    def draw(shape):
        return (sgn * mean0 + std0 * torch.randn(*shape, C, generator=g)).to(dt)

    z = draw((N, H, W))
    gamma = torch.rand(C, generator=g) + 0.5
    if small_gamma and not pooled:
        gamma[3::4] *= 0.01
    drop = make_drop(N, C, p, g) if p is not None else None
    planted = partner = None
    if pooled:
        planted = torch.rand(N, H // 2, W // 2, C, generator=g) < tie_frac
        partner = torch.randint(1, 4, (N, H // 2, W // 2, C), generator=g)

    def plant(z, where):
        zw = windows(z.double())
        m = first_max(zw)
        j = (m + partner) % 4
        top = torch.gather(zw, 3, m.unsqueeze(3))
        zw = torch.where((torch.arange(4).view(1, 1, 1, 4, 1) == j.unsqueeze(3)) & where.unsqueeze(3), top, zw)
        return unwindows(zw).to(dt)

    if pooled:
        z = plant(z, planted)
    for _ in range(100):
        mean = z.double().reshape(-1, C).mean(0)
        bsgn = -torch.sign(mean)
        bsgn[bsgn == 0] = 1.0
        beta = (bsgn * (0.25 + 1.25 * torch.rand(C, generator=_gen(seed + 1)).double())).float()
        st = stats(z, gamma, beta, eps)
        bad = torch.zeros(z.shape, dtype=torch.bool)
        if act == 1:
            zs, sf = pre(z, st["scale"], st["shift"])
            bad |= ((zs + sf).abs() < 2e-3 * (zs.abs() + sf.abs())).reshape(z.shape)
        if pooled:
            y = apply(z, st["scale"], st["shift"], act)  # without drop: the case holds with and without it
            near = _near(windows(y), windows(z.double()), dt, 8.0)
            near |= windows(bad.double()).sum(3) > 0
            bad = unwindows(near.unsqueeze(3).expand(-1, -1, -1, 4, -1).double()) > 0
        if not bad.any():
            break
        z = torch.where(bad, draw((N, H, W)), z)
        if pooled:
            z = plant(z, planted & near)
    else:
        raise RuntimeError("make_case: the input conditions were not met")
    rs = torch.sign(mean).float()
    rs[rs == 0] = 1.0
    out = dict(z=z, gamma=gamma, beta=beta, drop=drop, eps=eps, act=act, p=p, HW=H * W,
               rm0=rs * (0.5 + torch.rand(C, generator=g)), rv0=0.5 + torch.rand(C, generator=g),
               g=(0.3 + torch.randn(N, H, W, C, generator=g)).to(dt))
    if pooled:
        out["gp"] = (0.3 + torch.randn(N, H // 2, W // 2, C, generator=g)).to(dt)
    return out


def make_stress(M, C, dt, seed, mean0, std0, delta):
    """Statistics stress input z [1, M, 1, C]: channels of mean mean0 and deviation std0 whose first pixel
    (the kernels' shift) sits delta deviations from the mean (delta = 0: within one deviation).  Returns
    z and, per channel, the measured delta_c = |z_0 - mean_c| / std_c of the stored values."""
    g = _gen(seed)
    z = mean0 + std0 * torch.randn(M, C, generator=g)
    z[0] = mean0 + std0 * (delta if delta else (torch.rand(C, generator=g) - 0.5))
    z = z.to(dt)
    x = z.double()
    return z.reshape(1, M, 1, C), (x[0] - x.mean(0)).abs() / x.std(0, unbiased=False)


# ---------------------------------------------------------------- the cases ---
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
VEC = {F32: 4, BF16: 8, F16: 8}

Case = collections.namedtuple("Case", "name N H W C dt act p pooled mean0 std0 tie_frac seed")


def _case(name, N, H, W, C, dt, act, p=None, pooled=False, mean0=5.0, std0=3.0, tie_frac=0.4, seed=0):
    return Case(f"{name}-{IDS[dt]}-C{C}-act{act}", N, H, W, C, dt, act, p, pooled, mean0, std0, tie_frac,
                seed or 100 + 7 * N * H * W + C + act)


def plain_cases():
    """The shapes of tests/test_bn_kernels_gpu.py's un-pooled cases (see its table)."""
    out = []
    for dt in DTYPES:
        V = VEC[dt]
        out.append(_case("M1", 1, 1, 1, V, dt, 1, mean0=0.0, std0=0.02))  # variance 0: y = beta
        out.append(_case("M7", 1, 7, 1, V, dt, 1))
        out.append(_case("M63", 1, 63, 1, 64, dt, 1))
        out.append(_case("M65", 1, 65, 1, 64, dt, 1))
        out.append(_case("M3137", 1, 3137, 1, 1024 if dt == F32 else 2048, dt, 1))
        out.append(_case("M65603", 1, 65603, 1, V, dt, 1))
        for act in (0, 1):
            out.append(_case("drop7x9", 3, 7, 9, 64, dt, act, p=0.3))
            out.append(_case("drop1x41", 3, 1, 41, 64, dt, act, p=0.3))
    return out


def slice_case(dt):
    return _case("slice", 1, 5, 13, 64, dt, 1, p=0.3)


def nonorm_case(dt):
    return _case("nonorm", 1, 5, 13, 64, dt, 0, p=0.3, seed=77)


def m3137_case(dt, act=1):
    return _case("M3137", 1, 3137, 1, 64, dt, act)


def sync_case(dt, act=1):
    """M1 = 65 and M2 = 3072 pixels as the first and the last 3072 rows of one 3137-pixel batch."""
    return _case("sync", 1, 3137, 1, 64, dt, act, seed=991)


def pooled_cases():
    out = []
    for dt in DTYPES:
        for act in (0, 1):
            for C in (8, 64):
                out.append(_case("pool14x22", 3, 14, 22, C, dt, act, p=0.3, pooled=True))
            out.append(_case("pool2x2", 1, 2, 2, VEC[dt], dt, act, p=0.3, pooled=True, tie_frac=0.6))
    out.append(_case("pool66x64", 2, 66, 64, 1024, F32, 1, p=0.3, pooled=True))
    return out


def sync_pool_case(dt):
    """Three 14x22 images: the 'ranks' hold the first one and the other two."""
    return _case("syncpool", 3, 14, 22, 64, dt, 1, pooled=True, seed=503)


@functools.lru_cache(maxsize=4)
def inputs(case):
    """The stored inputs of a case (shared, not modified)."""
    return make_case(case.N, case.H, case.W, case.C, case.dt, case.seed, case.act, case.p, case.pooled,
                     case.mean0, case.std0, tie_frac=case.tie_frac)
