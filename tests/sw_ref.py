"""Float64 restatement of SwitchWhiten2d for every variant the operator documents: sw_type 2
(BW + IW), 3 (+ LN), 5 (+ BN + IN + LN), tied or separate mixing weights, with or without the
affine.  Written from the operator's formulas, in plain differentiable torch (autograd gives the
gradients), and pinned to the reference operator's own float64 results by tests/golden/sw_types.npz
(test_sw_types_cpu.py); the GPU tests compare the kernels against it.

With x [N, C, H, W] cut into G = C / 16 groups of c = 16 channels:

  batch      mu_bn [G, c], cov_bn [G, c, c]   over N H W   (eval: the running statistics)
  instance   mu_in [N, G, c], cov_in [N, G, c, c]   over H W, divisor H W
  layer      mean_ln [N], var_ln [N]   over C H W, the variance unbiased (divisor C H W - 1),
             from the input in eval mode too; var_ln enters as var_ln I in every group
  BN / IN    var_bn = diag(cov_bn), var_in = diag(cov_in)   (sw_type 5)

  m = softmax(sw_mean_weight);  v = softmax(sw_var_weight), or v = m when the weights are tied

  sw_type 2:  mean = m0 mu_bn + m1 mu_in
              cov  = v0 cov_bn + v1 cov_in + eps I
  sw_type 3:  mean = m0 mu_bn + m1 mu_in + m2 mean_ln
              cov  = v0 cov_bn + v1 cov_in + v2 var_ln I + eps I
  sw_type 5:  mean = (m0 + m2) mu_bn + (m1 + m3) mu_in + m4 mean_ln
              cov  = v0 cov_bn + v1 cov_in + v0 var_bn + v1 var_in + v4 var_ln I + eps I
              (the variance side reuses v0 and v1; v2 and v3 act through the normalisation only)

  Newton-Schulz: A = cov / tr(cov), P_0 = I, P_{k+1} = 1.5 P_k - 0.5 P_k^3 A, W = P_T / sqrt(tr(cov))
  y = W (x - mean), then * weight + bias per channel when the operator has an affine.
  Training updates running <- momentum * running + (1 - momentum) * batch statistic.
"""
import torch

GROUP = 16
PARAMS = ("sw_mean_weight", "sw_var_weight", "weight", "bias")


def state_keys(tie, affine):
    """The operator's state_dict keys, in registration order."""
    keys = ["sw_mean_weight"]
    if not tie:
        keys.append("sw_var_weight")
    if affine:
        keys += ["weight", "bias"]
    return keys + ["running_mean", "running_cov"]


def make_params(C, sw_type, tie, affine, gen):
    """Seeded non-trivial parameters and running statistics (float32 values), as the fixture's
    generator and the tests draw them: absent parameters are absent from the dict."""
    G = C // GROUP
    p = {"sw_mean_weight": torch.randn(sw_type, generator=gen)}
    if not tie:
        p["sw_var_weight"] = torch.randn(sw_type, generator=gen)
    if affine:
        p["weight"] = torch.rand(C, generator=gen) + 0.5
        p["bias"] = torch.randn(C, generator=gen) * 0.1
    p["running_mean"] = torch.randn(G, GROUP, 1, generator=gen) * 0.1
    a = torch.randn(G, GROUP, GROUP, generator=gen) * 0.3
    p["running_cov"] = a @ a.transpose(1, 2) + torch.eye(GROUP)
    return p


def make_input(shape, gen):
    x = torch.randn(*shape, generator=gen) * 2 + 0.5
    x = x + torch.randn(shape[0], shape[1], 1, 1, generator=gen)  # per-channel offsets: LN != IN
    gy = torch.randn(*shape, generator=gen)
    return x, gy


def switch_whiten(x, p, training, sw_type=2, T=5, eps=1e-5, momentum=0.9):
    """y for x [N, C, H, W] (float64).  p: dict of float64 tensors; a missing / None sw_var_weight is
    tie_weight, a missing / None weight is affine=False.  In training the running statistics of p
    are replaced by their updated values (new tensors: the caller's originals are not written)."""
    if sw_type not in (2, 3, 5):
        raise ValueError(sw_type)
    N, C, H, W = x.shape
    c, G = GROUP, C // GROUP
    xg = x.reshape(N, G, c, H * W)
    mu_in = xg.mean(-1)                                             # [N, G, c]
    xc = xg - mu_in[..., None]
    cov_in = xc @ xc.transpose(-1, -2) / (H * W)                    # [N, G, c, c]
    if training:
        xb = xg.permute(1, 2, 0, 3).reshape(G, c, N * H * W)
        mu_bn = xb.mean(-1)                                         # [G, c]
        xbc = xb - mu_bn[..., None]
        cov_bn = xbc @ xbc.transpose(-1, -2) / (N * H * W)          # [G, c, c]
        p["running_mean"] = momentum * p["running_mean"] + (1 - momentum) * mu_bn.detach()[..., None]
        p["running_cov"] = momentum * p["running_cov"] + (1 - momentum) * cov_bn.detach()
    else:
        mu_bn = p["running_mean"][..., 0]
        cov_bn = p["running_cov"]
    eye = torch.eye(c, dtype=x.dtype)
    m = torch.softmax(p["sw_mean_weight"], 0)
    vw = p.get("sw_var_weight")
    v = m if vw is None else torch.softmax(vw, 0)
    if sw_type in (3, 5):
        flat = x.reshape(N, -1)
        mean_ln = flat.mean(-1)[:, None, None]                                        # [N, 1, 1]
        var_ln = (flat - flat.mean(-1, keepdim=True)).pow(2).sum(-1) / (C * H * W - 1)  # unbiased
        ln_cov = var_ln[:, None, None, None] * eye
    if sw_type == 2:
        mean = m[0] * mu_bn + m[1] * mu_in
        cov = v[0] * cov_bn + v[1] * cov_in
    elif sw_type == 3:
        mean = m[0] * mu_bn + m[1] * mu_in + m[2] * mean_ln
        cov = v[0] * cov_bn + v[1] * cov_in + v[2] * ln_cov
    else:
        mean = (m[0] + m[2]) * mu_bn + (m[1] + m[3]) * mu_in + m[4] * mean_ln
        cov = (v[0] * cov_bn + v[1] * cov_in + v[0] * (cov_bn * eye) + v[1] * (cov_in * eye) + v[4] * ln_cov)
    cov = cov + eps * eye
    tr = torch.diagonal(cov, dim1=-2, dim2=-1).sum(-1)[..., None, None]
    A = cov / tr
    P = eye.expand(N, G, c, c)
    for _ in range(T):
        P = 1.5 * P - 0.5 * (P @ P @ P) @ A
    Wm = P / tr.sqrt()
    y = (Wm @ (xg - mean[..., None])).reshape(N, C, H, W)
    if p.get("weight") is not None:
        y = y * p["weight"].view(1, C, 1, 1) + p["bias"].view(1, C, 1, 1)
    return y


def run(x, gy, params, sw_type, act=0, T=5, eps=1e-5, momentum=0.9, training=True):
    """Forward + backward in float64 from float32-valued inputs (training=False: the running statistics
    as constants of the graph).  Returns a dict: y, gx, grad__<param>, post__running_mean /
    post__running_cov."""
    p = {k: v.double().clone().requires_grad_(k in PARAMS) for k, v in params.items()}
    xr = x.double().clone().requires_grad_(True)
    y = switch_whiten(xr, p, training, sw_type, T, eps, momentum)
    if act:
        y = torch.relu(y)
    y.backward(gy.double())
    out = {"y": y.detach(), "gx": xr.grad}
    for k in PARAMS:
        if k in params:
            out["grad__" + k] = p[k].grad
    out["post__running_mean"] = p["running_mean"].detach()
    out["post__running_cov"] = p["running_cov"].detach()
    return out


def run_eval(x, params, sw_type, act=0, T=5, eps=1e-5):
    p = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        y = switch_whiten(x.double(), p, False, sw_type, T, eps)
    return torch.relu(y) if act else y


# The fixture's variants (tests/golden/sw_types.npz): sw_type 3 and 5 with every tie / affine
# combination, and sw_type 2 wherever it leaves the SW counter's own configuration.
VARIANTS = [(t, tie, aff) for t in (3, 5) for tie in (False, True) for aff in (True, False)] + \
           [(2, True, True), (2, False, False), (2, True, False)]
FIXTURE_SHAPE = (2, 32, 3, 5)


def variant_name(sw_type, tie, affine):
    return f"t{sw_type}_tie{int(tie)}_aff{int(affine)}"


def fixture_case(sw_type, tie, affine):
    """(x, gy, params) of one fixture variant: seeded, so the fixture stores results only."""
    gen = torch.Generator().manual_seed(1000 + 100 * sw_type + 10 * int(tie) + int(affine))
    params = make_params(FIXTURE_SHAPE[1], sw_type, tie, affine, gen)
    x, gy = make_input(FIXTURE_SHAPE, gen)
    return x, gy, params
