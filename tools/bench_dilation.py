"""Measurements behind DESIGN.md §3.3 (dilated convolution by phase decomposition), device events,
warm-up first, interleaved rounds, best and median of rounds:

  layout  dg_space_to_batch / dg_batch_to_space at [16, 96, 128, C] (C = 512, 64), d = 2, fp32 and
          bf16: ms and achieved bytes/s (algorithmic bytes: one read + one write of the tensor),
          beside a plain device copy and the BN apply of the same tensor.  The operands rotate over
          several buffers so that no pass finds its input in the Infinity Cache.
  layers  forward + backward of CSRNet's six back-end layers (d = 2) on [16, 96, 128, 512] in
          phase-resident mode, beside the same six layers as dense 3x3 layers on [64, 48, 64, 512],
          alternating in one process.
  step    CSRNet DGTrainer 'simple' step (MSELoss, fused AdamW), batch 16 at 768 x 1024.

usage: bench_dilation.py [layout] [layers] [step] [--precision fp32 bf16]   (default: all)
"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from dgvcc_amd import engine as E  # noqa: E402
from dgvcc_amd import kernels as K  # noqa: E402
from dgvcc_amd.kernels import Act  # noqa: E402

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E specification


def timed(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(reps):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def rounds(arms, reps, n=5):
    """{name: [ms per round]} with the arms interleaved (one warm-up call each first)."""
    for fn in arms.values():
        fn(0)
    out = {k: [] for k in arms}
    for _ in range(n):
        for k, fn in arms.items():
            out[k].append(timed(fn, reps))
    return out


def show(name, ms, nbytes=None):
    best, med = min(ms), statistics.median(ms)
    rate = f"  {nbytes / best / 1e9:7.2f} TB/s best ({100 * nbytes / (best * 1e-3) / HBM_PEAK:4.1f}% of 8 TB/s)" \
        if nbytes else ""
    print(f"  {name:34s} best {best:8.3f} ms  median {med:8.3f} ms{rate}", flush=True)


def bench_layout(precisions):
    N, H, W, d, nbuf = 16, 96, 128, 2, 4
    for prec in precisions:
        dt = DT[prec]
        es = torch.tensor([], dtype=dt).element_size()
        for C in (512, 64):
            img = [Act(torch.randn(N, H, W, C, device=DEV).to(dt)) for _ in range(nbuf)]
            ph = [Act(torch.randn(*K.phase_shape(N, H, W, d), C, device=DEV).to(dt)) for _ in range(nbuf)]
            st = torch.stack([torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                              torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.1])
            arms = {
                "dg_space_to_batch": lambda i: K.space_to_batch(img[i % nbuf], d, ph[i % nbuf]),
                "dg_batch_to_space": lambda i: K.batch_to_space(ph[i % nbuf], d, img[i % nbuf]),
                "torch copy_": lambda i: ph[i % nbuf].buf.copy_(ph[(i + 1) % nbuf].buf),
                "dg_bn_apply (ReLU)": lambda i: K.bn_apply(img[i % nbuf], st, 1, img[(i + 1) % nbuf]),
            }
            print(f"layout {prec} [{N}, {H}, {W}, {C}] d={d} ({N * H * W * C * es / 1e6:.1f} MB each way)")
            for k, ms in rounds(arms, 20).items():
                show(k, ms, 2.0 * N * H * W * C * es)
            del img, ph


def _backend(dilated: bool):
    cfg, cin, mods = [512, 512, 512, 256, 128, 64], 512, []
    g = torch.Generator().manual_seed(0)
    for v in cfg:
        conv = nn.Conv2d(cin, v, 3, padding=2 if dilated else 1, dilation=2 if dilated else 1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(v, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
            conv.bias.zero_()
        mods += [conv, nn.ReLU(inplace=True)]
        cin = v
    return nn.Sequential(*mods).to(DEV)


def bench_layers(precisions):
    from dgvcc_amd.models import plans2 as P2
    N, H, W = 16, 96, 128
    for prec in precisions:
        dt = DT[prec]
        dil, dense = P2.ChainPlan(_backend(True)), P2.ChainPlan(_backend(False))
        x = Act(torch.randn(N, H, W, 512, device=DEV).to(dt))
        xs = Act(torch.empty(*K.phase_shape(N, H, W, 2), 512, device=DEV, dtype=dt))
        K.space_to_batch(x, 2, xs)
        g = Act(torch.randn(N, H, W, 64, device=DEV).to(dt))
        gs = Act(torch.empty(*K.phase_shape(N, H, W, 2), 64, device=DEV, dtype=dt))
        K.space_to_batch(g, 2, gs)

        def step(plan, xin, gin):
            E.invalidate_frozen()
            tape = {}
            plan.run(Act(xin.buf), dt, True, tape)
            plan.back(tape, Act(gin.buf))

        def fwd(plan, xin):
            plan.run(Act(xin.buf), dt, True, None)

        arms = {
            "dilated, resident  fwd+bwd": lambda i: step(dil, x, g),
            "dense on phases    fwd+bwd": lambda i: step(dense, xs, gs),
            "dilated, resident  fwd": lambda i: fwd(dil, x),
            "dense on phases    fwd": lambda i: fwd(dense, xs),
        }
        print(f"layers {prec}: six back-end layers, [{N}, {H}, {W}, 512] d=2 vs dense [{xs.N}, {xs.H}, {xs.W}, 512]")
        res = rounds(arms, 5)
        for k, ms in res.items():
            show(k, ms)
        keys = list(res)
        print(f"  difference fwd+bwd: best {min(res[keys[0]]) - min(res[keys[1]]):.3f} ms, median "
              f"{statistics.median(res[keys[0]]) - statistics.median(res[keys[1]]):.3f} ms;  fwd: best "
              f"{min(res[keys[2]]) - min(res[keys[3]]):.3f} ms", flush=True)
        gx = Act(torch.empty_like(x.buf))
        y = Act(torch.empty_like(g.buf))
        own = {
            "space_to_batch x [..512]": lambda i: K.space_to_batch(x, 2, xs),
            "batch_to_space y [..64]": lambda i: K.batch_to_space(gs, 2, y),
            "space_to_batch g [..64]": lambda i: K.space_to_batch(g, 2, gs),
            "batch_to_space gx [..512]": lambda i: K.batch_to_space(xs, 2, gx),
        }
        tot = 0.0
        for k, ms in rounds(own, 20).items():
            show(k, ms)
            tot += min(ms)
        print(f"  the four layout passes of a forward + backward: {tot:.3f} ms (best)", flush=True)


def bench_step(precisions, batch=16, H=768, W=1024, warm=2, steps=5):
    from oracle import dg_oracle as O
    from dgvcc_amd.losses import MSELoss
    from dgvcc_amd.models.baselines import CSRNet
    from dgvcc_amd.optim import AdamW
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    data = O.synthetic_batch(batch, H, W, seed=5, with_dmap=False)
    data = (data[0].to(DEV), data[1].to(DEV), tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in data[2]))
    for prec in precisions:
        m = CSRNet()
        m.load_state_dict(O.seeded_state_dict(m.state_dict()))
        m = m.to(DEV).set_precision(prec).train()
        opt = AdamW(m.parameters(), lr=1e-5, weight_decay=1e-4)
        with tempfile.TemporaryDirectory() as td:
            cwd = os.getcwd()
            os.chdir(td)
            try:
                tr = DGTrainer(2112, "bench", torch.device(DEV), 1000, 10000, "simple")
                for _ in range(warm):
                    tr.train_step(m, MSELoss(), opt, data, 0)
                ms = [timed(lambda i: tr.train_step(m, MSELoss(), opt, data, 0), 1) for _ in range(steps)]
            finally:
                os.chdir(cwd)
        print(f"step {prec}: CSRNet simple-mode train step, batch {batch} at {H}x{W}: best {min(ms):.1f} ms "
              f"median {statistics.median(ms):.1f} ms  ({batch / statistics.median(ms) * 1e3:.1f} frames/s median), "
              f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)
        del m, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["layout", "layers", "step"])
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"], choices=list(DT))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dilation.py needs a GPU: nothing is measured without one")
    for part in a.parts:
        {"layout": bench_layout, "layers": bench_layers, "step": bench_step}[part](a.precision)
