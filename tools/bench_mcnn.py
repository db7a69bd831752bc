"""Measurements behind DESIGN.md §3.4 (small-channel convolution, MCNN), device events, warm-up
first, interleaved rounds, best and median of rounds:

  layers  forward, input gradient and weight gradient of MCNN's twelve convolutions at their
          batch-16, 768 x 1024 sizes (full, half and quarter resolution), per precision: ms,
          achieved FLOP/s against the matrix-pipe peak (157.3 TF f32 MFMA, 2.5 PF 16-bit) and
          algorithmic bytes/s (the unpadded operands once) against 8 TB/s, and the bound the layer
          sits under (the larger of the two roofline times).
  step    the MCNN DGTrainer 'simple' train step (MSELoss, fused AdamW), batch 16 at 768 x 1024,
          alternating in one process with the same network assembled from stock torch.nn modules
          (NCHW; bf16 through torch.autocast), the same pooled-ground-truth MSE and
          torch.optim.AdamW.

usage: bench_mcnn.py [layers] [step] [--precision fp32 bf16 fp16] [--batch 16]   (default: all)
"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dgvcc_amd import engine as E  # noqa: E402
from dgvcc_amd import kernels as K  # noqa: E402
from dgvcc_amd.kernels import Act  # noqa: E402

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HBM_PEAK = 8.0e12                      # bytes/s, MI355X HBM3E specification
MFMA_PEAK = {"fp32": 157.3e12, "bf16": 2.5e15, "fp16": 2.5e15}
# (Cin, Cout, k, resolution divisor) of MCNN's twelve convolutions
FORMS = [(3, 16, 9, 1), (16, 32, 7, 2), (32, 16, 7, 4), (16, 8, 7, 4),
         (3, 20, 7, 1), (20, 40, 5, 2), (40, 20, 5, 4), (20, 10, 5, 4),
         (3, 24, 5, 1), (24, 48, 3, 2), (48, 24, 3, 4), (24, 12, 3, 4)]


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


def bench_layers(precisions, batch, H=768, W=1024):
    for prec in precisions:
        dt = DT[prec]
        es = torch.tensor([], dtype=dt).element_size()
        print(f"layers {prec}: batch {batch} at {H}x{W}; peak {MFMA_PEAK[prec] / 1e12:.1f} TF, 8 TB/s", flush=True)
        print(f"  {'form':>12s} {'size':>9s} {'pass':>6s} {'best ms':>8s} {'med ms':>8s} {'TF/s':>7s} {'%peak':>6s} "
              f"{'TB/s':>6s} {'%HBM':>5s}  bound", flush=True)
        tot = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
        for C, Cout, k, div in FORMS:
            h, w = H // div, W // div
            conv = nn.Conv2d(C, Cout, k, padding=k // 2).to(DEV)
            layer = E.SmallConvLayer(conv, None, E.ACT_RELU)
            x = Act(torch.randn(batch, h, w, layer.Cp_in, device=DEV).to(dt))
            x.buf[..., C:] = 0
            y = Act(torch.empty(batch, h, w, layer.Cp_out, device=DEV, dtype=dt))
            g = Act(torch.randn(batch, h, w, layer.Cp_out, device=DEV).to(dt))
            g.buf[..., Cout:] = 0
            gx = Act(torch.empty_like(x.buf))
            dw = torch.empty(Cout, C, k, k, device=DEV)
            db = torch.empty(Cout, device=DEV)
            wp, wf = layer._pack(dt, False), layer._pack(dt, True)
            bias = conv.bias.detach()
            arms = {"fwd": lambda i: K.smallconv_fwd(x, wp, C, Cout, k, y, bias, relu=True),
                    "wgrad": lambda i: K.smallconv_wgrad(x, g, C, Cout, k, dw, db)}
            if C != 3:  # the image layers need no input gradient
                arms["dgrad"] = lambda i: K.smallconv_dgrad(g, wf, C, Cout, k, gx)
            M = batch * h * w
            flops = 2.0 * M * C * Cout * k * k
            nbytes = {"fwd": es * M * (C + Cout), "dgrad": es * M * (C + Cout), "wgrad": es * M * (C + Cout)}
            for name, ms in rounds(arms, 3).items():
                best, med = min(ms), statistics.median(ms)
                tf, tb = flops / best / 1e9, nbytes[name] / best / 1e9
                t_f, t_b = flops / MFMA_PEAK[prec], nbytes[name] / HBM_PEAK
                bound = "HBM" if t_b > t_f else "MFMA"
                tot[name] += best
                print(f"  {f'{C}->{Cout} k{k}':>12s} {f'{h}x{w}':>9s} {name:>6s} {best:8.3f} {med:8.3f} {tf:7.1f} "
                      f"{100 * tf * 1e12 / MFMA_PEAK[prec]:6.1f} {tb:6.2f} {100 * tb * 1e12 / HBM_PEAK:5.1f}  {bound} "
                      f"(roofline {max(t_f, t_b) * 1e3:.3f} ms)", flush=True)
            del x, y, g, gx
        print(f"  sums of best: fwd {tot['fwd']:.2f} ms, dgrad {tot['dgrad']:.2f} ms, wgrad {tot['wgrad']:.2f} ms",
              flush=True)
        torch.cuda.empty_cache()


def stock_mcnn():
    """The same network from stock torch.nn modules (this tool's own restatement)."""
    def column(cfg):
        mods, cin = [], 3
        for i, (cout, k) in enumerate(cfg):
            mods += [nn.Conv2d(cin, cout, k, padding=k // 2), nn.ReLU(inplace=True)] + ([nn.MaxPool2d(2)] if i < 2 else [])
            cin = cout
        return nn.Sequential(*mods)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.branch1 = column([(16, 9), (32, 7), (16, 7), (8, 7)])
            self.branch2 = column([(20, 7), (40, 5), (20, 5), (10, 5)])
            self.branch3 = column([(24, 5), (48, 3), (24, 3), (12, 3)])
            self.fuse = nn.Sequential(nn.Conv2d(30, 1, 1))

        def forward(self, x):
            return self.fuse(torch.cat((self.branch1(x), self.branch2(x), self.branch3(x)), 1))
    return Net()


def bench_step(precisions, batch, H=768, W=1024, warm=2, n=5):
    from oracle import dg_oracle as O
    from dgvcc_amd.losses import MSELoss
    from dgvcc_amd.models.baselines import MCNN
    from dgvcc_amd.optim import AdamW
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    data = O.synthetic_batch(batch, H, W, seed=5, with_dmap=False)
    data = (data[0].to(DEV), data[1].to(DEV), tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in data[2]))
    img, gt = data[0], data[2][1].float()
    for prec in precisions:
        m = MCNN(load_weights=True)
        sd = O.seeded_state_dict(m.state_dict())
        m.load_state_dict(sd)
        m = m.to(DEV).set_precision(prec).train()
        opt = AdamW(m.parameters(), lr=1e-5, weight_decay=1e-4)
        ref = stock_mcnn()
        ref.load_state_dict(sd)
        ref = ref.to(DEV).train()
        ropt = torch.optim.AdamW(ref.parameters(), lr=1e-5, weight_decay=1e-4)
        tgt = 16 * F.avg_pool2d(gt, 4) * 1000

        def stock_step(i):
            ropt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=DT[prec], enabled=prec != "fp32"):
                pred = ref(img)
            loss = ((pred.float() - tgt) ** 2).mean()
            loss.backward()
            ropt.step()

        with tempfile.TemporaryDirectory() as td:
            cwd = os.getcwd()
            os.chdir(td)
            try:
                tr = DGTrainer(2112, "bench", torch.device(DEV), 1000, 10000, "simple")
                arms = {"dgvcc_amd MCNN": lambda i: tr.train_step(m, MSELoss(), opt, data, 0), "stock torch.nn": stock_step}
                for _ in range(warm):
                    for fn in arms.values():
                        fn(0)
                res = rounds(arms, 1, n)
            finally:
                os.chdir(cwd)
        ours, theirs = res["dgvcc_amd MCNN"], res["stock torch.nn"]
        for k, ms in res.items():
            print(f"step {prec}: {k:16s} batch {batch} at {H}x{W}: best {min(ms):8.1f} ms  median "
                  f"{statistics.median(ms):8.1f} ms  rounds {' '.join(f'{v:.1f}' for v in ms)}", flush=True)
        print(f"step {prec}: stock / dgvcc_amd = {min(theirs) / min(ours):.2f} (best), "
              f"{statistics.median(theirs) / statistics.median(ours):.2f} (median); peak memory "
              f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)
        del m, opt, ref, ropt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["layers", "step"])
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"], choices=list(DT))
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcnn.py needs a GPU: nothing is measured without one")
    for part in a.parts:
        {"layers": bench_layers, "step": bench_step}[part](a.precision, a.batch)
