"""Measurement behind DESIGN.md §3.5 (BL's VGG19 counter), device events, warm-up first,
interleaved rounds, best and median of rounds:

  step    the BL_VGG DGTrainer 'simple' train step (MSELoss on the ground truth sum-pooled onto the
          1/8 grid, fused AdamW), batch 16 at 768 x 1024, alternating in one process with the same
          network assembled from stock torch.nn modules (NCHW; bf16 through torch.autocast), the
          same pooled-ground-truth MSE and torch.optim.AdamW.

Prints one line per arm and precision with the step time and frames/s, and the ratio of the two.
The stock fp32 arm runs about 5 s per step on an MI355X (plus its convolution search in the warm-up),
so a run of both precisions takes several minutes: `--precision fp32` and `--precision bf16` can be
run as two invocations, each ratio staying within one process.

usage: bench_blvgg.py [--precision fp32 bf16 fp16] [--batch 16] [--size 768 1024] [--rounds 5]
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

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CFG_E = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512]


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
    """{name: [ms per round]} with the arms interleaved."""
    out = {k: [] for k in arms}
    for _ in range(n):
        for k, fn in arms.items():
            out[k].append(timed(fn, reps))
    return out


def stock_blvgg():
    """The same network from stock torch.nn modules (this tool's own restatement): VGG19 "E" features,
    bilinear x2 with align_corners=True, 512->256->128 in 3x3, 1x1 128->1, abs."""
    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            mods, cin = [], 3
            for v in CFG_E:
                if v == "M":
                    mods.append(nn.MaxPool2d(2, 2))
                else:
                    mods += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
                    cin = v
            self.features = nn.Sequential(*mods)
            self.reg_layer = nn.Sequential(nn.Conv2d(512, 256, 3, padding=1), nn.ReLU(inplace=True),
                                           nn.Conv2d(256, 128, 3, padding=1), nn.ReLU(inplace=True),
                                           nn.Conv2d(128, 1, 1))

        def forward(self, x):
            x = F.interpolate(self.features(x), scale_factor=2, mode="bilinear", align_corners=True)
            return torch.abs(self.reg_layer(x))
    return Net()


def bench_step(precisions, batch, H, W, warm=2, n=5):
    from oracle import dg_oracle as O
    from dgvcc_amd.losses import MSELoss
    from dgvcc_amd.models.baselines import BL_VGG
    from dgvcc_amd.optim import AdamW
    from dgvcc_amd.trainers.dgtrainer import DGTrainer
    data = O.synthetic_batch(batch, H, W, seed=5, with_dmap=False)
    data = (data[0].to(DEV), data[1].to(DEV), tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in data[2]))
    img, gt = data[0], data[2][1].float()
    for prec in precisions:
        m = BL_VGG()
        sd = O.seeded_state_dict(m.state_dict())
        m.load_state_dict(sd)
        m = m.to(DEV).set_precision(prec).train()
        opt = AdamW(m.parameters(), lr=1e-5, weight_decay=1e-4)
        ref = stock_blvgg()
        ref.load_state_dict(sd)
        ref = ref.to(DEV).train()
        ropt = torch.optim.AdamW(ref.parameters(), lr=1e-5, weight_decay=1e-4)
        tgt = 64 * F.avg_pool2d(gt, 8) * 1000

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
                arms = {"dgvcc_amd BL_VGG": lambda i: tr.train_step(m, MSELoss(), opt, data, 0),
                        "stock torch.nn": stock_step}
                for _ in range(warm):
                    for fn in arms.values():
                        fn(0)
                res = rounds(arms, 1, n)
            finally:
                os.chdir(cwd)
        ours, theirs = res["dgvcc_amd BL_VGG"], res["stock torch.nn"]
        for k, ms in res.items():
            best, med = min(ms), statistics.median(ms)
            print(f"step {prec}: {k:16s} batch {batch} at {H}x{W}: best {best:8.1f} ms ({1e3 * batch / best:7.1f} "
                  f"frames/s)  median {med:8.1f} ms ({1e3 * batch / med:7.1f} frames/s)  "
                  f"rounds {' '.join(f'{v:.1f}' for v in ms)}", flush=True)
        print(f"step {prec}: stock / dgvcc_amd = {min(theirs) / min(ours):.2f} (best), "
              f"{statistics.median(theirs) / statistics.median(ours):.2f} (median); peak memory "
              f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)
        del m, opt, ref, ropt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"], choices=list(DT))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=[768, 1024], metavar=("H", "W"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blvgg.py needs a GPU: nothing is measured without one")
    bench_step(a.precision, a.batch, a.size[0], a.size[1], n=a.rounds)
