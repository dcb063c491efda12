"""Times of the soft-target CE kernels and the device Mixup beside what they replace (profiles/soft_ce.md): HIP events around `--iters`
back-to-back calls after `--warmup`, alternating the candidates over `--rounds`; bytes from the shapes; one JSON line per candidate.

  xfm_mixup at [128, 3, 224, 224]          against  xf = x.flip(0).mul_(1 - lam); x.mul_(lam).add_(xf)   (timm Mixup._mix_batch)
  xfm_ce_smooth_fwd + bwd at R = 960, V = 50265  beside   xfm_ce_fwd + bwd at the same shape

    python tools/bench_soft_ce.py [--iters 50] [--warmup 10] [--rounds 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xfm_amd import functional as Fx  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s (MI355X data sheet)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_ce: needs the GPU (no fallback)")
    dev = "cuda"
    B, C, H, W = 128, 3, 224, 224
    x = torch.randn((B, C, H, W), device=dev)
    n = x.numel() * 4
    lam_mix = torch.full((B,), 0.3, device=dev)
    box0 = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    box_cut = torch.tensor([[40, 160, 30, 190]] * B, dtype=torch.int32, device=dev)
    cut_frac = 120 * 160 / float(H * W)

    def aten_mix():
        xf = x.flip(0).mul_(0.7)
        x.mul_(0.3).add_(xf)

    def aten_cut():
        x[:, :, 40:160, 30:190] = x.flip(0)[:, :, 40:160, 30:190]

    R, V, ld = 960, 50265, 50304
    logits = torch.randn((R, ld), device=dev) * 2
    labels = torch.randint(0, V, (R,), device=dev)
    labels[::7] = -100
    scale = torch.full((1,), 1.0 / R, device=dev)
    s = 0.1
    lse0, _ = Fx.ce_fwd(logits, V, labels)
    fwd_bytes_plain, fwd_bytes_smooth = 2 * R * V * 4, R * V * 4   # the plain forward walks the row twice (max, then sum-exp)
    bwd_bytes = R * V * 4 + R * ld * 2
    cands = {
        # name: (callable, bytes its kernels move)
        "mixup/xfm_mixup": (lambda: Fx.mixup_(x, lam_mix, box0), 2 * n),                       # read + write the batch once
        "mixup/aten flip,mul_,mul_,add_": (aten_mix, 9 * n),                                   # what its four kernels move: flip r+w, mul_ r+w, mul_ r+w, add_ 2r+w
        "cutmix/xfm_mixup": (lambda: Fx.mixup_(x, lam_mix, box_cut), int((1 + cut_frac) * n)),   # read all, write the box
        "cutmix/aten flip,slice copy": (aten_cut, int((2 + 2 * cut_frac) * n)),
        "ce/xfm_ce_fwd": (lambda: Fx.ce_fwd(logits, V, labels), fwd_bytes_plain),
        "ce/xfm_ce_smooth_fwd": (lambda: Fx.ce_smooth_fwd(logits, V, labels, 1 - s, s / V), fwd_bytes_smooth),
        "ce/xfm_ce_bwd": (lambda: Fx.ce_bwd(logits, V, labels, lse0, scale, ld), bwd_bytes),
        "ce/xfm_ce_smooth_bwd": (lambda: Fx.ce_smooth_bwd(logits, V, labels, 1 - s, s / V, lse0, scale, ld), bwd_bytes),
    }
    times = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, (fn, _) in cands.items():
            times[k].append(timed(fn, a.iters, a.warmup))
    for k, (_, nbytes) in cands.items():
        t = sorted(times[k])
        med = t[len(t) // 2]
        print(json.dumps({"name": k, "us_median": round(med * 1e6, 2), "us_min": round(t[0] * 1e6, 2), "us_max": round(t[-1] * 1e6, 2),
                          "bytes": nbytes, "TB_per_s": round(nbytes / med * 1e-12, 3), "hbm_fraction": round(nbytes / med / HBM_PEAK, 3)}), flush=True)


if __name__ == "__main__":
    main()
