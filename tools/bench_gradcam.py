"""One Grad-CAM evaluation pass (Grounding.py:76-126 `val`) at the workload's own shape -- configs/Grounding_synthetic.yaml: 32 expressions
of up to 40 tokens per batch, 384 px (577 image tokens), 12 + 12 layers, `block_num` from the config -- with
`cross_attention_gradcam(fused=True)` (one _EncoderFn segment above block_num, the activation-gradient chain down to dc2 of that layer, one
xfm_xattn_gradcam launch) against `fused=False` (the reference's recipe on the module contract: full backward, two [B, 12, T, 577] fp32
maps, the ATen lines of Grounding.py:101-115), side by side on one box (profiles/gradcam.md).

Both forms run in one process, alternating: a host clock around `--iters` passes that end in a device synchronise, after `--warmup` passes
of the same form, median over `--rounds`; peak allocated memory per form (reset before its timed passes); the box's clocks are read under
the fused form's load after the timed rounds (bench.sample_clocks) and printed as a third line.  Recorded, not gated.

    python tools/bench_gradcam.py [--iters 3] [--warmup 1] [--rounds 3] [--batches 1] [--depth 12]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import sample_clocks  # noqa: E402
from xfm_amd import gradcam as GC  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402
from xfm_amd import task as T  # noqa: E402
from xfm_amd.model_retrieval import XFMForRetrieval  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters, torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=1)
    ap.add_argument("--depth", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gradcam: needs the GPU (no fallback)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = T.load_yaml(os.path.join(root, "configs", "Grounding_synthetic.yaml"))
    if a.depth != 12:
        cfg.update(text_num_hidden_layers=a.depth, text_fusion_start_at=a.depth, fusion_num_hidden_layers=a.depth, vision_depth=a.depth,
                   block_num=min(cfg["block_num"], a.depth - 1))
    B, res, block_num = cfg["batch_size"], cfg["image_res"], cfg["block_num"]
    m = XFMForRetrieval(cfg)
    m.load_state_dict(syn.formula_state_dict(m.state_dict()), strict=True)
    m.cuda().finalize().eval()
    loader = []
    for i in range(a.batches):
        image, (ids, atts), ref_ids = syn.grounding_eval_batch(B, seed=384 + i, image_res=res, max_tokens=cfg["max_tokens"], first_ref_id=i * B)
        loader.append((image.cuda(), (ids.cuda(), atts.cuda()), ref_ids))
    dev, p = torch.device("cuda"), res // cfg["patch_size"]
    forms = {"fused": lambda: GC.val(m, loader, dev, block_num, p, fused=True)[0],
             "unfused": lambda: GC.val(m, loader, dev, block_num, p, fused=False)[0]}
    cf, cu = forms["fused"]().double(), forms["unfused"]().double()
    rel = float((cf - cu).norm() / cu.norm())
    times, peak = {k: [] for k in forms}, {k: 0 for k in forms}
    for _ in range(a.rounds):
        for name in ("unfused", "fused"):
            t, mem = timed(forms[name], a.iters, a.warmup)
            times[name].append(t)
            peak[name] = max(peak[name], mem)
    for name in ("unfused", "fused"):
        t = sorted(times[name])
        print(json.dumps({"name": "gradcam/" + name, "ms_median": round(t[len(t) // 2] * 1e3, 3), "ms_min": round(t[0] * 1e3, 3),
                          "ms_max": round(t[-1] * 1e3, 3), "peak_allocated_mib": round(peak[name] / 2 ** 20, 1), "expressions": a.batches * B,
                          "tokens": int(loader[0][1][0].shape[1]), "image_res": res, "depth": a.depth, "block_num": block_num,
                          "fused_vs_unfused_rel_l2": rel}), flush=True)
    print(json.dumps({"name": "gradcam/clocks_under_load", **sample_clocks(forms["fused"], n_steps=4)}), flush=True)


if __name__ == "__main__":
    main()
