"""One grounding evaluation pass (Grounding_bbox.py:73-93 + grounding_eval_bbox) on the kernel path -- xfm_amd.grounding_loop.evaluation:
xfm_box_eval once per batch, ONE device read per pass -- and as a host walk that reads each sample's prediction back and computes its IoU
in Python, as the reference's evaluation does, side by side on one box (profiles/grounding_eval.md).
Shape of configs/xfm-ft/Grounding_bbox.yaml: 20 expressions of up to 40 tokens per batch, 384 px, 12 + 12 layers; `--batches` batches per
pass, already on the device (the upload is the same in both forms and is not what is compared).

Both forms run in one process, alternating: a host clock around `--iters` passes that end in a device synchronise, after `--warmup` passes
of the same form, median over `--rounds`; the box's clocks are read under the kernel form's load after the timed rounds
(bench.sample_clocks) and printed as a third line.  Recorded, not gated: the model's forward dominates both forms.

    python tools/bench_grounding_eval.py [--iters 5] [--warmup 2] [--rounds 3] [--batches 3] [--depth 12]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import sample_clocks  # noqa: E402
from xfm_amd import grounding_loop as GL  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402
from xfm_amd.model_grounding import XFMForGrounding  # noqa: E402

B, RES, MAX_TOKENS = 20, 384, 40


class Loader(list):
    dataset = None


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


@torch.no_grad()
def host_walk(model, loader, config):
    """The reference's shape of the pass: every prediction kept as a record (Grounding_bbox.py:90-91), then one read-back and one Python
    IoU per sample (dataset/utils.py:275-301)."""
    model.eval()
    ds = loader.dataset
    box, size, split = ds.ref_box.tolist(), ds.ref_size.tolist(), ds.ref_split.tolist()
    result = []
    for image, (text_ids, text_atts), ref_ids in loader:
        outputs_coord = model(image, text_ids, text_atts, target_bbox=None)
        for r_id, coord in zip(ref_ids, outputs_coord):
            result.append({'ref_id': r_id.item(), 'pred': coord})
    counts = [[0, 0], [0, 0], [0, 0]]
    for res in result:
        r = ds.ref_index[res['ref_id']]
        cx, cy, w, h = res['pred'].tolist()   # the per-sample device read
        (rx, ry, rw, rh), (W, H) = box[r], size[r]
        pw, ph = w * W, h * H
        px, py = cx * W - pw / 2, cy * H - ph / 2
        x1, y1 = max(rx, px), max(ry, py)
        x2, y2 = min(rx + rw - 1, px + pw - 1), min(ry + rh - 1, py + ph - 1)
        inter = (x2 - x1 + 1) * (y2 - y1 + 1) if x1 < x2 and y1 < y2 else 0
        union = rw * rh + pw * ph - inter
        counts[split[r]][1] += 1
        counts[split[r]][0] += int(union > 0 and inter / union >= 0.5)
    return {f'{name}_d': counts[s][0] / counts[s][1] for s, name in enumerate(GL.SPLITS)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--depth", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grounding_eval: needs the GPU (no fallback)")
    cfg = {"use_beit_v2": True, "image_res": RES, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": a.depth, "text_fusion_start_at": a.depth, "fusion_num_hidden_layers": a.depth,
           "fusion_fusion_start_at": 0, "vision_depth": a.depth, "batch_size": B}
    m = XFMForGrounding(cfg)
    m.load_state_dict(syn.formula_state_dict(m.state_dict()), strict=True)
    m.cuda().finalize().eval()
    loader = Loader()
    for i in range(a.batches):
        image, (ids, atts), ref_ids = syn.grounding_eval_batch(B, seed=384 + i, image_res=RES, max_tokens=MAX_TOKENS, first_ref_id=i * B)
        loader.append((image.cuda(), (ids.cuda(), atts.cuda()), ref_ids))
    loader.dataset = syn.grounding_refs(a.batches * B, seed=385)
    dev = torch.device("cuda")
    devnull = open(os.devnull, "w")

    def kernel_pass():
        out, sys.stdout = sys.stdout, devnull   # (evaluation prints the accuracies as the reference does)
        try:
            return GL.evaluation(m, loader, dev, cfg)
        finally:
            sys.stdout = out

    forms = {"kernel": kernel_pass, "host_walk": lambda: host_walk(m, loader, cfg)}
    same = forms["kernel"]() == forms["host_walk"]()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for name in ("host_walk", "kernel"):
            times[name].append(timed(forms[name], a.iters, a.warmup))
    for name in ("host_walk", "kernel"):
        t = sorted(times[name])
        print(json.dumps({"name": "grounding_eval/" + name, "ms_median": round(t[len(t) // 2] * 1e3, 3), "ms_min": round(t[0] * 1e3, 3),
                          "ms_max": round(t[-1] * 1e3, 3), "expressions": a.batches * B, "batches": a.batches, "image_res": RES,
                          "depth": a.depth, "same_accuracy": bool(same)}), flush=True)
    print(json.dumps({"name": "grounding_eval/clocks_under_load", **sample_clocks(kernel_pass, n_steps=4)}), flush=True)


if __name__ == "__main__":
    main()
