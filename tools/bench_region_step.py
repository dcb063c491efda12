"""The region pre-training step (model_pretrain.XFM.forward_multimodal with ret_bbox_loss / ret_bbox_giou, forward + backward) with the
fused region glue (xfm_region_pool_*, xfm_rows_index_sum fold, xfm_box_loss_*) and with the ATen glue, side by side on one box
(profiles/region_step.md).  Shape of configs/Pretrain_synthetic_regions.yaml: 96 samples over 64 images, 224 px, 12 + 12 + 12 layers.

The A/B knob is xfm_amd.beit2.REGION_GLUE_FUSED (XFM_REGION_GLUE=0 in the environment): this tool flips it between rounds, so both
forms run in one process, alternating.  HIP events around `--iters` steps after `--warmup` steps of the same form; median over
`--rounds`.  The glue alone (region outputs + per-sample copy + box loss, forward + backward on tensors of the step's shapes) is timed
the same way, and its kernel launches are counted with torch.profiler in a pass of its own.

    python tools/bench_region_step.py [--iters 10] [--warmup 3] [--rounds 5] [--depth 12]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xfm_amd import beit2, synthetic as syn  # noqa: E402
from xfm_amd.model_pretrain import XFM  # noqa: E402
from xfm_amd.xfm import XFMBase, gather_images  # noqa: E402

BS, N_IMG = 96, 64


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


def region_inputs(vocab):
    t = syn.region_batch(BS, BS, 1, seed=77, vocab=vocab)   # one sample per image ...
    idx = torch.tensor(sorted(list(range(N_IMG)) + list(range(BS - N_IMG))))   # ... regrouped: 32 images carry two samples, 32 one
    return [t[0][:N_IMG], idx] + list(t[2:])


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_region_step: needs the GPU (no fallback)")
    cfg = {"use_beit_v2": True, "image_res": 224, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": a.depth, "text_fusion_start_at": a.depth, "fusion_num_hidden_layers": a.depth,
           "fusion_fusion_start_at": 0, "embed_dim": 256, "temp": 0.07, "vision_depth": a.depth}
    m = XFM(cfg)
    m.load_state_dict(syn.formula_state_dict(m.state_dict()), strict=True)
    m.cuda().finalize().train()
    image, idx, text_ids, text_atts, text_ids_masked, masked_pos, masked_ids, image_atts, target_bbox, is_image = \
        (t.cuda() for t in region_inputs(syn.VOCAB))

    def step():
        m.zero_grad()
        loss = m(image, text_ids, text_atts, text_ids_masked=text_ids_masked, masked_pos=masked_pos, masked_ids=masked_ids,
                 image_atts=image_atts, idx_to_group_img=idx, target_bbox=target_bbox, is_image=is_image, ret_bbox_loss=True,
                 ret_bbox_giou=True, data_source="region")
        (loss["loss_itc"] + loss["loss_itm"] + loss["loss_mlm"] + loss["loss_bbox"] + loss["loss_giou"]).backward()

    # the glue alone, on tensors of the step's shapes
    P, D = (224 // 16) ** 2, 768
    full = syn.symmetric("bench_region.full", (N_IMG, 1 + P, D), 1.0).to(torch.bfloat16).cuda().requires_grad_(True)
    cot = syn.symmetric("bench_region.cot", (BS, 1 + P, D), 1.0).to(torch.bfloat16).cuda()
    coord = torch.sigmoid(syn.symmetric("bench_region.coord", (BS, 4), 1.0)).cuda().requires_grad_(True)

    def glue():
        full.grad = coord.grad = None
        y = beit2.region_outputs(full, idx, image_atts)
        fused = beit2.REGION_GLUE_FUSED
        y2 = gather_images(full, idx) if fused else full.index_select(0, idx)
        torch.autograd.backward([y, y2], [cot, cot])
        l1, giou = XFMBase.get_bbox_loss(None, coord, target_bbox, is_image, fused=fused)
        (l1 + giou).backward()

    times = {(what, mode): [] for what in ("step", "glue") for mode in ("fused", "aten")}
    for _ in range(a.rounds):
        for mode in ("fused", "aten"):
            beit2.REGION_GLUE_FUSED = mode == "fused"
            times[("step", mode)].append(timed(step, a.iters, a.warmup))
            times[("glue", mode)].append(timed(glue, 10 * a.iters, a.warmup))
    launches = {}
    for mode in ("fused", "aten"):
        beit2.REGION_GLUE_FUSED = mode == "fused"
        try:
            launches[mode] = kernel_launches(glue)
        except Exception as e:   # the profiler is optional: the times above stand without it
            launches[mode] = f"not measured ({type(e).__name__})"
    for (what, mode), t in times.items():
        t = sorted(t)
        out = {"name": f"{what}/{mode}", "ms_median": round(t[len(t) // 2] * 1e3, 4), "ms_min": round(t[0] * 1e3, 4),
               "ms_max": round(t[-1] * 1e3, 4), "samples": BS, "images": N_IMG, "depth": a.depth}
        if what == "glue":
            out["kernel_launches"] = launches[mode]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
