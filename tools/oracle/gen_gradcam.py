"""Generate tests/golden/gradcam_small.npz from the REAL reference (behind ref_shim, as gen_golden.py does).

Run in the build container only:   python tools/oracle/gen_gradcam.py

Grounding.py itself cannot be imported here (refTools, hdfs, a model class that no longer exists), so its `val` (:76-126) is compiled from
its file (gen_golden._reference_functions, as for Imagenet.py's adjust_learning_rate) and driven as it stands; what cannot run is handed
in as plain objects: a `model` namespace whose `text_encoder` is the reference XFMForRetrieval's fusion encoder (the attribute path
`text_encoder.base_model.base_model.encoder.layer[block_num].crossattention.self` of :84 then reaches fusion layer `block_num`) and whose
other attributes are the reference model's own, a tokenizer that returns the token ids it is given, a loader of one batch, and
utils.MetricLogger as a pass-through.  `grounding_eval` and `computeIoU` are the reference's own dataset/utils.py:178-223, 349-361, imported
behind stubs of the third-party modules that file imports (as gen_grounding_loop.reference_eval does), `Tensor.cuda` the identity for the
call, the REFER object and the detector file as plain dicts.

The model: reference XFMForRetrieval, a 2-block vision tower, 2 text layers, 3 fusion layers, formula weights, eval mode; block_num = 1;
96 px images (p = 6); B = 5 expressions of ragged lengths, one of length 3.

Stored (data only): the token ids and masks (the images are regenerated from their seed), the reference's cams, its P and dP at block_num
(the rows past a sequence's length zeroed), the same cams from the reference under bf16 autocast and per ref [rel-L2, cosine] of those
against the fp32 ones (the floor, as amp_floor is for gradients), 3 to 6 detector boxes per ref, image sizes, ref boxes and splits, the
chosen indices, scores, IoUs and the accuracy dict of the reference's own grounding_eval.

The boxes are chosen FROM the cams so that every decision has a margin the 16-bit towers cannot flip: every winner's score is >= 1.3 x the
runner-up's, every IoU is at least 0.05 away from 0.5, every ref has a positive score.  Asserted below, with the file size."""
import importlib
import json
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402
import ref_shim  # noqa: E402
from xfm_amd import gradcam as GC  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

GRADCAM = {"B": 5, "image_res": 96, "patch": 16, "block_num": 1, "text_layers": 2, "fusion_layers": 3, "max_tokens": 12, "min_len": 3,
           "seed": 4100, "seed_tries": 200, "alpha": 0.5, "ref_ids": [907, 12, 4471, 33, 260], "split": [0, 1, 2, 0, 1],
           "image_sizes": [[640, 480], [500, 375], [427, 640], [333, 500], [612, 612]],   # (width, height)
           "near": [True, False, True, True, False], "win_ratio": 1.3, "iou_margin": 0.05}
SPLIT_NAMES = ["val", "testA", "testB"]


def reference_utils():
    """dataset/utils.py of the reference, imported inside a stand-in `dataset` package behind stubs of what it imports and does not use."""
    ref_shim.install()
    pkg = types.ModuleType("dataset")
    pkg.__path__ = [os.path.join(ref_shim.REF_ROOT, "dataset")]
    pkg.__spec__ = importlib.machinery.ModuleSpec("dataset", loader=None, is_package=True)
    sys.modules["dataset"] = pkg
    for name, attrs in (("vqaTools", {}), ("vqaTools.vqaEval", {"VQAEval": None}), ("refTools", {}), ("refTools.evaluation", {}),
                        ("refTools.evaluation.refEvaluation", {"RefEvaluation": None}), ("pycocotools", {}),
                        ("pycocotools.coco", {"COCO": None}), ("pycocoevalcap", {}), ("pycocoevalcap.eval", {"COCOEvalCap": None})):
        if name not in sys.modules:
            ref_shim._stub(name, **attrs)
    return importlib.import_module("dataset.utils")


class _Logger:
    def __init__(self, delimiter="  "):
        pass

    def log_every(self, iterable, print_freq, header=None):
        yield from iterable


class _Tokens(NS):
    def to(self, device):
        return self


def run_val(val, m, batch, block_num, p):
    """The reference's val on one batch -> (cams [B, p, p], P, dP of fusion layer block_num)."""
    model = NS(eval=m.eval, text_encoder=m.fusion_encoder, get_vision_embeds=m.get_vision_embeds, get_cross_embeds=m.get_cross_embeds,
               itm_head=m.itm_head, zero_grad=m.zero_grad, num_attention_heads=m.num_attention_heads)
    val.__globals__["utils"] = NS(MetricLogger=_Logger)
    image, (ids, atts), ref_ids = batch
    tokenizer = lambda text, padding=None, return_tensors=None: _Tokens(input_ids=text[0], attention_mask=text[1])   # noqa: E731
    result = val(model, [(image, (ids, atts), ref_ids)], tokenizer, "cpu", "itm", block_num, p)
    att = m.fusion_encoder.base_model.base_model.encoder.layer[block_num].crossattention.self
    assert [r["ref_id"] for r in result] == ref_ids.tolist()
    return torch.stack([r["pred"] for r in result]).detach(), att.get_attention_map().detach().clone(), att.get_attn_gradients().detach().clone()


def choose_boxes(cam, size, near, k, n_boxes, alpha, L):
    """Detector boxes and a ref box for one map, chosen from it: the winner clears the runner-up by win_ratio, the IoU 0.5 by iou_margin."""
    W, H = size
    p = cam.shape[0]
    u = syn.uniform01("gradcam.boxes", 400 * 4, L["seed"] + k).reshape(400, 4)
    w, h = np.floor(20 + u[:, 2] * 0.5 * W) + 0.5, np.floor(20 + u[:, 3] * 0.5 * H) + 0.25
    x, y = np.floor(u[:, 0] * (W - w)) + 0.25, np.floor(u[:, 1] * (H - h)) + 0.5
    cand = np.stack([x, y, w, h], axis=1)
    hw = np.array([[H, W]])
    score = np.array([GC.cam_box_rank_host(cam[None], hw, [c[None]], np.zeros((1, 4)), [0], alpha)[0][0, 1] for c in cand])
    order = np.argsort(-score)
    win = order[0]
    assert score[win] > 0
    rest = [j for j in order[1:] if 0 < score[j] * L["win_ratio"] <= score[win]][:n_boxes - 1]
    assert len(rest) == n_boxes - 1, "not enough boxes under the winner's margin"
    chosen = [rest[0], win] + rest[1:]            # (the winner is not the first box)
    dets = cand[chosen]
    bx = cand[win]
    if near:      # a ground truth close to the winner: IoU well above 0.5
        ref = [np.floor(bx[0]) + 2, np.floor(bx[1]) + 1, np.floor(bx[2]) - 3, np.floor(bx[3]) - 2]
    else:         # a ground truth in the corner farthest from it
        rw, rh = np.floor(0.2 * W), np.floor(0.2 * H)
        ref = [0.0 if bx[0] + bx[2] / 2 > W / 2 else W - rw, 0.0 if bx[1] + bx[3] / 2 > H / 2 else H - rh, rw, rh]
    iou = GC.compute_iou([float(v) for v in ref], [float(v) for v in bx])
    assert abs(iou - 0.5) >= L["iou_margin"] and (iou > 0.5) == near, (k, iou)
    return dets, np.asarray(ref, dtype=np.float64), 1, float(score[win]), float(max(score[j] for j in rest))


def main():
    ref_shim.install()
    from models.model_retrieval import XFMForRetrieval
    (val,) = G._reference_functions("Grounding.py", ["val"])
    ref_shim.init_single_process_group()
    L = dict(GRADCAM)
    torch.manual_seed(0)
    cfg = ref_shim.pretrain_config(text_layers=L["text_layers"], fusion_layers=L["fusion_layers"], overrides={"image_res": L["image_res"]})
    with G.shallow_vit():
        m = XFMForRetrieval(cfg)
    G.load_formula(m)
    m.eval()
    B, p = L["B"], L["image_res"] // L["patch"]
    for seed in range(L["seed"], L["seed"] + L["seed_tries"]):   # ragged lengths, one of exactly 3 tokens
        image, (ids, atts), _ = syn.grounding_eval_batch(B, seed=seed, image_res=L["image_res"], max_tokens=L["max_tokens"], min_len=L["min_len"])
        lens = atts.sum(1).tolist()
        if min(lens) == 3 and len(set(lens)) >= 4:
            break
    else:
        raise RuntimeError("no seed with ragged lengths and one expression of 3 tokens")
    L["batch_seed"], L["lens"] = seed, lens
    ref_ids = torch.tensor(L["ref_ids"])
    batch = (image, (ids, atts), ref_ids)
    cams, P, dP = run_val(val, m, batch, L["block_num"], p)
    assert cams.shape == (B, p, p) and P.shape == dP.shape == (B, m.num_attention_heads, ids.shape[1], 1 + p * p)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        cams16, _, _ = run_val(val, m, batch, L["block_num"], p)
    cams16 = cams16.float()
    floor = []
    for b in range(B):
        a, r = cams16[b].double().reshape(-1), cams[b].double().reshape(-1)
        floor.append([float((a - r).norm() / r.norm()), float((a @ r) / (a.norm() * r.norm()))])
    print("lens", lens, "cam rms", [float(c.pow(2).mean().sqrt()) for c in cams], "\nbf16 autocast floor [rel-L2, cos]", floor, flush=True)
    valid = (torch.arange(ids.shape[1])[None, :] < atts.sum(1)[:, None])[:, None, :, None]
    out = {"text_ids": ids.numpy(), "text_atts": atts.numpy(), "cam": cams.numpy(), "P": (P * valid).numpy(), "dP": (dP * valid).numpy(),
           "cam_bf16_autocast": cams16.numpy(), "floor": np.asarray(floor)}

    # ---- the boxes, chosen from the cams; then the reference's own grounding_eval on them ----
    dets, ref_box, want_idx, margins = [], [], [], []
    for k in range(B):
        d, rb, idx, s_win, s_next = choose_boxes(cams[k].numpy(), L["image_sizes"][k], L["near"][k], k, 3 + k % 4, L["alpha"], L)
        dets.append(d)
        ref_box.append(rb)
        want_idx.append(idx)
        margins.append(s_win / s_next)
    assert min(margins) >= L["win_ratio"] and all(3 <= len(d) <= 6 for d in dets)
    du = reference_utils()
    refer = NS(Refs={r: {"image_id": 100 + k, "split": SPLIT_NAMES[L["split"][k]]} for k, r in enumerate(L["ref_ids"])},
               refToAnn={r: {"bbox": [float(v) for v in ref_box[k]]} for k, r in enumerate(L["ref_ids"])},
               Imgs={100 + k: {"width": L["image_sizes"][k][0], "height": L["image_sizes"][k][1]} for k in range(B)})
    det_file = {str(100 + k): [[float(v) for v in row] for row in dets[k]] for k in range(B)}
    results = [{"ref_id": r, "pred": cams[k].clone()} for k, r in enumerate(L["ref_ids"])]
    picked = []
    orig_iou, orig_cuda = du.computeIoU, torch.Tensor.cuda

    def recording_iou(box1, box2):
        picked.append([float(v) for v in box2])
        return orig_iou(box1, box2)
    du.computeIoU, torch.Tensor.cuda = recording_iou, (lambda self, *a, **kw: self)
    try:
        acc = du.grounding_eval(results, det_file, None, refer, L["alpha"], mask_size=p)
    finally:
        du.computeIoU, torch.Tensor.cuda = orig_iou, orig_cuda
    ref_idx = [det_file[str(100 + k)].index(picked[k]) for k in range(B)]
    assert ref_idx == want_idx, (ref_idx, want_idx)
    rows, counts = GC.cam_box_rank_host(cams.numpy(), np.array([[s[1], s[0]] for s in L["image_sizes"]]), dets, np.stack(ref_box), L["split"],
                                        L["alpha"])
    assert [int(r[0]) for r in rows] == ref_idx
    ious = [float(orig_iou(ref_box[k].tolist(), dets[k][ref_idx[k]].tolist())) for k in range(B)]
    assert np.abs(rows[:, 2] - np.asarray(ious)).max() < 1e-12
    assert all(abs(v - 0.5) >= L["iou_margin"] for v in ious) and [v >= 0.5 for v in ious] == L["near"]
    host_acc = {f"{SPLIT_NAMES[s]}_d": counts[s, 0] / counts[s, 1] for s in range(3)}
    assert host_acc == acc, (host_acc, acc)
    print("chosen", ref_idx, "\nscore ratio winner / runner-up", margins, "\nIoU", ious, "\nacc", acc, flush=True)
    out["det_count"] = np.asarray([len(d) for d in dets], dtype=np.int32)
    out["dets"] = np.concatenate(dets)
    out["ref_box"], out["ref_size"] = np.stack(ref_box), np.asarray(L["image_sizes"], dtype=np.float64)
    out["ref_split"] = np.asarray(L["split"], dtype=np.int32)
    out["chosen"], out["score"], out["iou"] = np.asarray(ref_idx, dtype=np.int64), rows[:, 1].copy(), np.asarray(ious)
    meta = {"spec": G.spec_of(m), "vit_depth": G.SHALLOW, "acc": acc, "score_ratio": margins, **L}
    G.save("gradcam_small", out, meta)
    path = os.path.join(G.OUT, "gradcam_small.npz")
    assert os.path.getsize(path) < 1024 * 1024 and not os.path.exists(os.path.join(G.OUT, "gradcam_small.part1.npz")), "fixture over the committed-file size limit"
    print(json.dumps({k: v for k, v in meta.items() if k != "spec"})[:2000])


if __name__ == "__main__":
    main()
