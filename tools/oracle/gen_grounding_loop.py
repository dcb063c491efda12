"""Generate tests/golden/grounding_loop_small.npz from the REAL reference (behind ref_shim, as gen_golden.py does).

Run in the build container only:   python tools/oracle/gen_grounding_loop.py

Grounding_bbox.py itself cannot be imported here (ruamel, the dataset package, a tokenizer, refTools), so, as for vqa_loop_small: the
MODEL is the reference's XFMForGrounding (shallow towers, formula weights), the schedule is the reference's scheduler.create_scheduler, the
four optimizer groups are formed by the reference's optim.create_optimizer, and the loop of Grounding_bbox.py:39-93 is restated call for
call around them on token-id batches.  The model stays in eval mode (dropout and drop-path off), which is how the other task fixtures
make the run reproducible.

Stored (data only):
  * ONE evaluation pass at the formula weights (the state both sides can build exactly): 6 refs in batches of (2, 4) -- the predicted
    coords, and from the reference's OWN dataset/utils.py computeIoU / grounding_eval_bbox (imported behind stubs of the third-party
    modules that file imports and does not use here, `Tensor.cuda` the identity for the call): the pixel boxes, the IoUs, the correct
    flags and the accuracy dict; the ref tables (8 rows, two of them never asked for, in an order that is not the samples').
  * two training iterations (B = 4, T <= 16): both losses per iteration, the learning rate of every group after each scheduler step.

The margin condition: the refs are BUILT from the reference's predictions -- a jittered copy of the predicted pixel box (IoU about 0.9)
or a box far from it (IoU 0) -- and every sample's flag must stay the same when each of its 4 coordinates moves by -1e-2, 0 or +1e-2 in
all 81 combinations: 1e-2 is the coordinate bound of tests/test_hip_modules.py::test_grounding_model_vs_golden, so no allowed error of the
16-bit towers flips a flag, and flags and accuracies are compared for EQUALITY.  All three splits are present and both outcomes occur.
Every ref is a valid ground truth (whole pixels, inside its image), and the formula weights often predict boxes that leave the image, where
no valid box can follow them: a jittered ref that fails the condition (a half-overlapping one does) is REJECTED, the sample gets a far ref
instead, and the evaluation seed is searched for a pass in which at least three samples keep their jittered ref.

The same two iterations also run under the reference's bf16 autocast; its losses must lie within 1e-2 of the fp32 ones -- half the 2e-2
bound the GPU test uses, so that bound is known to be reachable before any GPU sees it."""
import copy
import itertools
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402  (puts the repository root on sys.path and installs nothing by itself)
import ref_shim  # noqa: E402
from gen_vqa_loop import AttrDict, _reference_optim  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

COORD_TOL = 1e-2   # tests/test_hip_modules.py::test_grounding_model_vs_golden
GROUNDING_LOOP = {"B": 4, "train_seeds": [1201, 1202], "max_tokens": 16, "min_len": 5, "image_res": 224,
                  "eval_B": 6, "eval_seed": 1311, "eval_seed_tries": 60, "eval_batches": [2, 4],
                  "ref_ids": [4007, 12, 583, 90210, 31, 2718], "table_ref_ids": [31, 77, 90210, 12, 2718, 4007, 5, 583],
                  "sample_split": [0, 1, 2, 0, 1, 2],   # (which samples get a jittered ref is decided by the search in main())
                  "image_sizes": [[640, 480], [500, 375], [427, 640], [640, 428], [333, 500], [612, 612], [640, 360], [480, 640]],
                  "optimizer": {"opt": "adamW", "lr": 2e-5, "weight_decay": 0.01, "lr_mult": 2},
                  "schedular": {"sched": "linear", "lr": 2e-5, "epochs": 2, "num_warmup_steps": 0.25}}
SPLIT_NAMES = ["val", "testA", "testB"]


def iou64(coord, box, size):
    """The evaluation's rule in fp64 (dataset/utils.py:281-288 + computeIoU) for one sample -> (pixel box, IoU)."""
    cx, cy, w, h = (float(v) for v in coord)
    W, H = (float(v) for v in size)
    rx, ry, rw, rh = (float(v) for v in box)
    pw, ph = w * W, h * H
    px, py = cx * W - pw / 2, cy * H - ph / 2
    x1, y1 = max(rx, px), max(ry, py)
    x2, y2 = min(rx + rw - 1, px + pw - 1), min(ry + rh - 1, py + ph - 1)
    inter = (x2 - x1 + 1) * (y2 - y1 + 1) if x1 < x2 and y1 < y2 else 0.0
    return (px, py, pw, ph), inter / (rw * rh + pw * ph - inter)


def margin_ok(coord, box, size):
    """The flag of the sample under all 81 moves of its coordinates by {-tol, 0, +tol} -> (all equal, the IoUs' range)."""
    ious = [iou64(np.asarray(coord, dtype=np.float64) + np.asarray(d) * COORD_TOL, box, size)[1]
            for d in itertools.product((-1, 0, 1), repeat=4)]
    flags = {v >= 0.5 for v in ious}
    return len(flags) == 1, (min(ious), max(ious))


def build_ref(coord, size, near, k):
    """A valid ground-truth box (whole pixels, inside the image) for one prediction: a jittered copy of the predicted pixel box, or a box
    in the corner of the image farthest from it."""
    W, H = size
    (px, py, pw, ph), _ = iou64(coord, (0, 0, 1, 1), size)
    if near:
        x, y = px + (0.02 + 0.005 * k) * pw, py - (0.015 + 0.004 * k) * ph
        w, h = pw * (0.97 + 0.01 * (k % 3)), ph * (1.03 - 0.01 * (k % 2))
        x, y = max(x, 0.0), max(y, 0.0)
        w, h = min(w, W - x), min(h, H - y)
    else:
        w, h = 0.2 * W, 0.2 * H
        x = 0.0 if px + pw / 2 > W / 2 else W - w
        y = 0.0 if py + ph / 2 > H / 2 else H - h
    box = [float(np.floor(x)), float(np.floor(y)), float(max(np.floor(w), 1.0)), float(max(np.floor(h), 1.0))]
    assert box[0] >= 0 and box[1] >= 0 and box[2] > 0 and box[3] > 0 and box[0] + box[2] <= W and box[1] + box[3] <= H, (box, size)
    return box


def reference_eval(coords, ref_ids, refer):
    """The reference's own grounding_eval_bbox and computeIoU on `coords` -> (accuracy dict, pixel boxes as it forms them, IoUs, source).
    dataset/utils.py is imported inside a stand-in `dataset` package (its __init__ needs torchvision / PIL) with stubs for the third-party
    modules it imports at the top and at the bottom; `Tensor.cuda` is the identity for the call (no GPU here), so the in-place pixel
    scaling of :282-286 lands in the tensors handed over -- clones -- which are then the pixel boxes the reference computed."""
    import importlib
    import types
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
    du = importlib.import_module("dataset.utils")
    results = [{"ref_id": r, "pred": c.clone()} for r, c in zip(ref_ids, coords)]
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **kw: self
    try:
        acc = du.grounding_eval_bbox(results, refer)
    finally:
        torch.Tensor.cuda = orig_cuda
    pixel = torch.stack([r["pred"] for r in results])
    ious = [float(du.computeIoU(refer.refToAnn[r["ref_id"]]["bbox"], r["pred"])) for r in results]
    return acc, pixel, ious, "reference"


def train_two(m, create_optimizer, create_scheduler, loader, autocast):
    """Grounding_bbox.py:50-65 on `loader` -> (losses [n, 2], learning rates after every scheduler step [n, groups], optimizer)."""
    L = GROUNDING_LOOP
    arg_opt = AttrDict(L["optimizer"])
    optimizer = create_optimizer(arg_opt, m)
    arg_sche = AttrDict(L["schedular"])
    arg_sche['step_per_epoch'] = len(loader)
    lr_scheduler = create_scheduler(arg_sche, optimizer)
    losses, lrs = [], []
    for image, (text_ids, text_atts), target_bbox in loader:
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            _, loss_bbox, loss_giou = m(image, text_ids, text_atts, target_bbox=target_bbox)
            loss = loss_bbox + loss_giou
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        lr_scheduler.step()
        losses.append([loss_bbox.item(), loss_giou.item()])
        lrs.append([g["lr"] for g in optimizer.param_groups])
    return losses, lrs, optimizer, arg_sche


def main():
    ref_shim.install()
    from models.model_grounding import XFMForGrounding
    create_optimizer, create_scheduler = _reference_optim()
    ref_shim.init_single_process_group()
    L = GROUNDING_LOOP
    torch.manual_seed(0)
    cfg = ref_shim.pretrain_config(text_layers=2, fusion_layers=2, overrides={"image_res": L["image_res"]})
    with G.shallow_vit():
        m = XFMForGrounding(cfg)
    G.load_formula(m)
    m.eval()
    out = {}

    # ---- one evaluation pass at the formula weights (Grounding_bbox.py:73-93) in batches of (2, 4) ----
    # The formula weights often predict boxes that leave the image, and a valid ground truth (inside the image) cannot follow them there:
    # the evaluation seed is searched for the pass in which the most samples admit a jittered ref that clears the margin condition.
    R = len(L["table_ref_ids"])
    row_of = {r: i for i, r in enumerate(L["table_ref_ids"])}
    best = None
    for seed in range(L["eval_seed"], L["eval_seed"] + L["eval_seed_tries"]):
        image, (text_ids, text_atts), _ = syn.grounding_eval_batch(L["eval_B"], seed=seed, image_res=L["image_res"],
                                                                   max_tokens=L["max_tokens"], min_len=L["min_len"])
        coords, o = [], 0
        for n in L["eval_batches"]:
            with torch.no_grad():
                coords.append(m(image[o:o + n], text_ids[o:o + n], text_atts[o:o + n], target_bbox=None))
            o += n
        coords = torch.cat(coords).float()
        assert coords.shape == (L["eval_B"], 4)
        near = []
        for k, ref_id in enumerate(L["ref_ids"]):
            size = L["image_sizes"][row_of[ref_id]]
            try:
                ok, rng = margin_ok(coords[k].tolist(), build_ref(coords[k].tolist(), size, True, k), size)
            except AssertionError:   # (no valid box near this prediction)
                ok, rng = False, (0.0, 0.0)
            near.append(bool(ok and rng[0] >= 0.5))
        print("eval seed", seed, "samples that admit a jittered ref:", near, flush=True)
        if best is None or sum(near) > sum(best[1]):
            best = (seed, near, coords)
        if sum(near) >= 3:
            break
    eval_seed, near_ok, coords = best
    assert sum(near_ok) >= 2, "no evaluation seed with two samples whose jittered ref clears the margin"
    sample_near = list(near_ok)
    while sum(sample_near) > 4:   # (both outcomes must occur)
        sample_near[len(sample_near) - 1 - sample_near[::-1].index(True)] = False
    # the ref tables, built from the predictions; rows the samples do not ask for get a formula box
    ref_box, ref_size, ref_split = np.zeros((R, 4), np.float32), np.asarray(L["image_sizes"], np.float32), np.full(R, 0, np.int32)
    spare = syn.grounding_refs(R, seed=17)
    for i in range(R):
        if L["table_ref_ids"][i] not in L["ref_ids"]:
            ref_split[i] = i % 3
            ref_box[i] = (spare.ref_box[i] * 0.5).floor().clamp(min=1.0).numpy()
    margins = []
    for k, ref_id in enumerate(L["ref_ids"]):
        i = row_of[ref_id]
        ref_box[i] = build_ref(coords[k].tolist(), L["image_sizes"][i], sample_near[k], k)
        ref_split[i] = L["sample_split"][k]
        ok, rng = margin_ok(coords[k].tolist(), ref_box[i], ref_size[i])
        assert ok, f"sample {k}: the flag flips inside the coordinate tolerance, IoU in {rng}: reject this ref"
        assert (rng[0] >= 0.5) == sample_near[k], (k, rng)
        margins.append(list(rng))
    L = dict(L, eval_seed=eval_seed, sample_near=sample_near)
    assert sorted(set(L["sample_split"])) == [0, 1, 2] and len(set(L["sample_near"])) == 2
    refer = NS(Refs={r: {"image_id": 100 + row_of[r], "split": SPLIT_NAMES[int(ref_split[row_of[r]])]} for r in L["ref_ids"]},
               refToAnn={r: {"bbox": [float(v) for v in ref_box[row_of[r]]]} for r in L["ref_ids"]},
               Imgs={100 + row_of[r]: {"width": int(ref_size[row_of[r], 0]), "height": int(ref_size[row_of[r], 1])} for r in L["ref_ids"]})
    restated = [iou64(coords[k].tolist(), ref_box[row_of[r]], ref_size[row_of[r]]) for k, r in enumerate(L["ref_ids"])]
    try:
        acc, pixel, ious, source = reference_eval(coords, L["ref_ids"], refer)
    except Exception as e:   # the import could not be made to work: the restatement above stands in
        print("reference evaluation unavailable:", repr(e), flush=True)
        correct = [v >= 0.5 for _, v in restated]
        acc = {f"{SPLIT_NAMES[s]}_d": sum(c for c, t in zip(correct, L["sample_split"]) if t == s) / L["sample_split"].count(s) for s in range(3)}
        pixel, ious, source = torch.tensor([p for p, _ in restated]), [v for _, v in restated], "restated"
    correct = [v >= 0.5 for v in ious]
    assert correct == L["sample_near"], (correct, ious)
    assert np.abs(np.asarray(ious) - np.asarray([v for _, v in restated])).max() < 1e-6   # fp32 pixel boxes against fp64
    print("coords", coords.tolist(), "\nref_box", ref_box.tolist(), "\npixel", pixel.tolist(), "\nious", ious, "\nmargins", margins,
          "\nacc", acc, "source", source, flush=True)
    out["eval/coord"] = coords.numpy()
    out["eval/pixel_box"] = pixel.float().numpy()
    out["eval/iou"] = np.asarray(ious, dtype=np.float64)
    out["eval/correct"] = np.asarray(correct, dtype=np.bool_)
    out["eval/ref_box"], out["eval/ref_size"], out["eval/ref_split"] = ref_box, ref_size, ref_split

    # ---- two training iterations (Grounding_bbox.py:39-70), fp32 and under bf16 autocast ----
    loader = [syn.grounding_batch(L["B"], seed=s, image_res=L["image_res"], max_tokens=L["max_tokens"], min_len=L["min_len"])
              for s in L["train_seeds"]]
    m16 = copy.deepcopy(m)
    losses, lrs, optimizer, arg_sche = train_two(m, create_optimizer, create_scheduler, loader, autocast=False)
    losses16, _, _, _ = train_two(m16, create_optimizer, create_scheduler, loader, autocast=True)
    print("loss", losses, "\nbf16 autocast", losses16, "\nlr", lrs, flush=True)
    gap = float(np.abs(np.asarray(losses) - np.asarray(losses16)).max())
    assert gap < 1e-2, f"bf16 autocast moves a loss by {gap}: the 2e-2 bound of the GPU test is not known to be reachable"
    out["train/loss"] = np.asarray(losses, dtype=np.float64)
    out["train/loss_bf16_autocast"] = np.asarray(losses16, dtype=np.float64)
    out["train/lr"] = np.asarray(lrs, dtype=np.float64)
    names = {id(p): n for n, p in m.named_parameters()}
    groups = [[names[id(p)] for p in g["params"]] for g in optimizer.param_groups]
    meta = {"spec": G.spec_of(m), "text_layers": 2, "fusion_layers": 2, "vit_depth": G.SHALLOW, "groups": [len(g) for g in groups],
            "stepped": sum(1 for p in m.parameters() if p in optimizer.state), "num_warmup_steps": arg_sche["num_warmup_steps"],
            "num_training_steps": arg_sche["num_training_steps"], "acc": acc, "eval_source": source, "coord_tol": COORD_TOL,
            "iou_range_under_tol": margins, "bf16_autocast_gap": gap, **L}
    G.save("grounding_loop_small", out, meta)
    print(json.dumps({k: v for k, v in meta.items() if k != "spec"})[:3000])


if __name__ == "__main__":
    main()
