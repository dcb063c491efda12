"""Shared helpers of the grounding-loop tests (test infrastructure): the fixture's configuration, batches and loader, an independent fp64
numpy restatement of the evaluation's IoU rule, the CPU model path -- the oracle's grounding forward behind an nn.Module with the
reference's call form -- and the input cases of the xfm_box_eval kernel tests.

Run as a program (`python tests/grounding_loop_util.py`) it is the child of the kernel test's XFM_DETERMINISTIC check: it runs xfm_box_eval
on every case and prints one line of hex digests."""
import hashlib
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

if __name__ == "__main__":   # (under pytest, tests/conftest.py has put the repository root on the path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from golden_util import load, state_from_spec  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402


def fixture():
    return load("grounding_loop_small")


def loop_config(meta, **kw):
    cfg = {"use_beit_v2": True, "image_res": meta["image_res"], "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": meta["text_layers"], "text_fusion_start_at": meta["text_layers"],
           "fusion_num_hidden_layers": meta["fusion_layers"], "fusion_fusion_start_at": 0, "embed_dim": 256, "temp": 0.07,
           "learnable_temp": True, "max_temp": 0.5, "min_temp": 0.001, "vision_depth": meta["vit_depth"],
           "batch_size": meta["B"], "max_tokens": meta["max_tokens"],
           "schedular": dict(meta["schedular"]), "optimizer": dict(meta["optimizer"])}
    cfg.update(kw)
    return cfg


def train_batches(meta):
    """The fixture's two training batches in the loop's layout: (image, (text_ids, text_atts), target_bbox)."""
    return [syn.grounding_batch(meta["B"], seed=s, image_res=meta["image_res"], max_tokens=meta["max_tokens"], min_len=meta["min_len"])
            for s in meta["train_seeds"]]


class TestLoader(list):
    """A list of (image, text, ref_ids) batches with the `dataset` the evaluation reads."""
    __test__ = False

    def __init__(self, batches, dataset):
        super().__init__(batches)
        self.dataset = dataset


def eval_loader(z, meta, splits=None):
    """The fixture's six refs as batches of (2, 4), with its ref tables (8 rows in an order that is not the samples')."""
    splits = splits or meta["eval_batches"]
    image, (ids, atts), _ = syn.grounding_eval_batch(meta["eval_B"], seed=meta["eval_seed"], image_res=meta["image_res"],
                                                     max_tokens=meta["max_tokens"], min_len=meta["min_len"])
    ref_ids = torch.tensor(meta["ref_ids"])
    assert sum(splits) == meta["eval_B"] == ref_ids.numel()
    dataset = NS(ref_box=torch.from_numpy(z["eval/ref_box"]), ref_size=torch.from_numpy(z["eval/ref_size"]),
                 ref_split=torch.from_numpy(z["eval/ref_split"]), ref_index={r: i for i, r in enumerate(meta["table_ref_ids"])})
    batches, o = [], 0
    for n in splits:
        batches.append((image[o:o + n], (ids[o:o + n], atts[o:o + n]), ref_ids[o:o + n]))
        o += n
    return TestLoader(batches, dataset)


def fixture_rows(meta):
    """Row of the ref tables of each of the fixture's six samples."""
    return np.asarray([meta["table_ref_ids"].index(r) for r in meta["ref_ids"]])


def fixture_counts(z, meta):
    """The [3, 2] counts the fixture's flags and splits amount to."""
    counts = np.zeros((3, 2), dtype=np.int64)
    for flag, s in zip(z["eval/correct"].tolist(), z["eval/ref_split"][fixture_rows(meta)].tolist()):
        counts[s] += (int(flag), 1)
    return counts


# ------------------------------------------------------------------------------------------------ fp64 restatement of the IoU rule
def box_eval_restated(coord, ref_row, ref_box, ref_size, ref_split):
    """dataset/utils.py:281-288 + computeIoU (:349-361) + the counting of grounding_eval_bbox (:290-301), written out on whole arrays in
    fp64 from the fp32 inputs.  -> (out fp64 [n, 5] = pixel x, y, w, h and IoU; counts int64 [3, 2]).  A row outside the tables: NaN, counted
    nowhere.  union <= 0: IoU 0."""
    coord = np.asarray(coord, dtype=np.float32).astype(np.float64)
    n, R = coord.shape[0], np.asarray(ref_box).shape[0]
    rows = np.arange(n) if ref_row is None else np.asarray(ref_row, dtype=np.int64)
    live = (rows >= 0) & (rows < R)
    safe = np.where(live, rows, 0)
    box = np.asarray(ref_box, dtype=np.float32).astype(np.float64)[safe]
    size = np.asarray(ref_size, dtype=np.float32).astype(np.float64)[safe]
    split = np.asarray(ref_split, dtype=np.int64)[safe]
    pw, ph = coord[:, 2] * size[:, 0], coord[:, 3] * size[:, 1]
    px, py = coord[:, 0] * size[:, 0] - pw / 2, coord[:, 1] * size[:, 1] - ph / 2
    x1, y1 = np.maximum(box[:, 0], px), np.maximum(box[:, 1], py)
    x2, y2 = np.minimum(box[:, 0] + box[:, 2] - 1, px + pw - 1), np.minimum(box[:, 1] + box[:, 3] - 1, py + ph - 1)
    inter = np.where((x1 < x2) & (y1 < y2), (x2 - x1 + 1) * (y2 - y1 + 1), 0.0)
    union = box[:, 2] * box[:, 3] + pw * ph - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union <= 0, 0.0, inter / np.where(union <= 0, 1.0, union))
    out = np.stack([px, py, pw, ph, iou], axis=1)
    out[~live] = np.nan
    counts = np.zeros((3, 2), dtype=np.int64)
    for s in range(3):
        sel = live & (split == s)
        counts[s] = (int((iou[sel] >= 0.5).sum()), int(sel.sum()))
    return out, counts


# ------------------------------------------------------------------------------------------------ the CPU model path
class OracleGrounding(torch.nn.Module):
    """XFMForGrounding on the CPU: oracle arithmetic, the reference's forward(image, text_ids, text_atts, target_bbox=None)."""

    def __init__(self, state, meta):
        super().__init__()
        from oracle import xfm_oracle as O
        self.O = O
        self.names = list(state)
        self.cfg = O.default_cfg(text_layers=meta["text_layers"], fusion_layers=meta["fusion_layers"], vit_depth=meta["vit_depth"])
        self.init_params = []
        self._flat = {k: f"p{i}" for i, k in enumerate(self.names)}
        for k in self.names:   # `<head>.decoder.bias` IS `<head>.bias` in the reference (tied, xroberta.py:1322-1323): one parameter
            if k.endswith("decoder.bias"):
                self._flat[k] = self._flat[k[: -len("decoder.bias")] + "bias"]
        for k, v in state.items():
            if k.endswith("decoder.bias"):
                continue
            if v.dtype.is_floating_point:
                self.register_parameter(self._flat[k], torch.nn.Parameter(v.clone()))
            else:
                self.register_buffer(self._flat[k], v.clone())

    def table(self):
        return {k: getattr(self, a) for k, a in self._flat.items()}

    def named_parameters(self, *a, **kw):   # under the reference's names: the optimizer groups go by them
        back = {a: k for k, a in self._flat.items() if not k.endswith("decoder.bias")}
        for n, p in super().named_parameters(*a, **kw):
            yield back[n], p

    def forward(self, image, text_ids, text_atts, target_bbox=None, fused=False):
        if fused:
            raise RuntimeError("get_bbox_loss(fused=True) runs on HIP kernels: it needs GPU tensors")
        output_coord = self.O.grounding_forward(self.table(), self.cfg, image, text_ids, text_atts)
        if target_bbox is None:
            return output_coord
        loss_bbox, loss_giou = self.O.bbox_loss(output_coord, target_bbox)
        return output_coord, loss_bbox, loss_giou


def oracle_model(meta):
    return OracleGrounding(state_from_spec(meta["spec"]), meta)


# ------------------------------------------------------------------------------------------------ xfm_box_eval kernel cases
BOX_EVAL_N = (1, 3, 256, 257, 1000)   # one sample; fewer than a wave; exactly the workgroup; one more (a second stride); several strides
KINDS = ("threshold", "random", "disjoint", "one_pixel", "contained", "union0", "split_low", "split_high", "row_low", "row_high")
THRESHOLD_MARGIN = 2.0 ** -20


def _sample(kind, g):
    """-> (coord [4], box [4], size [2], split) of one sample.  Every value is rounded to fp32 here, so the restatement and the kernel see the
    same numbers."""
    split = int(g.integers(0, 3))
    W, H = float(g.integers(100, 700)), float(g.integers(100, 700))
    if kind == "threshold":   # every step exact in binary: pw = 10, ph = 5, px = py = 0, inter = 50, union = 100, IoU = 0.5 exactly
        return [0.25, 0.125, 0.5, 0.25], [0.0, 0.0, 10.0, 10.0], [20.0, 20.0], split
    if kind == "one_pixel":   # px = rx + rw - 1 exactly (W = H = 512, all values dyadic): x1 == x2, no intersection by the strict `<`
        rx, rw, pw = float(g.integers(10, 200)), float(g.integers(20, 100)), 64.0
        px = rx + rw - 1.0
        return [(px + pw / 2) / 512.0, 0.5, pw / 512.0, 0.25], [rx, 192.0, rw, 128.0], [512.0, 512.0], split
    rw, rh = np.floor(W * g.uniform(0.1, 0.6)) + 1, np.floor(H * g.uniform(0.1, 0.6)) + 1
    rx, ry = np.floor(g.uniform(0, W - rw)), np.floor(g.uniform(0, H - rh))
    if kind == "disjoint":    # the reference in the left half, the prediction in the right one
        rw = np.floor(W * g.uniform(0.1, 0.4)) + 1
        rx = np.floor(g.uniform(0, W / 2 - rw))
        w = g.uniform(0.05, 0.4)
        coord = [0.55 + w / 2 + g.uniform(0, 0.4 - w), g.uniform(0.2, 0.8), w, g.uniform(0.1, 0.4)]
    elif kind == "contained":   # the prediction inside the reference (IoU = the ratio of the areas, up to the -1 / +1 of the rule)
        s = g.uniform(0.3, 0.95)
        coord = [(rx + rw / 2) / W, (ry + rh / 2) / H, s * rw / W, s * rh / H]
    elif kind == "union0":    # empty boxes on both sides (union 0), or a negative reference area (union < 0)
        if g.integers(0, 2):
            return [g.uniform(0.1, 0.9), g.uniform(0.1, 0.9), 0.0, 0.0], [rx, ry, 0.0, 0.0], [W, H], split
        return [g.uniform(0.1, 0.9), g.uniform(0.1, 0.9), 0.0, 0.0], [rx, ry, -rw, rh], [W, H], split
    else:                     # a shifted, rescaled copy of the reference: IoU anywhere in (0, 1)
        sx, sy = g.uniform(0.6, 1.5), g.uniform(0.6, 1.5)
        coord = [(rx + rw / 2 + g.uniform(-0.4, 0.4) * rw) / W, (ry + rh / 2 + g.uniform(-0.4, 0.4) * rh) / H, sx * rw / W, sy * rh / H]
    if kind == "split_low":
        split = -1
    elif kind == "split_high":
        split = 3
    return coord, [rx, ry, rw, rh], [W, H], split


def box_case(n, shuffled, seed=0):
    """-> NS(coord fp32 [n, 4], ref_row int32 [n] or None, ref_box fp32 [R, 4], ref_size fp32 [R, 2], ref_split int32 [R], kinds).
    The kinds cycle over KINDS, so from n = 10 on every one occurs.  shuffled: R = n + 3 rows in a random order, and the row_low / row_high
    samples name row -1 / row R.  Not shuffled (ref_row NULL = rows 0 .. n - 1): the table is one row SHORT from n = 2 on, so the last
    sample's row lies outside it.  Asserts that only the constructed threshold samples sit within 2^-20 of IoU 0.5."""
    g = np.random.default_rng(1000 * n + 17 * int(shuffled) + seed)
    kinds = [KINDS[i % len(KINDS)] for i in range(n)]
    samples = [_sample(k, g) for k in kinds]
    coord = np.asarray([s[0] for s in samples], dtype=np.float32)
    if shuffled:
        R = n + 3
        perm = g.permutation(R)
        rows = perm[:n].astype(np.int32)
        spare = [_sample("random", g) for _ in range(R - n)]
        box, size, split = np.zeros((R, 4), np.float32), np.zeros((R, 2), np.float32), np.zeros(R, np.int32)
        for r, s in zip(perm, samples + spare):
            box[r], size[r], split[r] = s[1], s[2], s[3]
        for i, k in enumerate(kinds):
            if k == "row_low":
                rows[i] = -1
            elif k == "row_high":
                rows[i] = R
    else:
        R = max(n - 1, 1)
        rows = None
        box = np.asarray([s[1] for s in samples], dtype=np.float32)[:R]
        size = np.asarray([s[2] for s in samples], dtype=np.float32)[:R]
        split = np.asarray([s[3] for s in samples], dtype=np.int32)[:R]
    out, _ = box_eval_restated(coord, rows, box, size, split)
    for i, k in enumerate(kinds):
        if np.isnan(out[i, 4]):
            continue
        if k == "threshold":
            assert out[i, 4] == 0.5, (i, out[i])
        else:
            assert abs(out[i, 4] - 0.5) > THRESHOLD_MARGIN, (i, k, out[i])
    return NS(coord=coord, ref_row=rows, ref_box=box, ref_size=size, ref_split=split, kinds=kinds, n=n, R=R)


def run_box_eval(case, out_offset=0, calls=1):
    """xfm_box_eval on the GPU, every operand at an unaligned offset inside a poisoned buffer, `out` a NaN-poisoned [.., 5] buffer with two
    rows after the written range -> NS(out [n, 5], counts [3, 2], and what must hold the poison afterwards).  calls = 2: a second call
    with out NULL adds into the same counts."""
    from xfm_amd import functional as Fx
    dev = "cuda"
    POISON_BITS = 0x7FC00123   # a NaN that the kernel's own NaN rows (0x7FC00000) cannot be mistaken for

    def inside(a, before, fill):
        t = torch.from_numpy(np.ascontiguousarray(a))
        parent = torch.full((before + t.numel() + 3,), fill, dtype=t.dtype, device=dev)
        view = parent[before:before + t.numel()]
        view.copy_(t.reshape(-1))
        return view.view(t.shape), parent

    coord, coord_p = inside(case.coord, 1, 9.0e9)
    box, box_p = inside(case.ref_box, 3, 9.0e9)
    size, size_p = inside(case.ref_size, 1, 9.0e9)
    split, split_p = inside(case.ref_split, 1, 1)
    rows, rows_p = inside(case.ref_row, 3, 0) if case.ref_row is not None else (None, None)
    counts_p = torch.full((1 + 6 + 2,), 1234567, dtype=torch.int64, device=dev)
    counts = counts_p[1:7]
    counts.zero_()
    n = case.n
    out_p = torch.full(((out_offset + n + 2) * 5 + 1,), POISON_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    out = out_p[1:].view(out_offset + n + 2, 5)   # (rows start one float into the allocation)
    before = [t.clone() for t in (coord_p, box_p, size_p, split_p)] + ([rows_p.clone()] if rows_p is not None else [])
    Fx.box_eval(coord, rows, box, size, split, counts, out, out_offset)
    for _ in range(calls - 1):
        Fx.box_eval(coord, rows, box, size, split, counts, None, 0)
    torch.cuda.synchronize()
    after = [coord_p, box_p, size_p, split_p] + ([rows_p] if rows_p is not None else [])
    inputs_kept = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                      for a, b in zip(after, before))
    bits = out_p.view(torch.int32)
    lo, hi = 1 + out_offset * 5, 1 + (out_offset + n) * 5
    out_kept = bool((bits[:lo] == POISON_BITS).all()) and bool((bits[hi:] == POISON_BITS).all())
    counts_kept = counts_p[0].item() == 1234567 and counts_p[7:].tolist() == [1234567, 1234567]
    return NS(out=out[out_offset:out_offset + n].cpu().numpy(), counts=counts.view(3, 2).cpu().numpy(), inputs_kept=inputs_kept,
              out_kept=out_kept, counts_kept=counts_kept)


def box_eval_digests():
    """One hex digest of (out, counts) per kernel case, in a fixed order: what the parent and the XFM_DETERMINISTIC=1 child compare."""
    digests = []
    for n in BOX_EVAL_N:
        for shuffled in (False, True):
            r = run_box_eval(box_case(n, shuffled), out_offset=5, calls=2)
            digests.append(hashlib.sha256(r.out.tobytes() + r.counts.tobytes()).hexdigest()[:16])
    return digests


if __name__ == "__main__":
    print("BOX_EVAL " + " ".join(box_eval_digests()), flush=True)
