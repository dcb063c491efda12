"""fp64 restatements, elementwise error bounds and case builders for the Grad-CAM kernels (test infrastructure; any device):
xfm_xattn_gradcam (csrc/gradcam.hip) and xfm_cam_box_rank (csrc/grounding.hip).  Poison, sentinels and the checkers are
gemm_strided_util's; the method is attention_util's: every reference is the fp64 value of what the kernel computes from its ACTUAL bf16 /
fp32 inputs, next to a bound on a correct fp32 evaluation's error, one term per rounding (u32 = 2^-23 = two fp32 unit roundoffs; a sum of
n terms is charged n u32 relative to sum |term|, whatever its order).

xfm_xattn_gradcam, per (b, h), head_dim 64, from the GIVEN fp32 lse:
    x  = scale q.k - lse        e_x  = u32 (C_K scale sum_d |q_d k_d| + |lse|)
                                the 64 products of bf16 operands are exact, their 64 fp32 MFMA additions are charged 64 u32 (C_K = 66 as
                                in attention_util: two more for the fma); the fma with the scale and the subtraction of lse are ONE
                                rounding of a value of at most scale sum |q k| + |lse|
    P  = exp(x)                 e_P  = P (e_x + E_EXP u32): the argument's error moves exp by its own size, relative; expf is within one ulp
                                (1 u32) -- counted as E_EXP = 2 as in attention_util.  (No 1.5 |x| term: that one belongs to
                                __expf = v_exp(x log2 e), the kernel calls expf.)
    dP = dO.v                   e_dP = 64 u32 sum_d |dO_d v_d|       (64 additions; no further rounding)
    term = P max(dP, 0)         |max(a, 0) - max(b, 0)| <= |a - b|: e_term = e_P max(dP, 0) + P e_dP
    cam = sum_{h, t} term / (H t_div)
                                e_cam = [sum e_term + (N + 2) u32 sum |term|] / (H t_div), N = H Sq terms: one fma per term (its product
                                and its addition are one rounding, charged with the N additions), the two lane exchanges' additions, and
                                the division.
    Rows t >= q_len[b]: P and dP exactly 0.  An entry whose source is outside [0, n_src): zeros.

xfm_cam_box_rank: see box_rank_ref (fp64 from the same fp32 tap weights: only the order of fp64 sums differs) and interp_scores (the
reference's own recipe: F.interpolate on the CPU, then the Python loop of dataset/utils.py:193-201)."""

import numpy as np
import torch

from attention_util import C_K, E_EXP, chunks, stat_ld
from gemm_strided_util import NAN, SENTINEL, U32, embed, embed_vec  # noqa: F401

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
SCALE = 0.125

# (B, H, Sq, Sk) of the issue; lens: one per entry (the ragged forms), kv_src: permutation / shared source / own
SHAPES = {"s37": (3, 2, 64, 37), "s197": (2, 12, 40, 197), "s577": (2, 12, 33, 577)}
LENS = {"s37": (64, 17, 1), "s197": (16, 5), "s577": (33, 17)}
KV_SRC = {"s37": ((2, 0, 1), 3), "s197": ((1, 1), 2), "s577": (None, 2)}   # (index per entry, number of sources)
MODES = ("dense", "dense_len", "packed")


def _randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F32)


def make_case(name, mode, seed=7):
    """Operands on the CPU: q / dout rows [rows, H*64] bf16, kv [n_src*Sk, 2*H*64] bf16, the entries' (start, len), kv_src."""
    B, H, Sq, Sk = SHAPES[name]
    idx, n_src = KV_SRC[name]
    D = H * 64
    lens = (Sq,) * B if mode == "dense" else LENS[name]
    if mode == "packed":   # the entries back to back, two slack rows between them and three in front
        start, at = [], 3
        for n in lens:
            start.append(at)
            at += n + 2
        rows = at
    else:
        start, rows = [b * Sq for b in range(B)], B * Sq
    q = (_randn((rows, D), seed) * 1.5).to(BF16)
    dout = _randn((rows, D), seed + 1).to(BF16)
    kv = torch.cat([(_randn((n_src * Sk, D), seed + 2) * 1.5), _randn((n_src * Sk, D), seed + 3)], dim=1).to(BF16)
    return dict(name=name, mode=mode, B=B, H=H, Sq=Sq, Sk=Sk, D=D, n_src=n_src, lens=lens, start=start, q=q, dout=dout, kv=kv,
                kv_src=idx, t_div=Sq + 3)


def gradcam_ref(c, lse_given=None, bad_src=()):
    """-> dict of fp64 tensors: lse (the exact one), P, dP, cam and the bounds bP, bdP, bcam; from lse_given (fp32 [B, H, >= Sq]) when
    passed, else from the exact lse rounded to fp32 (returned as lse32)."""
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    q, do, kv = c["q"].double(), c["dout"].double(), c["kv"].double()
    P, dP = torch.zeros(B, H, Sq, Sk, dtype=F64), torch.zeros(B, H, Sq, Sk, dtype=F64)
    bP, bdP = torch.zeros_like(P), torch.zeros_like(P)
    lse = torch.zeros(B, H, Sq, dtype=F64)
    lse32 = torch.full((B, H, stat_ld(Sq)), NAN, dtype=F32)
    for b in range(B):
        n, s0 = c["lens"][b], c["start"][b]
        src = b if c["kv_src"] is None else c["kv_src"][b]
        if b in bad_src:
            continue
        for h in range(H):
            qh, dh = q[s0:s0 + n, h * 64:(h + 1) * 64], do[s0:s0 + n, h * 64:(h + 1) * 64]
            kh = kv[src * Sk:(src + 1) * Sk, h * 64:(h + 1) * 64]
            vh = kv[src * Sk:(src + 1) * Sk, D + h * 64:D + (h + 1) * 64]
            s = SCALE * (qh @ kh.t())
            mag = SCALE * (qh.abs() @ kh.abs().t())
            lse[b, h, :n] = torch.logsumexp(s, dim=1)
            if lse_given is None:
                lse32[b, h, :n] = lse[b, h, :n].float()
                lg = lse32[b, h, :n].double()
            else:
                lg = lse_given[b, h, :n].double()
            x = s - lg[:, None]
            e_x = U32 * (C_K * mag + lg.abs()[:, None])
            P[b, h, :n] = torch.exp(x)
            bP[b, h, :n] = P[b, h, :n] * (e_x + E_EXP * U32)
            dP[b, h, :n] = dh @ vh.t()
            bdP[b, h, :n] = 64 * U32 * (dh.abs() @ vh.abs().t())
    relu = dP.clamp(min=0)
    term = P * relu
    div = float(H * c["t_div"])
    cam = term.sum(dim=(1, 2))[:, 1:] / div
    bcam = ((bP * relu + P * bdP).sum(dim=(1, 2)) + (H * Sq + 2) * U32 * term.sum(dim=(1, 2)))[:, 1:] / div
    return dict(lse=lse, lse32=lse32, P=P, dP=dP, cam=cam, bP=bP, bdP=bdP, bcam=bcam)


def fwd_lse_bound(c, ref):
    """The bound of the lse that xfm_attn_fwd's grouped route leaves (attention_util's header, the grouped kernels' counts):
    e_s = u32 (C_K scale sum |q k|) + 2 u32 (|s| + |lse|), e_p = e_s + u32 (1.5 |s - rowmax| + E_EXP),
    e_lse = sum_j P e_p + u32 (|lse| + Sk + 8 chunks)."""
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    q, kv = c["q"].double(), c["kv"].double()
    out = torch.zeros(B, H, Sq, dtype=F64)
    for b in range(B):
        n, s0 = c["lens"][b], c["start"][b]
        src = b if c["kv_src"] is None else c["kv_src"][b]
        for h in range(H):
            qh = q[s0:s0 + n, h * 64:(h + 1) * 64]
            kh = kv[src * Sk:(src + 1) * Sk, h * 64:(h + 1) * 64]
            s = SCALE * (qh @ kh.t())
            mag = SCALE * (qh.abs() @ kh.abs().t())
            lse = ref["lse"][b, h, :n]
            e_s = U32 * C_K * mag + 2 * U32 * (s.abs() + lse.abs()[:, None])
            e_p = e_s + U32 * (1.5 * (s - s.max(dim=1, keepdim=True).values).abs() + E_EXP)
            P = torch.exp(s - lse[:, None])
            out[b, h, :n] = (P * e_p).sum(dim=1) + U32 * (lse.abs() + Sk + 8 * chunks(Sk))
    return out


class GradcamBuffers:
    """The operands inside poisoned parents on `device`: q and dout as column slices (8 columns in, 4 rows down) of NaN-filled bf16
    parents, k | v the two halves of ONE NaN-bordered parent, lse [B, H, stat_ld] with NaN in its padding and past every length, the three
    outputs inside SENTINEL-filled vectors."""

    def __init__(self, c, lse32, device):
        B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
        self.c = c
        self.q, self.q_parent = embed(c["q"].to(device), D + 16, 8, 4, 3, NAN)
        self.dout, self.do_parent = embed(c["dout"].to(device), D + 24, 16, 4, 3, NAN)
        kv, self.kv_parent = embed(c["kv"].to(device), 2 * D + 8, 8, 4, 3, NAN)
        self.k, self.v = kv[:, :D], kv[:, D:]
        self.lse = lse32.to(device).contiguous()
        dev_i32 = lambda v: torch.tensor(v, dtype=I32, device=device)   # noqa: E731
        self.q_start = dev_i32(c["start"]) if c["mode"] == "packed" else None
        self.q_len = dev_i32(c["lens"]) if c["mode"] != "dense" else None
        self.kv_src = dev_i32(c["kv_src"]) if c["kv_src"] is not None else None
        self.device = device

    def outputs(self, cam, p_out, dp_out):
        c = self.c
        B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
        # (the outputs start as NaN: an element the kernel leaves unwritten fails every bound)
        mk = lambda n, on: embed_vec(torch.full((n,), NAN, dtype=F32, device=self.device), 8, 8, SENTINEL) if on else (None, None)   # noqa: E731
        return mk(B * (Sk - 1), cam), mk(B * H * Sq * Sk, p_out), mk(B * H * Sq * Sk, dp_out)

    def args(self, _lib, cam, p, dp, **over):
        c = self.c
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        kw = dict(q=self.q.data_ptr(), q_rs=self.q.stride(0), dout=self.dout.data_ptr(), do_rs=self.dout.stride(0),
                  k=self.k.data_ptr(), k_rs=self.k.stride(0), v=self.v.data_ptr(), v_rs=self.v.stride(0),
                  lse=self.lse.data_ptr(), stat_ld=self.lse.shape[-1], q_start=ptr(self.q_start), q_len=ptr(self.q_len),
                  kv_src=ptr(self.kv_src), n_src=c["n_src"], B=c["B"], H=c["H"], Sq=c["Sq"], Sk=c["Sk"], scale=SCALE,
                  t_div=c["t_div"], cam=ptr(cam), p_out=ptr(p), dp_out=ptr(dp))
        kw.update(over)
        return _lib.GradcamArgs(**kw)


# ------------------------------------------------------------------------------------------------------------------ box ranking
def tap_weights(n_out, n_in):
    """ATen's bicubic taps (align_corners=False, A = -0.75) in fp32, operation by operation (numpy rounds every fp32 operation on its own)
    -> (idx [n_out, 4], w fp32 [n_out, 4])."""
    f = np.float32
    A = f(-0.75)
    scale = f(n_in) / f(n_out)
    real = scale * (np.arange(n_out).astype(np.float32) + f(0.5)) - f(0.5)
    i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    t = np.minimum(np.maximum(real - i0.astype(np.float32), f(0.0)), f(1.0))
    x0, x2 = t + f(1.0), f(1.0) - t
    x3 = x2 + f(1.0)
    c2 = lambda x: ((A * x - f(5.0) * A) * x + f(8.0) * A) * x - f(4.0) * A   # noqa: E731
    c1 = lambda x: ((A + f(2.0)) * x - (A + f(3.0))) * x * x + f(1.0)         # noqa: E731
    w = np.stack([c2(x0), c1(t), c1(x2), c2(x3)], axis=1)
    assert w.dtype == np.float32 and real.dtype == np.float32
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, w


def _bound(v, hi):
    return hi if v >= hi else (int(v) if v > 0 else 0)


def _axis_sums(lo, ext, size, p, taps):
    idx, w = taps
    s0, s1 = _bound(lo, size), _bound(lo + ext, size)
    a, mag = np.zeros(p), np.zeros(p)
    if s1 > s0:
        np.add.at(a, idx[s0:s1].ravel(), w[s0:s1].ravel().astype(np.float64))
        np.add.at(mag, idx[s0:s1].ravel(), np.abs(w[s0:s1].ravel().astype(np.float64)))
    return a, mag


def iou_ref(r, d):
    x1, y1 = max(r[0], d[0]), max(r[1], d[1])
    x2, y2 = min(r[0] + r[2] - 1, d[0] + d[2] - 1), min(r[1] + r[3] - 1, d[1] + d[3] - 1)
    inter = (x2 - x1 + 1) * (y2 - y1 + 1) if x1 < x2 and y1 < y2 else 0.0
    union = r[2] * r[3] + d[2] * d[3] - inter
    return 0.0 if union <= 0 else inter / union


def box_scores_ref(cam, hw, dets, alpha):
    """fp64 scores of one ref's boxes from the fp32 tap weights -> (score [k], mag [k]): mag = |a|^T |cam| |b| / area^alpha, the size of
    what the sums add up (every bound below is a multiple of it)."""
    p = cam.shape[0]
    cam64 = cam.astype(np.float64)
    ty, tx = tap_weights(hw[0], p), tap_weights(hw[1], p)
    sc, mg = np.zeros(len(dets)), np.zeros(len(dets))
    for d, (x, y, w, h) in enumerate(dets):
        a, am = _axis_sums(y, h, hw[0], p, ty)
        b, bm = _axis_sums(x, w, hw[1], p, tx)
        area = (w * h) ** alpha
        sc[d] = (a @ (cam64 @ b)) / area
        mg[d] = (am @ (np.abs(cam64) @ bm)) / area
    return sc, mg


def interp_scores(cam, hw, dets, alpha):
    """The reference's recipe on the CPU: F.interpolate(mode='bicubic') to (height, width), then the slice sums of utils.py:196-198 (the
    fp32 pixels summed in fp64, so the only fp32 roundings are the interpolation's own)."""
    p = cam.shape[0]
    m = torch.nn.functional.interpolate(torch.from_numpy(cam).view(1, 1, p, p), size=(int(hw[0]), int(hw[1])), mode='bicubic').squeeze(0).squeeze(0)
    out = []
    for (x, y, w, h) in dets:
        sl = m[int(y):int(y + h), int(x):int(x + w)]
        out.append(float(sl.double().sum()) / (w * h) ** alpha)
    return np.asarray(out)


def pick_first_max(scores):
    best, pick = 0.0, -1
    for d, s in enumerate(scores):
        if s > best:
            best, pick = s, d
    return pick, best


# Bounds of a score, as multiples of `mag` (box_scores_ref):
#   kernel vs box_scores_ref: the same fp32 weights, fp64 sums in another order -- (rows + columns + p^2 + p) additions and products of
#   2^-53 each, and pow's ulp: charged (h + w + p p + p + 4) 2^-52.
#   F.interpolate vs box_scores_ref: every output pixel is 4 products wy (sum of 4 products wx cam) in fp32: 4 + 4 additions and 2
#   products deep, charged 10 u32 relative to the pixel's sum |wy wx cam| -- and the sum over the box's pixels of those is `mag`.
def kernel_score_bound(mag, hw, p):
    return (hw[0] + hw[1] + p * p + p + 4) * 2.0 ** -52 * mag


INTERP_COUNT = 10


def interp_score_bound(mag):
    return INTERP_COUNT * U32 * mag


# ---- cases of the box-rank tests: per p, five refs -- a small image with a box over the border and one whose slice is empty; a 480 x 640
# image with 256 boxes; a 5 x 7 image (smaller than the map) with one box; tied scores (the best box twice: the first must win); a ref
# with no positive score (a negative map, and a box outside the image whose score is exactly 0)
BOX_P = (6, 14, 24, 30)


def _uniform(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g, dtype=F64).numpy()


def _rand_boxes(k, hw, seed):
    u = _uniform(k * 4, seed).reshape(k, 4)
    H, W = hw
    w, h = 1.0 + u[:, 2] * 0.7 * W, 1.0 + u[:, 3] * 0.7 * H
    x, y = u[:, 0] * (W - 1), u[:, 1] * (H - 1)       # (about a third of them overrun the border)
    return np.stack([x, y, w, h], axis=1)


def box_rank_case(p, alpha=0.5):
    """-> dict(cam fp32 [5, p, p], hw int [5, 2], dets list of [k, 4] fp64, ref_box [5, 4], split [5])."""
    g = torch.Generator().manual_seed(100 + p)
    cam = torch.rand((5, p, p), generator=g, dtype=F32).numpy()
    cam[4] = -cam[4] - np.float32(0.01)
    hw = np.array([[37, 53], [480, 640], [5, 7], [37, 53], [37, 53]], dtype=np.int32)
    dets = [_rand_boxes(5, hw[0], 11 * p), _rand_boxes(256, hw[1], 13 * p), np.array([[1.25, 0.5, 4.0, 3.75]]),
            _rand_boxes(4, hw[3], 17 * p), _rand_boxes(3, hw[4], 19 * p)]
    dets[0][1] = (50.6, 30.2, 9.0, 11.0)      # over both borders
    dets[0][3] = (53.5, 3.0, 4.0, 4.0)        # columns 53 : 57 of a 53-wide image: an empty slice, score exactly 0
    sc, _ = box_scores_ref(cam[3], hw[3], dets[3], alpha)
    best = dets[3][int(np.argmax(sc))].copy()
    others = [d for i, d in enumerate(dets[3]) if i != int(np.argmax(sc))]
    dets[3] = np.stack([others[0], best, best, others[1], others[2]])
    dets[4] = np.concatenate([dets[4], np.array([[60.0, 2.0, 3.0, 3.0]])])   # outside the image: exactly 0, still no positive score
    ref_box = np.stack([d[min(1, len(d) - 1)] for d in dets]) + np.array([0.5, -0.25, 1.0, 2.0])
    ref_box[1] = dets[1][0]
    return dict(p=p, cam=cam, hw=hw, dets=dets, ref_box=ref_box, split=np.array([0, 1, 2, 0, 1], dtype=np.int32), alpha=alpha)


def box_rank_expect(case, bound_of):
    """Scores, picks and the margin check of every ref against `bound_of(mag, hw, p)`: the pick is decided (every other DISTINCT box is
    further away than twice the bound, and a ref without a pick has every score <= -bound or exactly 0) -- asserted for every ref, none
    left out.  -> list of (scores, mags, pick, best, iou)."""
    out = []
    for i in range(len(case["dets"])):
        d = case["dets"][i]
        sc, mg = box_scores_ref(case["cam"][i], case["hw"][i], d, case["alpha"])
        bd = np.array([bound_of(m, case["hw"][i], case["p"]) for m in mg])
        pick, best = pick_first_max(sc)
        if pick >= 0:
            for j in range(len(d)):
                if not np.array_equal(d[j], d[pick]):
                    assert best - sc[j] > 2 * (bd[j] + bd[pick]), (case["p"], i, j, best, sc[j], bd[j])
            assert best > 2 * bd[pick]
            assert pick == min(j for j in range(len(d)) if np.array_equal(d[j], d[pick]))
        else:
            assert all(s == 0.0 or s < -2 * b for s, b in zip(sc, bd)), (case["p"], i)
        iou = iou_ref(case["ref_box"][i], d[pick]) if pick >= 0 else 0.0
        assert pick < 0 or abs(iou - 0.5) > 1e-9
        out.append((sc, mg, pick, best, iou))
    return out


def run_box_rank(case, device, calls=1, out_offset=0):
    """One xfm_cam_box_rank pass over the case's refs on `device` -> (out fp64 [n, 3], counts [3, 2], everything around them kept)."""
    from xfm_amd import functional as Fx
    n = len(case["dets"])
    start = np.zeros(n + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(d) for d in case["dets"]])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    out_parent = torch.full((out_offset + n + 2, 3), SENTINEL, dtype=F64, device=device)
    counts = torch.zeros(3, 2, dtype=torch.int64, device=device)
    for _ in range(calls):
        Fx.cam_box_rank(dev(case["cam"]), dev(case["hw"]), dev(np.concatenate(case["dets"])), dev(start), max(len(d) for d in case["dets"]),
                        dev(case["ref_box"]), dev(case["split"]), case["alpha"], counts, out_parent, out_offset)
    torch.cuda.synchronize()
    o = out_parent.cpu().numpy()
    kept = bool((o[:out_offset] == SENTINEL).all() and (o[out_offset + n:] == SENTINEL).all())
    return o[out_offset:out_offset + n], counts.cpu().numpy(), kept


def _digest(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def gradcam_digests(device="cuda"):
    """Bits of every output of the isolation cases and of the box-rank cases (compared across XFM_DETERMINISTIC settings)."""
    from xfm_amd import _lib
    import ctypes
    lib = _lib.load()
    out = []
    for name in SHAPES:
        for mode in MODES:
            c = make_case(name, mode)
            ref = gradcam_ref(c)
            bufs = GradcamBuffers(c, ref["lse32"], device)
            (cam, _), (p, _), (dp, _) = bufs.outputs(True, True, True)
            a = bufs.args(_lib, cam, p, dp)
            assert lib.xfm_xattn_gradcam(ctypes.byref(a), None) == 0
            torch.cuda.synchronize()
            out += [_digest(cam), _digest(p), _digest(dp)]
    for p in BOX_P:
        o, cnt, _ = run_box_rank(box_rank_case(p), device)
        out += [_digest(torch.from_numpy(o.copy())), _digest(torch.from_numpy(cnt.copy()))]
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("GRADCAM " + " ".join(gradcam_digests()))
