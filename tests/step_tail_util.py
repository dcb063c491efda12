"""fp64 references and elementwise error bounds of the kernels at the tail of a training step (test infrastructure; any device): the
contrastive family (contrastive.hip: rownorm, itc_fwd / itc_bwd / itc_dtemp, hard_neg) and the optimizer family (optimizer.hip: adamw in
both rules, sumsq).  Poison, sentinels and the checkers are gemm_strided_util's, poisoned_in / Outs rowwise_util's; the case builders at
the end are shared by the host and GPU tests.

Every reference returns (ref, b32) pairs: the fp64 value of what the kernel computes from its ACTUAL fp32 inputs, and a bound on a correct
fp32 evaluation's error, one U32 term per rounding (U32 = 2^-23 = two fp32 unit roundoffs, so a count of n U32 grants 2n roundings).  A sum
of n terms is charged n roundings relative to sum |term|, whatever its order: the bounds do not encode the kernels' reduction trees.  Scalars
that cross the C ABI as `float` (lr, wd, beta*, eps, bc1, bc2, and temp / clip / g, which are fp32 on the device) are rounded to fp32 first
(f32()).  The build contracts FMAs, so no bound assumes that a product was rounded: a count is an upper limit.  __expf / __logf are charged
as rowwise_util.ce_bwd_ref charges them: exp(a) is off by U32 (|a| + 4) relative.

rownorm forward, y = x / max(|x|, 1e-12f), inv = 1 / max(|x|, 1e-12f) of a row of E elements:
    inv     inv (E/2 + 2) U32     (s = sum x^2: E roundings relative to s, every term >= 0; the root halves them and rounds; the division)
    y       |y| (E/2 + 3) U32     (one product more)
    A row whose norm is far below the floor (the all-zero row, the row times 1e-20, whose squares are subnormal) has n = 1e-12f exactly.
rownorm backward from the GIVEN y and inv:  s = dy . y,  dx = (dy - y s) inv:
    dx      |inv| (|y| E U32 sum |dy y| + 3 U32 (|dy| + |y s|))      (the product, the subtraction, the product with inv)

itc, L = (I . T) / temp over N rows of width E:
    logits  eL = E U32 sum_k |a_k b_k| / temp     (E products summed; 1 / temp and the product with it sit in the count's factor two)
    lse     U32 (|lse| + N + 90) + max_j eL       (rowwise_util's lse bound; the logit error enters as an absolute term)
    cnt     exact (a count of at most N <= 16000 ones)
    term_r  = (lse_r - pos_r) / 2N, pos_r = L_rr or the mean of the cnt_r positives' logits:
            (b_lse + e_pos + 2 U32 (|lse| + |pos|)) / 2N,   e_pos = mean eL + (cnt + 1) U32 mean |L| over the positives
    loss    = sum of the 2N terms: sum b_term + 2N U32 sum |term|
itc backward from the GIVEN lse and cnt, a1 = L - lse_r, a2 = L - lse_c, G = exp(a1) + exp(a2) - label, gs = g / 2N:
    eG      = sum_k exp(a_k) (eL + U32 (|a_k| + 4)) + U32 (2 (exp a1 + exp a2) + 4 label) + 2^-126
            (the two additions; the label 1 / cnt_r + 1 / cnt_j is two divisions and an addition, without idx it is exact)
    dL      = G gs:  e_dL = gs (eG + 2 U32 |G|)     (gs's division, the product)
    dI      = dL . T / temp:  (e_dL . |T| + N U32 |dL| . |T|) / temp + 2 U32 |dI|;   dT the same with dL^T and I
    dtemp   = d0 - gs sum_ij G L / temp:  gs / temp (sum (eG |L| + |G| eL) + (2N + 8) U32 sum |G L|) + U32 max(|d0|, |dtemp|)
            (a row's N products summed, the N row shares summed, the products with gs and 1 / temp, the += onto d0)

hard_neg: the draw of block b is u = (rng_u32(rng_row_key(seed, b), 0) >> 8) / 2^24 (mix32 / rng_row_key / rng_u32 replicate common.h with
    Python integers); image row r uses block r, text row r block B + r.  Weights w = softmax(L_r) + 1e-5f, same-id entries zeroed, c their
    running sum, W = c[B - 1].  The kernel picks the first j with w_j > 0 and u W < c_j in fp32, so its c_j is off by at most
    delta = (B + 30) U32 W: B additions of the scan, B of W itself in the count's factor two; exp of an argument in [-8, 0] 12 U32, the
    division by the sum, the + 1e-5, the product u W.  check_draw accepts a pick iff 0 <= pick < B, w[pick] > 0 and
    c[pick - 1] - delta <= u W < c[pick] + delta, and asserts delta / W <= 1e-4: the widening admits neighbours holding at most 2e-4 of
    the mass.  The cases make the logits exact in fp32 (hard_neg_case), so the draw is a function of the seed alone.

adamw, per element, g' = g clip:  m' = b1 m + (1 - b1) g',  v' = b2 v + (1 - b2) g'^2   (1 - b of an fp32 b in [0.5, 1] is exact)
    m'      e_m = U32 (2 |b1 m| + 3 |(1 - b1) g'|)      -- relative to the TERMS: what is left when they cancel is charged in full
    v'      e_v = U32 (2 b2 v + 5 (1 - b2) g'^2),  r_v = e_v / v'  (0 where v' = 0)
    update  transformers: u = lr sqrt(bc2) / bc1 m' / (sqrt v' + eps);   torch: u = lr / bc1 m' / (sqrt v' / sqrt bc2 + eps);  with den the
            denominator and q the sqrt(v') part of it:  e_u = |step| / den e_m + |u| (r_v / 2 (q / den) + 7 U32)
            (m' error through the quotient; the root halves v' relative error, of which q / den reaches u; seven roundings: the root(s),
            the step's product and division, + eps, the product with m', the division)
    p'      transformers: p1 = p - u, p' = p1 - lr wd p1:  e_u + 2 U32 lr wd P + 2 U32 P       P = max(|p|, |p1|, |p'|)
            torch:        p0 = p (1 - lr wd), p' = p0 - u:  e_u + 2 U32 lr wd P + 3 U32 P
            (lr wd and its product with p; one U32 P per rounding at p's own magnitude: the two subtractions, and in the torch rule 1 - lr wd
            and the product with it.  Elementwise throughout: nothing is relative to max |p|, so the decay lr wd |p| = 1e-5 |p| of the first
            group stands 40 times above the 2.4e-7 |p| granted.)
sumsq:      out = out0 + sum x^2:  (n + 260) U32 sum x^2 + U32 |out0|      (n terms; 256 lanes and 4 waves of tree; the final +=)"""
import torch

from gemm_strided_util import NAN, SENTINEL, U32, assert_outside_untouched, check_f32, embed_vec  # noqa: F401
from rowwise_util import FLUSH, Outs, poisoned_in, randn  # noqa: F401

F32, F64, I64 = torch.float32, torch.float64, torch.int64
WIDTHS = (64, 128, 256, 512, 768, 1024)
LOSS_MAXN = 16000          # XFM_LOSS_MAXN
M32 = 0xFFFFFFFF


def f32(x):
    """a Python number as the fp32 value the C ABI hands the kernel"""
    return float(torch.tensor(x, dtype=F32))


NORM_FLOOR, W_FLOOR = f32(1e-12), f32(1e-5)


def report(where, kernel, case, what, ratio):
    print(f"step-ratio {where} {kernel} {case} {what} {ratio:.3g}")
    return ratio


# ------------------------------------------------------------------------------------------------------------- poisoned buffers
def poisoned_ids(ids, device, fill):
    """an integer vector (idx, group) as a range of a parent filled with `fill`, a VALID id: a read past either end does not fault or
    produce a NaN, it counts for that id"""
    return embed_vec(ids.to(device), 8, 8, fill)[0]


class TailOuts(Outs):
    """rowwise_util.Outs with integer outputs (hard_neg's int64 picks): their surroundings and contents are compared as integers"""

    INT_FILL = -7          # no valid pick: a row the kernel never wrote fails the range check

    def add_ids(self, name, n):
        t = torch.full((n,), self.INT_FILL, dtype=I64, device=self.device)
        v, p = embed_vec(t, 8, 8, self.INT_FILL)
        self.items[name] = (p, v, t.clone())
        return v.data_ptr()

    def check_outside(self):
        for name, (p, v, _) in self.items.items():
            if v.dtype.is_floating_point:
                assert_outside_untouched(p, v, SENTINEL, name)
            else:
                off = v.storage_offset() - p.storage_offset()
                out = torch.cat([p[:off], p[off + v.shape[0]:]])
                assert bool((out == self.INT_FILL).all()), f"{name}: elements outside the view were written"

    def check_unchanged(self):
        self.check_outside()
        for name, (_, v, t0) in self.items.items():
            if not v.dtype.is_floating_point:
                same = torch.equal(v, t0)
            else:
                same = torch.equal(v.contiguous().view(torch.int32), t0.view(torch.int32))
            assert same, f"{name} was written by a rejected call"


def bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ rownorm
def rownorm_fwd_ref(x):
    """{"y": (ref, b32) [R, E], "inv": (ref, b32) [R]}"""
    X = x.double()
    E = X.shape[1]
    inv = 1.0 / (X * X).sum(1).sqrt().clamp_min(NORM_FLOOR)
    y = X * inv.unsqueeze(1)
    return {"y": (y, y.abs() * (E / 2 + 3) * U32), "inv": (inv, inv * (E / 2 + 2) * U32)}


def rownorm_bwd_ref(dy, y, inv):
    """(dx, b32) from the y and inv handed to the kernel"""
    DY, Y, IV = dy.double(), y.double(), inv.double().unsqueeze(1)
    E = Y.shape[1]
    s = (DY * Y).sum(1, keepdim=True)
    sa = (DY * Y).abs().sum(1, keepdim=True)
    dx = (DY - Y * s) * IV
    return dx, IV.abs() * (Y.abs() * E * U32 * sa + 3 * U32 * (DY.abs() + (Y * s).abs()))


# ---------------------------------------------------------------------------------------------------------------------------- itc
def _logits(own, oth, temp):
    """(L, eL) of the rows `own` against all of `oth`, fp64"""
    return own @ oth.t() / temp, own.shape[1] * U32 * (own.abs() @ oth.abs().t()) / temp


def _chunks(rows, chunk):
    return [rows[i:i + chunk] for i in range(0, rows.numel(), chunk)]


def itc_fwd_ref(I, T, temp, idx=None, chunk=2048):
    """{"lse": (ref, b32) [2N] (rows, then columns), "cnt": [N] fp64 or None, "loss": (ref, b32) scalars}; temp: the fp32 device value"""
    Id, Td, t = I.double(), T.double(), float(temp)
    N = Id.shape[0]
    lse, b_lse, term_sum, term_abs, term_b, cnt = [], [], 0.0, 0.0, 0.0, None
    for own, oth in ((Id, Td), (Td, Id)):
        for rows in _chunks(torch.arange(N, device=I.device), chunk):
            L, eL = _logits(own[rows], oth, t)
            l = torch.logsumexp(L, 1)
            bl = U32 * (l.abs() + N + 90) + eL.max(1).values
            if idx is None:
                pos, e_pos = L.gather(1, rows.unsqueeze(1))[:, 0], eL.gather(1, rows.unsqueeze(1))[:, 0]
            else:
                same = (idx[rows].unsqueeze(1) == idx.unsqueeze(0)).double()
                c = same.sum(1)
                pos = (L * same).sum(1) / c
                e_pos = (eL * same).sum(1) / c + (c + 1) * U32 * (L.abs() * same).sum(1) / c
            term = (l - pos) / (2 * N)
            term_sum, term_abs = term_sum + term.sum(), term_abs + term.abs().sum()
            term_b = term_b + ((bl + e_pos + 2 * U32 * (l.abs() + pos.abs())) / (2 * N)).sum()
            lse.append(l)
            b_lse.append(bl)
        if idx is not None and cnt is None:
            cnt = (idx.unsqueeze(1) == idx.unsqueeze(0)).sum(1).double() if N <= 4096 else None
    return {"lse": (torch.cat(lse), torch.cat(b_lse)), "cnt": cnt, "loss": (term_sum.reshape(1), (term_b + 2 * N * U32 * term_abs).reshape(1))}


def _itc_bwd_side(own, oth, lse_own, lse_oth, temp, gs, idx, cnt, rows, grads, chunk):
    """the rows `rows` of one direction: (d_own, b32) or None, and the three sums behind dtemp over those rows"""
    N = own.shape[0]
    out, bnd, S, B1, B2 = [], [], 0.0, 0.0, 0.0
    for rc in _chunks(rows, chunk):
        L, eL = _logits(own[rc], oth, temp)
        a1, a2 = L - lse_own[rc].unsqueeze(1), L - lse_oth.unsqueeze(0)
        p1, p2 = torch.exp(a1), torch.exp(a2)
        if idx is None:
            lab = 2.0 * (rc.unsqueeze(1) == torch.arange(N, device=own.device).unsqueeze(0)).double()
        else:
            lab = (idx[rc].unsqueeze(1) == idx.unsqueeze(0)).double() * (1.0 / cnt[rc].unsqueeze(1) + 1.0 / cnt.unsqueeze(0))
        G = p1 + p2 - lab
        eG = p1 * (eL + U32 * (a1.abs() + 4)) + p2 * (eL + U32 * (a2.abs() + 4)) + U32 * (2 * (p1 + p2) + 4 * lab) + FLUSH
        S, B1, B2 = S + (G * L).sum(), B1 + (eG * L.abs() + G.abs() * eL).sum(), B2 + (G * L).abs().sum()
        if grads:
            dL, e_dL = G * gs, abs(gs) * (eG + 2 * U32 * G.abs())
            ref = dL @ oth / temp
            out.append(ref)
            bnd.append((e_dL @ oth.abs() + N * U32 * (dL.abs() @ oth.abs())) / temp + 2 * U32 * ref.abs())
    return ((torch.cat(out), torch.cat(bnd)) if grads else None), S, B1, B2


def itc_bwd_ref(I, T, temp, lse, g, dtemp0, idx=None, cnt=None, rows=None, chunk=2048):
    """{"dI", "dT", "dtemp": (ref, b32)} from the lse [2N] and cnt [N] handed to the kernel; g, temp: the fp32 device values.  rows: the rows
    of dI and dT to compute (a LongTensor; default all) -- dtemp always covers the whole matrix, a row chunk at a time."""
    Id, Td, t = I.double(), T.double(), float(temp)
    N = Id.shape[0]
    allrows = torch.arange(N, device=I.device)
    ls = lse.double()
    lr_, lc_ = ls[:N], ls[N:2 * N]
    gs = float(g) / (2 * N)
    c = cnt.double() if cnt is not None else None
    sel = allrows if rows is None else rows
    dI, S, B1, B2 = _itc_bwd_side(Id, Td, lr_, lc_, t, gs, idx, c, sel, True, chunk)
    if rows is not None:
        _, S, B1, B2 = _itc_bwd_side(Id, Td, lr_, lc_, t, gs, idx, c, allrows, False, chunk)
    dT = _itc_bwd_side(Td, Id, lc_, lr_, t, gs, idx, c, sel, True, chunk)[0]
    d0 = float(dtemp0)
    dtemp = d0 - gs * S / t
    b = abs(gs) / t * (B1 + (2 * N + 8) * U32 * B2) + U32 * max(abs(d0), abs(float(dtemp)))
    return {"dI": dI, "dT": dT, "dtemp": (dtemp.reshape(1), torch.as_tensor(b, dtype=F64, device=I.device).reshape(1))}


# ----------------------------------------------------------------------------------------------------------------------- hard_neg
def mix32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def rng_row_key(seed_lo, seed_hi, row):
    return mix32((mix32((row ^ seed_lo) & M32) + 0x9E3779B9 * seed_hi + 0x85EBCA6B) & M32)


def rng_u32(row_key, col):
    return mix32((col + row_key) & M32)


def hard_neg_u(seed, first_block, count):
    """fp64 [count]: the uniform draws of blocks first_block .. first_block + count - 1 (image rows: first_block 0, text rows: B)"""
    lo, hi = seed & M32, (seed >> 32) & M32
    return torch.tensor([(rng_u32(rng_row_key(lo, hi, first_block + r), 0) >> 8) / 16777216.0 for r in range(count)], dtype=F64)


def hard_neg_weights(I, T, temp, idx=None):
    """(w_img, w_txt) fp64 [B, B]: row r of w_img weighs the texts for image r, row r of w_txt the images for text r"""
    L = I.double() @ T.double().t() / float(temp)
    B = L.shape[0]
    same = torch.eye(B, dtype=torch.bool, device=L.device) if idx is None else idx.unsqueeze(1) == idx.unsqueeze(0)
    zero = torch.zeros((), dtype=F64, device=L.device)
    return tuple(torch.where(same, zero, torch.softmax(M, 1) + W_FLOOR) for M in (L, L.t()))


def draw_exact(u, w):
    """the fp64 inverse-CDF pick of every row (rows without any weight: -1)"""
    c = torch.cumsum(w, 1)
    x = (u.to(w.device) * c[:, -1]).unsqueeze(1)
    hit = (w > 0) & (x < c)
    B = w.shape[1]
    first = torch.where(hit, torch.arange(B, device=w.device).expand_as(hit), torch.full_like(hit, B, dtype=I64)).min(1).values
    lastpos = torch.where(w > 0, torch.arange(B, device=w.device).expand_as(hit), torch.full_like(hit, -1, dtype=I64)).max(1).values
    return torch.where(first < B, first, lastpos)


def check_draw(pick, u, w, what=""):
    """every row: 0 <= pick < B, w[pick] > 0, c[pick - 1] - delta <= u W < c[pick] + delta (see the header).  Returns the worst
    distance of u W from [c[pick - 1], c[pick]) in units of delta (0: inside the exact interval)."""
    B = w.shape[1]
    pick = pick.to(w.device)
    assert pick.dtype == I64 and pick.shape == (w.shape[0],), (pick.dtype, pick.shape)
    assert bool(((pick >= 0) & (pick < B)).all()), f"{what}: a pick outside [0, {B}): {pick.tolist()}"
    c = torch.cumsum(w, 1)
    W = c[:, -1]
    assert bool((W > 0).all()), f"{what}: a row without any weight"
    delta = (B + 30) * U32 * W
    assert float((delta / W).max()) <= 1e-4, f"{what}: the widening (B + 30) U32 exceeds 1e-4 of the mass"
    wp = w.gather(1, pick.unsqueeze(1))[:, 0]
    assert bool((wp > 0).all()), f"{what}: rows {(wp <= 0).nonzero()[:, 0].tolist()[:8]} picked an entry of weight 0 (past the bound: not drawable)"
    hi = c.gather(1, pick.unsqueeze(1))[:, 0]
    lo = hi - wp
    x = u.to(w.device) * W
    dist = torch.maximum(lo - x, x - hi).clamp_min(0) / delta
    bad = ~((lo - delta <= x) & (x < hi + delta))
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {B} draws past the bound, first row {int(bad.nonzero()[0])}: pick "
                                 f"{int(pick[bad][0])}, u W = {float(x[bad][0])!r} outside [{float(lo[bad][0])!r}, {float(hi[bad][0])!r}) "
                                 f"+- {float(delta[bad][0]):.3g}")
    return float(dist.max())


# -------------------------------------------------------------------------------------------------------------------------- adamw
def adamw_ref(rule, p, g, m, v, gid, lrs, wds, beta1, beta2, eps, bc1, bc2, clip=None):
    """{"p", "m", "v": (ref, b32)}: one step of the rule ("transformers" / "torch", include/xfm_hip.h) on fp32 p, g, m, v; gid: the group id
    of every ELEMENT (int64); lrs / wds the four slots; clip: the fp32 device scalar or None"""
    dev = p.device
    P0, G, M, V = p.double(), g.double(), m.double(), v.double()
    lr = torch.tensor([f32(x) for x in lrs], dtype=F64, device=dev)[gid]
    wd = torch.tensor([f32(x) for x in wds], dtype=F64, device=dev)[gid]
    b1, b2, ep, c1, c2 = f32(beta1), f32(beta2), f32(eps), f32(bc1), f32(bc2)
    gj = G * (1.0 if clip is None else float(clip))
    t1, t2 = b1 * M, (1.0 - b1) * gj
    m1, e_m = t1 + t2, U32 * (2 * t1.abs() + 3 * t2.abs())
    s1, s2 = b2 * V, (1.0 - b2) * gj * gj
    v1, e_v = s1 + s2, U32 * (2 * s1.abs() + 5 * s2.abs())
    rv = torch.where(v1 > 0, e_v / v1.clamp_min(1e-300), torch.zeros_like(v1))
    if rule == "transformers":
        step, q = lr * (c2 ** 0.5) / c1, v1.sqrt()
    else:
        step, q = lr / c1, v1.sqrt() / (c2 ** 0.5)
    den = q + ep
    u = step * m1 / den
    e_u = step.abs() / den * e_m + u.abs() * (0.5 * rv * q / den + 7 * U32)
    if rule == "transformers":
        p1 = P0 - u
        pn = p1 - lr * wd * p1
        big = torch.maximum(torch.maximum(P0.abs(), p1.abs()), pn.abs())
        b_p = e_u + 2 * U32 * lr * wd * big + 2 * U32 * big
    else:
        pn = P0 * (1.0 - lr * wd) - u
        big = torch.maximum(P0.abs(), pn.abs())
        b_p = e_u + 2 * U32 * lr * wd * big + 3 * U32 * big
    return {"p": (pn, b_p), "m": (m1, e_m), "v": (v1, e_v)}


def sumsq_ref(x, out0):
    s = (x.double() ** 2).sum()
    return (s + float(out0)).reshape(1), ((x.numel() + 260) * U32 * s + U32 * abs(float(out0))).reshape(1)


# -------------------------------------------------------------------------------------------------- cases (host and GPU tests alike)
ROWNORM_SHAPES = [(1, 64), (3, 1024), (5, 768), (7, 512), (130, 128), (257, 256)]
ITC_SHAPES = [(1, 64), (3, 1024), (5, 768), (64, 512), (257, 64), (260, 128), (300, 256)]
ITC_TEMPS = (0.07, 0.5)
ITC_G, ITC_DTEMP0 = 1.7, 0.5
HARD_NEG_SHAPES = [(2, 64), (5, 1024), (64, 768), (257, 64), (300, 128), (300, 512)]
HARD_NEG_TEMP = 0.0625
HARD_NEG_SEEDS = (0, 1, 1 << 32, (77 << 32) | 5, (1 << 63) - 1)
ADAMW_SIZES = (256, 1280, 4096 * 1024 + 512)
ADAMW_LR, ADAMW_WD = (1e-3, 3e-3, 1e-4, 1e3), (0.01, 0.2, 0.0, 0.5)
ADAMW_STEPS = (1, 2, 1000)
ADAMW_EPS = 1e-8
# (betas, clip, zero_grad): every value of every option, each clip with each zero_grad
ADAMW_OPTIONS = (((0.9, 0.98), None, 0), ((0.9, 0.999), 0.5, 1), ((0.9, 0.98), 0.5, 0), ((0.9, 0.999), None, 1))
SUMSQ_SIZES = (4, 1020, 1024, 1028, 1024 * 1024 + 4)
BLK_ZERO, BLK_TINY, BLK_CANCEL = 1, 2, 3      # the planted 256-blocks of an AdamW arena with at least five blocks


def rownorm_case(R, E, seed=0):
    """x, dy fp32 [R, E]: from three rows on the last row is all zero, row 1 times 1e-20 (its squares are subnormal: the floor 1e-12 decides)
    and one row times 1e15 (row 2; row 0 at R = 3); R = 1 is one plain row"""
    x, dy = randn((R, E), 1.0, 300 + seed), randn((R, E), 1.0, 301 + seed)
    if R > 2:
        x[1] *= 1e-20
        x[2 if R > 3 else 0] *= 1e15
        x[R - 1] = 0.0
    return {"x": x, "dy": dy}


def rownorm_given(x):
    """the fp32 y and inv handed to the backward: the fp64 reference rounded"""
    ref = rownorm_fwd_ref(x)
    return ref["y"][0].float(), ref["inv"][0].float()


def shared_ids(N, seed):
    """int64 [N]: ids (from 1000 up) shared by about three rows each, in random positions"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randperm(N, generator=g) // 3 + 1000


def itc_case(N, E, with_idx, seed=0):
    """I, T fp32 [N, E]: unit rows, T = I + half a unit of noise (cosine about 0.9 on the diagonal); idx or None"""
    a = randn((N, E), 1.0, 310 + seed).double()
    b = randn((N, E), 1.0, 311 + seed).double()
    a = a / a.norm(dim=1, keepdim=True)
    t = a + 0.5 * b / b.norm(dim=1, keepdim=True)
    return {"I": a.float(), "T": (t / t.norm(dim=1, keepdim=True)).float(), "idx": shared_ids(N, 312 + seed) if with_idx else None}


def itc_plants(N):
    """the columns j at which T_j = I_r is planted in turn (None: nothing planted), and the row r"""
    cols = [None]
    for j in (0, 3, 255, 256, N - 1):
        if 0 <= j < N and j not in cols:
            cols.append(j)
    return cols, min(2, N - 1)


def itc_planted(c, j, r):
    if j is None:
        return c["T"]
    T = c["T"].clone()
    T[j] = c["I"][r]
    return T


def hard_neg_case(B, E, with_idx, seed=0):
    """I, T fp32 [B, E] whose logits at temp = 1/16 are exact in fp32 in any order: every row has 16 entries of +-1/8 (the first 8 columns
    and 8 more random ones) and is zero elsewhere, so every product is +-1/64, every partial sum a multiple of 1/64 below 1, and 1 / temp
    = 16.  The first 8 columns of T are I's: the own entry carries 8/64 more than a stranger's."""
    g = torch.Generator(device="cpu").manual_seed(320 + seed)

    def rows():
        x = torch.zeros((B, E))
        for r in range(B):
            cols = torch.cat([torch.arange(8), 8 + torch.randperm(E - 8, generator=g)[:8]])
            x[r, cols] = (torch.randint(0, 2, (16,), generator=g).float() * 2 - 1) / 8
        return x
    I, T = rows(), rows()
    T[:, :8] = I[:, :8]
    return {"I": I, "T": T, "idx": shared_ids(B, 321 + seed) if with_idx else None}


def adamw_groups(n):
    """(uint8 [n / 256] ids 0, 1, 2 cycling, int64 [n] the id of every element)"""
    blocks = torch.arange(n // 256) % 3
    return blocks.to(torch.uint8), blocks.repeat_interleave(256)


def adamw_state(n, seed=0):
    """p ~ N(0, 1), m ~ N(0, 0.03), v = N(0, 0.1)^2; m = v = 0 in the zero-gradient and the tiny-gradient block"""
    p, m, v = randn((n,), 1.0, 330 + seed), randn((n,), 0.03, 331 + seed), randn((n,), 0.1, 332 + seed) ** 2
    if n >= 5 * 256:
        for blk in (BLK_ZERO, BLK_TINY):
            m[blk * 256:(blk + 1) * 256] = 0.0
            v[blk * 256:(blk + 1) * 256] = 0.0
    return p, m, v


def adamw_grad(n, step, m, beta1, seed=0):
    """the gradient of one step: N(0, 0.1); block 1 zero (with m = v = 0: pure decay), block 2 about 1e-8 = eps (where the rules part),
    block 3 cancels the CURRENT m: beta1 m + (1 - beta1) g is 1e-4 of its terms"""
    g = randn((n,), 0.1, 340 + 7 * step + seed)
    if n >= 5 * 256:
        g[BLK_ZERO * 256:(BLK_ZERO + 1) * 256] = 0.0
        g[BLK_TINY * 256:(BLK_TINY + 1) * 256] = randn((256,), 1e-8, 341 + 7 * step + seed)
        s = slice(BLK_CANCEL * 256, (BLK_CANCEL + 1) * 256)
        b1 = f32(beta1)
        g[s] = (-(b1 / (1.0 - b1)) * m[s].double().cpu() * (1.0 + randn((256,), 1e-4, 342 + 7 * step + seed).double())).float()
    return g


def bias_corrections(beta1, beta2, step):
    return 1.0 - beta1 ** step, 1.0 - beta2 ** step
