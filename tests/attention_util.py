"""fp64 reference, elementwise error bounds, case builders and buffer layout of the attention routes that take a key mask, a causal mask or
dropout (test infrastructure; any device): the PLAIN = false instantiations of attn_fwd_kernel / attn_bwd_dq_kernel<0, ...> /
attn_bwd_dkv_kernel (attention_general.hip), the packed xattn_fwd_kernel<true, ...> and the grouped kernels (attention_grouped.hip).  Poison,
sentinels and the checkers are gemm_strided_util's; the style is rowwise_util's: every reference returns (ref, b32) pairs, the fp64 value of
what the kernel computes from its ACTUAL bf16 / fp32 inputs and a bound on a correct fp32 evaluation's error, one term per rounding.
u32 = 2^-23 is two fp32 unit roundoffs (a count of n u32 grants 2n roundings), u16 = 2^-8 covers one bf16 rounding.  A sum of n terms is
charged n u32 relative to sum |term|, whatever its order: the bounds do not encode the kernels' reduction trees.

Reference, per (b, h), head_dim 64:   s = scale q.k^T + bias + (masked ? -10000 : 0),   masked = (keep == 0) | (causal & kj > qi)
    (-10000 once, whichever reason applies: score_masked in attention_common.h, line 442 of attention_general.hip; kj > qi also for Sq != Sk)
    forward    lse = logsumexp_j s,  P = exp(s - lse),  W = P * dropkeep * ps,  o = W.v          (ps = fp32(1 / (1 - p)), as the kernels hold it)
    backward, from the GIVEN fp32 lse:   P = exp(s - lse),  dP = (dO.v^T) * dropkeep * ps,  delta = sum_j P dP,  dS = P (dP - delta),
               dq = scale dS.k,  dk = scale dS^T.q,  dv = W^T.dO,  dbias += sum_b dS;   dk / dv fold over the query rows that share a source.
    Where a row mixes masked and visible keys, exp(-10000 + ...) is exactly 0 in fp32 and in fp64, so the masked keys' large score error
    never enters a sum (it is multiplied by P = 0).  Where every key of a row is masked, -10000 cancels and the row is an ordinary softmax
    whose scores carry the u32 10000 term.

Counts (each constant is a count of roundings the kernels make, none is fitted to their output):
    score      e_s = u32 (66 scale sum_d |q_d k_d| + |bias| + 10000 masked)
               66 = 64 + 2 as gemm_strided_util's K + 2: the 64 products of bf16 operands are exact, their 64 fp32 MFMA additions are
               charged 64 u32; the fma with the scale and the bias and the addition of the mask term are two more roundings, of a value of
               at most scale sum|q k| + |bias| (+ 10000 when masked): u32 of each magnitude.
               The grouped kernels work in the exponent of 2: fma(raw, fl(scale log2 e), key term) with the key term fl(-10000 log2 e),
               and in the backward fl(-lse log2 e) + key term.  Four more roundings (the two constants' products, the lse product, the
               sum), each of a value of at most |s| + |lse| (+ 10000 masked) in natural units:  e_s += 2 u32 (|s'| + |lse| + 10000 masked),
               s' = the score without the mask term.
    P          relative e_p = e_s + u32 (1.5 |s - rowmax| + E_EXP),  E_EXP = 2
               __expf(a) = v_exp(a fl(log2 e)): the subtraction, the product and the constant's own rounding each move the result by at
               most u |a| relative = 1.5 u32 |a| together.  In the online softmax a = (s - m_chunk) + sum of the alpha exponents
               (m_old - m_new), all of one sign, so sum |a| = |s - rowmax| and the same term covers the alphas' arguments.  E_EXP: v_exp's
               result is within one ulp (1 u32) and the product with ps is one rounding (1/2 u32): 1.5, counted as 2.  (The outline
               this derivation follows has 4 there; no further rounding of P was found in the kernels, so the count stands at 2.)  The
               maximum itself is exact (a selection), and a common factor of a row cancels in the normalisation.
    o          sum_j W_ij |v_jd| (u16 + e_p,ij) + (|o_id| + sum_j W_ij |v_jd|) (sum_j P_ij e_p,ij + (Sk + 8 chunks) u32), then check_bf16
               u16: P is rounded to bf16 before P.V.  Second group: the row sum l carries the P-weighted mean of e_p and its Sk additions;
               o is divided by it (|o| times its relative error); the P.V accumulation is Sk more additions relative to sum W |v|; and per
               64-key chunk one alpha (v_exp's ulp: 1 u32) multiplied into l and into the accumulator (1/2 each) -- 2 of the 8 -- the
               reciprocal of l and the final product (1 + 1/2) sit in the rest.
    lse        sum_j P e_p + u32 (|lse| + Sk + 8 chunks)         (l's relative error is log's absolute one; m + log l and log's own
               v_log . ln 2 are roundings of values of at most |lse| + log Sk)
    backward   e_P = P (e_s + u32 (1.5 |s - lse| + E_EXP))      [the same roundings: the subtraction of the given lse, __expf, x ps]
               e_dP = 66 u32 ps sum_d |dO_d v_d|  (zero where dropped: the select is exact)      [64 additions, the product with ps]
               e_delta = sum_j (e_P |dP| + P e_dP) + Sk u32 sum_j |P dP|                           [Sk products and Sk additions: Sk u32]
               e_dS = e_P |dP - delta| + P (e_dP + e_delta) + 2 u32 |dS|                           [the subtraction, the product]
               dq  scale sum_j |k_jd| (u16 |dS_ij| + e_dS,ij) + (Sk + 2) u32 scale sum_j |k_jd dS_ij|   [dS to bf16; Sk additions, x scale]
               dk  the transpose, summed over the queries: Sq + 2 additions; grouped: over every query row of the source, rows Sq + 2
               dv  sum_i |dO_id| (u16 W_ij + ps e_P,ij) + (Sq + 2) u32 sum_i |dO_id| W_ij
               dq, dk, dv through check_bf16; the dK/dV kernels use the delta the dQ kernel wrote, which is within e_delta of the
               reference's: that is the P e_delta term of e_dS.
               dbias (fp32, +=)  sum_b e_dS + (B + 2) u32 sum_b |dS| + max(1, B / 2) u32 |initial|
               (B additions onto the running value, by atomics or by dbias_reduce_kernel: B roundings of at most |initial| + sum |dS|)
               delta  check_f32 with e_delta.
    row fold (xfm_rows_index_sum): bf16 rows summed in fp32, reference = the fp64 sum of the rows it was given, b32 = R u32 sum |row|.

Layout (AttnBuffers): q, k, v are column slices of ONE NaN-filled [rows + 7, 3 H 64 + 8] bf16 parent (row stride a multiple of 8, slices
on 16-byte boundaries, 4 rows before and 3 after); dO the same in a parent of its own; o, dq, dk, dv, lse, delta, dbias live in
7.0-filled parents whose outside must keep its bits; dbias starts at 0.5 (so += is checked, and its columns [Sk, ld) must be
bit-unchanged); stat_ld = 4 (Sq // 4 + 1), so lse and delta always have padding: the forward must leave it alone, and before the backward
it is NaN in both (the backward must neither read nor write it); the given lse's whole parent must keep its bits; the bias-gradient workspace is exactly xfm_attn_bwd_workspace bytes
inside a sentinel parent."""
from collections import namedtuple

import torch

from gemm_strided_util import (NAN, SENTINEL, U16, U32, assert_outside_untouched, check_bf16, check_f32, embed,  # noqa: F401
                               embed_vec)

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
MASK_NEG = -10000.0
SCALE = 0.125            # 1 / sqrt(64), exact in every format
C_K = 66                 # see the header
E_EXP = 2                # see the header
DBIAS_INIT = 0.5


def drop_scale32(p):
    """1 / (1 - p) as the kernels hold it (an fp32 argument)"""
    return float(torch.tensor(1.0 / (1.0 - p), dtype=F32)) if p > 0.0 else 1.0


def stat_ld(Sq):
    return (Sq // 4 + 1) * 4


def chunks(Sk):
    return (Sk + 63) // 64


# ------------------------------------------------------------------------------------------------------------------------ cases
# route: the forward route the shape reaches (packed | small | resident | streamed | grouped | grouped_stream | kvindex); idx: the key/value
# source of every query batch row (None: its own); mask: key-mask family or None; score: randn | steep; bias: with an additive bias
Spec = namedtuple("Spec", "route B H Sq Sk U idx grouped mask causal p score bias name")
FAMILIES = ("tail", "holes", "chunk0", "one", "all")
SEED = 0x5EED0001CAFE       # dropout seed of every case (seed_hi = 0x5EED, seed_lo = 0x0001CAFE)


def keep_mask(family, U, Sk):
    """int32 [U, Sk], 1 = keep.  tail: a ragged masked tail, entry 0 included; holes: every third key (residue u % 2, so residue 2 is always
    kept); chunk0: keys 0..63; one: a single kept key, in the last 64-key chunk; all: every key of entry 0 masked, the others holes."""
    keep = torch.ones((U, Sk), dtype=I32)
    kj = torch.arange(Sk)
    last0 = 64 * ((Sk - 1) // 64)
    for u in range(U):
        if family == "tail":
            keep[u, Sk - (1 + (7 * u + 3) % max(Sk // 2, 1)):] = 0
        elif family == "holes" or (family == "all" and u > 0):
            keep[u, kj % 3 == u % 2] = 0
        elif family == "chunk0":
            assert Sk >= 130
            keep[u, :64] = 0
        elif family == "one":
            keep[u] = 0
            keep[u, last0 + (5 * u + 1) % (Sk - last0)] = 1
        elif family == "all":
            keep[u] = 0
        else:
            raise ValueError(family)
    return keep


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def make_case(sp):
    """CPU tensors of one case: q, dO [B, Sq, H, 64], k, v [U, Sk, H, 64] bf16, bias fp32 [H, Sq, ld] (columns [Sk, ld) zero, as the
    library's producers leave them) or None, keep int32 [U, Sk] or None, idx int64 [B].
    steep: q = 3 q + 8 e and one kept key of the last chunk (the last kept key where that chunk has none) = 8 e, e = 1/8 in every dimension:
    scores of standard deviation about 3 and a planted key at 8 +- 3, above most rows' other keys, so the running maximum keeps moving
    and ends in the last chunk."""
    B, H, Sq, Sk, U = sp.B, sp.H, sp.Sq, sp.Sk, sp.U
    c = {"sp": sp, "q": _randn((B, Sq, H, 64), 1), "k": _randn((U, Sk, H, 64), 2), "v": _randn((U, Sk, H, 64), 3).to(BF16),
         "do": _randn((B, Sq, H, 64), 4).to(BF16), "bias": None, "keep": None,
         "idx": torch.arange(B) if sp.idx is None else torch.tensor(sp.idx, dtype=torch.int64)}
    if sp.mask is not None:
        c["keep"] = keep_mask(sp.mask, U, Sk)
    if sp.score == "steep":
        c["q"] = 3.0 * c["q"] + 1.0
        kept = torch.ones(Sk, dtype=torch.bool) if c["keep"] is None else (c["keep"] != 0).all(0)
        js = int(kept.nonzero().max())
        c["k"][:, js] = 1.0
    c["q"], c["k"] = c["q"].to(BF16), c["k"].to(BF16)
    if sp.bias:
        ld = (Sk + 3) // 4 * 4 + (4 if Sk <= 256 else 0)       # past 256 keys the workspace route wants ld <= 64 chunks(Sk)
        c["bias"] = torch.zeros((H, Sq, ld))
        c["bias"][:, :, :Sk] = _randn((H, Sq, Sk), 5)
    return c


def to_device(c, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


# (route, B, H, Sq, Sk, U, idx, grouped): each the smallest shape that reaches its route; H = 2 throughout (the head offset).
# Forward: attn_packable = Sq, Sk <= 64, no bias, B >= 2; else launch_attn_fwd with nw = min(ceil(Sq / 16), 8) waves (balanced over blocks),
# LDS-resident when Sk <= 256 and nw >= 4, streamed otherwise.  Backward of every non-plain case: attn_bwd_dq_kernel<0, RES, false> with the
# same geometry and attn_bwd_dkv_kernel<RES', false> with the roles swapped (waves over Sk, resident when Sq <= 256 and >= 4 waves).
SHAPES = [
    ("packed", 3, 2, 30, 30, 3, None, False),         # 2 query tiles a row, 3 rows in one workgroup
    ("packed", 2, 2, 64, 64, 2, None, False),         # the full chunk: 4 tiles a row, 2 rows a workgroup
    ("packed", 3, 2, 17, 50, 3, None, False),         # Sq != Sk, ragged tiles both ways
    ("small", 1, 2, 30, 30, 1, None, False),          # B = 1 keeps it off the packed route: 2 waves -> the streamed instantiation, one chunk
    ("small", 2, 2, 30, 30, 2, None, False),          # run WITH a bias only (below), which keeps it off the packed route
    ("resident", 2, 2, 70, 130, 2, None, False),      # 5 waves, 3 chunks; dK/dV: 2 blocks of 5 waves, 2 query chunks resident
    ("resident", 2, 2, 130, 256, 2, None, False),     # 2 blocks of 5 waves, the 4 chunks the resident form holds
    ("streamed", 2, 2, 40, 300, 2, None, False),      # 3 waves, 5 chunks through the double buffer; dK/dV: 3 blocks of 7 waves
    ("streamed", 2, 2, 130, 321, 2, None, False),     # 2 query blocks, 6 chunks, a last chunk of one key
    ("causal", 2, 2, 30, 30, 2, None, False),         # packed forward
    ("causal", 2, 2, 64, 64, 2, None, False),         # packed forward, full chunk
    ("causal", 2, 2, 65, 65, 2, None, False),         # general resident, a second chunk of one key / one query
    ("causal", 2, 2, 130, 130, 2, None, False),       # resident, the diagonal crosses two chunk boundaries
    ("causal", 2, 2, 300, 300, 2, None, False),       # streamed forward / dQ, and dK/dV streamed too (Sq > 256)
    ("causal", 2, 2, 20, 50, 2, None, False),         # Sq != Sk pins kj > qi (not kj - (Sk - Sq) > qi)
    ("grouped", 5, 2, 30, 130, 2, (1, 0, 1, 1, 0), True),            # xattn_fwd / dq / dkv kernels, keys LDS-resident
    ("grouped_stream", 5, 2, 40, 300, 2, (0, 1, 1, 0, 1), True),     # Sk > 256: the streamed pair + xattn_dkv_kernel
    ("kvindex", 4, 2, 30, 130, 2, (1, 0, 0, 1), False),              # general kernels reading shared sources, per-row dK/dV + row fold
]
# the general kernels, with the bias cases of specs(); the packed and grouped routes reject / never see a bias; kvindex (general kernels
# too) gets one bias case of its own there
TAKES_BIAS = ("small", "resident", "streamed", "causal")


def specs():
    """Every case of the suite.  Per shape: every key-mask family without dropout; causal, causal + tail, causal + all and causal + tail
    with p = 0.1 where square (causal alone at 20 x 50); holes with p = 0.1; one steep case (holes); p = 0.5 (no key mask) once per route.
    Where the route takes a bias: holes, holes with p = 0.1 and causal + tail again with a bias; kv_index: holes with a bias."""
    out, seen_half = [], set()
    for route, B, H, Sq, Sk, U, idx, grouped in SHAPES:
        def add(name, mask=None, causal=False, p=0.0, score="randn", bias=False):
            out.append(Spec(route, B, H, Sq, Sk, U, idx, grouped, mask, causal, p, score, bias, name))

        can_causal = not grouped and idx is None
        only_bias = route == "small" and B == 2
        general = route in TAKES_BIAS and not (Sq <= 64 and Sk <= 64 and B >= 2)
        for fam in FAMILIES:
            if fam != "chunk0" or Sk >= 130:
                add(fam, mask=fam, bias=only_bias)
        if can_causal and (Sq == Sk or route == "causal"):
            add("causal", causal=True, bias=only_bias)
        if can_causal and Sq == Sk:
            add("causal+tail", mask="tail", causal=True, bias=only_bias)
            add("causal+all", mask="all", causal=True, bias=only_bias)     # entry 0: masked AND causally hidden keys, -10000 once
            add("causal+tail+p0.1", mask="tail", causal=True, p=0.1, bias=only_bias)     # decoder training: all three at once
        add("holes+p0.1", mask="holes", p=0.1, bias=only_bias)
        add("steep", mask="holes", score="steep", bias=only_bias)
        if route not in seen_half:
            seen_half.add(route)
            add("p0.5", p=0.5, bias=only_bias)
        if general:
            add("holes+bias", mask="holes", bias=True)
            add("holes+p0.1+bias", mask="holes", p=0.1, bias=True)
            if Sq == Sk:
                add("causal+tail+bias", mask="tail", causal=True, bias=True)
        if route == "kvindex":      # attn_check forbids a bias only for packed rows: the general kernels take one beside kv_index
            add("holes+bias", mask="holes", bias=True)
    return out


def spec_id(sp):
    return f"{sp.route}-{sp.B}x{sp.H}x{sp.Sq}x{sp.Sk}-{sp.name}"


def shape_of(sp):
    return f"{sp.B}x{sp.H}x{sp.Sq}x{sp.Sk}"


# -------------------------------------------------------------------------------------------------------------------- reference
def _heads(t):
    """[N, S, H, 64] -> fp64 [N, H, S, 64]"""
    return t.permute(0, 2, 1, 3).double()


def masked_of(c):
    """bool [B, 1, Sq, Sk]: the scores that get -10000"""
    sp = c["sp"]
    dev = c["q"].device
    m = torch.zeros((sp.B, 1, sp.Sq, sp.Sk), dtype=torch.bool, device=dev)
    if c["keep"] is not None:
        m = m | (c["keep"][c["idx"]] == 0)[:, None, None, :]
    if sp.causal:
        qi, kj = torch.arange(sp.Sq, device=dev)[:, None], torch.arange(sp.Sk, device=dev)[None, :]
        m = m | (kj > qi)[None, None]
    return m


def scores_ref(c, lse_for_grouped=None):
    """(s, e_s) fp64 [B, H, Sq, Sk]"""
    sp = c["sp"]
    Q, K = _heads(c["q"]), _heads(c["k"][c["idx"]])
    s = SCALE * (Q @ K.transpose(-1, -2))
    mag = C_K * SCALE * (Q.abs() @ K.abs().transpose(-1, -2))
    if c["bias"] is not None:
        b = c["bias"][:, :, :sp.Sk].double().unsqueeze(0)
        s, mag = s + b, mag + b.abs()
    masked = masked_of(c).double()
    if sp.grouped:
        lse_mag = 0.0 if lse_for_grouped is None else lse_for_grouped.double().abs().unsqueeze(-1)
        mag = mag + 2 * (s.abs() + lse_mag - MASK_NEG * masked)
    return s + MASK_NEG * masked, U32 * (mag - MASK_NEG * masked)


def _drop(c, M):
    """(keep-and-scale factor fp64 [B, H, Sq, Sk] or 1.0, ps)"""
    p = c["sp"].p
    if p == 0.0:
        assert M is None
        return 1.0, 1.0
    ps = drop_scale32(p)
    return M.double() * ps, ps


def fwd_ref(c, M=None):
    """M: the dropout keep mask, bool [B, H, Sq, Sk] (None without dropout).  -> {"o": (ref [B*Sq, H*64], b32), "lse": (ref [B*H, Sq], b32)}"""
    sp = c["sp"]
    s, e_s = scores_ref(c)
    lse = torch.logsumexp(s, -1)
    if sp.grouped:      # the grouped forward's lse is m ln 2 + log l of exponent-of-2 scores: its scores' error carries |lse| too
        s, e_s = scores_ref(c, lse)
    P = torch.exp(s - lse.unsqueeze(-1))
    e_p = e_s + U32 * (1.5 * (s - s.max(-1, keepdim=True).values).abs() + E_EXP)
    F, _ = _drop(c, M)
    W = P * F
    V = _heads(c["v"][c["idx"]])
    o, mag = W @ V, W @ V.abs()
    nsum = sp.Sk + 8 * chunks(sp.Sk)
    lerr = (P * e_p).sum(-1)
    b_o = (W * (U16 + e_p)) @ V.abs() + (o.abs() + mag) * (lerr + nsum * U32).unsqueeze(-1)
    b_lse = lerr + U32 * (lse.abs() + nsum)
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(sp.B * sp.Sq, sp.H * 64)   # noqa: E731
    return {"o": (rows(o), rows(b_o)), "lse": (lse.reshape(sp.B * sp.H, sp.Sq), b_lse.reshape(sp.B * sp.H, sp.Sq))}


def bwd_ref(c, lse32, M=None):
    """lse32: the fp32 [B*H, Sq] statistics handed to the kernels.  -> (ref, b32) pairs: delta [B*H, Sq], dq [B*Sq, H*64], dk / dv
    [N*Sk, H*64] (N = B per query row for the general kernels, = U folded per source for the grouped ones), dbias [H*Sq, Sk] (with a bias)."""
    sp = c["sp"]
    B, H, Sq, Sk = sp.B, sp.H, sp.Sq, sp.Sk
    lse = lse32.double().reshape(B, H, Sq)
    s, e_s = scores_ref(c, lse)
    d = s - lse.unsqueeze(-1)
    P = torch.exp(d)
    e_P = P * (e_s + U32 * (1.5 * d.abs() + E_EXP))
    F, ps = _drop(c, M)
    Q, K, V, DO = _heads(c["q"]), _heads(c["k"][c["idx"]]), _heads(c["v"][c["idx"]]), _heads(c["do"])
    dP = (DO @ V.transpose(-1, -2)) * F
    e_dP = C_K * U32 * (DO.abs() @ V.abs().transpose(-1, -2)) * F
    PdP = P * dP
    delta = PdP.sum(-1)
    e_delta = (e_P * dP.abs() + P * e_dP).sum(-1) + Sk * U32 * PdP.abs().sum(-1)
    dmd = dP - delta.unsqueeze(-1)
    dS = P * dmd
    e_dS = e_P * dmd.abs() + P * (e_dP + e_delta.unsqueeze(-1)) + 2 * U32 * dS.abs()
    r16 = U16 * dS.abs() + e_dS
    dq = SCALE * (dS @ K)
    b_dq = SCALE * (r16 @ K.abs()) + (Sk + 2) * U32 * SCALE * (dS.abs() @ K.abs())
    W = P * F
    nq = Sq + 2
    if sp.grouped:
        nq = Sq * int(torch.bincount(c["idx"], minlength=sp.U).max()) + 2
    dk = SCALE * (dS.transpose(-1, -2) @ Q)
    b_dk = SCALE * (r16.transpose(-1, -2) @ Q.abs()) + nq * U32 * SCALE * (dS.abs().transpose(-1, -2) @ Q.abs())
    dv = W.transpose(-1, -2) @ DO
    b_dv = (U16 * W + e_P * F).transpose(-1, -2) @ DO.abs() + nq * U32 * (W.transpose(-1, -2) @ DO.abs())
    qrows = lambda t: t.permute(0, 2, 1, 3).reshape(B * Sq, H * 64)   # noqa: E731

    def krows(t):
        if sp.grouped:    # one gradient per source: the sum over its query rows (zero for a source nobody reads)
            t = torch.zeros((sp.U,) + t.shape[1:], dtype=F64, device=t.device).index_add_(0, c["idx"], t)
        return t.permute(0, 2, 1, 3).reshape(t.shape[0] * Sk, H * 64)

    out = {"delta": (delta.reshape(B * H, Sq), e_delta.reshape(B * H, Sq)), "dq": (qrows(dq), qrows(b_dq)),
           "dk": (krows(dk), krows(b_dk)), "dv": (krows(dv), krows(b_dv))}
    if c["bias"] is not None:
        ref = DBIAS_INIT + dS.sum(0)
        b = e_dS.sum(0) + (B + 2) * U32 * dS.abs().sum(0) + max(1.0, B / 2) * U32 * DBIAS_INIT
        out["dbias"] = (ref.reshape(H * Sq, Sk), b.reshape(H * Sq, Sk))
    return out


def fold_ref(rows16, idx, U):
    """(ref, b32) of xfm_rows_index_sum on the bf16 rows [R, len] it was given"""
    X = rows16.double()
    z = torch.zeros((U, X.shape[1]), dtype=F64, device=X.device)
    return z.clone().index_add_(0, idx, X), X.shape[0] * U32 * z.index_add_(0, idx, X.abs())


# ------------------------------------------------------------------------------------------------------------------------ layout
def _nan_bits(t):
    return torch.equal(t.contiguous().view(torch.int32), torch.full_like(t, NAN).contiguous().view(torch.int32))


class AttnBuffers:
    """The operands of one case on `device`, laid out as the header says.  Pointers and strides go into xfm_attn_args by name."""

    def __init__(self, c, device):
        sp = c["sp"]
        self.sp, self.dev = sp, device
        B, H, Sq, Sk, U = sp.B, sp.H, sp.Sq, sp.Sk, sp.U
        D = H * 64
        self.D, self.ld_stat = D, stat_ld(Sq)
        rows = max(B * Sq, U * Sk)
        self.qkv = torch.full((rows + 7, 3 * D + 8), NAN, dtype=BF16, device=device)
        self.q = self.qkv[4:4 + B * Sq, 8:8 + D]
        self.k = self.qkv[4:4 + U * Sk, 8 + D:8 + 2 * D]
        self.v = self.qkv[4:4 + U * Sk, 8 + 2 * D:8 + 3 * D]
        self.q.copy_(c["q"].reshape(B * Sq, D))
        self.k.copy_(c["k"].reshape(U * Sk, D))
        self.v.copy_(c["v"].reshape(U * Sk, D))
        self.do, self.do_parent = embed(c["do"].reshape(B * Sq, D).to(device), D + 8, 8, 4, 3, NAN)
        self.keep = None if c["keep"] is None else c["keep"].to(device).contiguous()
        self.bias = self.bias_parent = self.bias_t = self.bias_t_parent = None
        if c["bias"] is not None:
            ld = c["bias"].shape[2]
            self.bias, self.bias_parent = embed(c["bias"].reshape(H * Sq, ld).to(device), ld, 0, 4, 3, NAN)
            ldt = stat_ld(Sq)
            bt = torch.zeros((H, Sk, ldt))
            bt[:, :, :Sq] = c["bias"][:, :, :Sk].transpose(1, 2)
            self.bias_t, self.bias_t_parent = embed(bt.reshape(H * Sk, ldt).to(device), ldt, 0, 4, 3, NAN)
        self.kv_index = self.grp_start = self.grp_rows = None
        if sp.grouped:
            order = torch.sort(c["idx"].cpu(), stable=True).indices
            start = torch.zeros(U + 1, dtype=torch.int64)
            start[1:] = torch.cumsum(torch.bincount(c["idx"].cpu(), minlength=U), 0)
            self.grp_start, self.grp_rows = start.to(I32).to(device), order.to(I32).to(device)
        elif sp.idx is not None:
            self.kv_index = c["idx"].to(I32).to(device)
        self.outs, self.given = {}, {}

    def begin(self):
        """forget the outputs of the previous call"""
        self.outs, self.given = {}, {}

    # ---- outputs: views of 7.0-filled parents
    def out16(self, name, rows):
        v, p = embed(torch.full((rows, self.D), SENTINEL, dtype=BF16, device=self.dev), self.D + 8, 4, 4, 3, SENTINEL)
        self.outs[name] = (p, [v])
        return v

    def stat(self, name, given=None, nan_padding=False):
        """lse / delta [B*H, stat_ld]: the kernels own columns [0, Sq); given: an input's values (its parent is NaN)"""
        R, Sq, ld = self.sp.B * self.sp.H, self.sp.Sq, self.ld_stat
        fill = NAN if given is not None else SENTINEL
        t = torch.full((R, ld), fill, dtype=F32, device=self.dev)
        if given is not None:
            t[:, :Sq] = given
        elif nan_padding:
            t[:, Sq:] = NAN
        v, p = embed(t, ld, 0, 4, 3, fill)
        if given is None:
            self.outs[name] = (p, [v])
            self.outs[name + ":padding"] = (v[:, Sq:], nan_padding)
        else:      # an input: its whole parent -- values, NaN padding, NaN rows around -- must keep its bits
            self.given[name] = (p, p.clone())
        return v

    def dbias(self):
        ld = self.bias.shape[1]
        v, p = embed(torch.full((self.sp.H * self.sp.Sq, ld), DBIAS_INIT, dtype=F32, device=self.dev), ld, 0, 4, 3, SENTINEL)
        self.outs["dbias"] = (p, [v])
        return v

    def workspace(self, nbytes):
        assert nbytes % 4 == 0
        v, p = embed_vec(torch.full((nbytes // 4,), SENTINEL, dtype=F32, device=self.dev), 8, 8, SENTINEL)
        self.outs["dbias_ws"] = (p, [v])
        return v

    def check_outside(self):
        """every parent's outside, the statistics' padding, dbias's columns [Sk, ld) and the given statistics kept their bits"""
        for name, (p, before) in self.given.items():
            assert torch.equal(p.view(torch.int32), before.view(torch.int32)), f"{name}: the given statistics or their parent were written"
        for name, (p, views) in self.outs.items():
            if name.endswith(":padding"):
                pad, is_nan = p, views
                ok = _nan_bits(pad) if is_nan else torch.equal(pad, torch.full_like(pad, SENTINEL))
                assert ok, f"{name} was written"
            else:
                assert_outside_untouched(p, views[0], SENTINEL, name)
        if "dbias" in self.outs:
            pad = self.outs["dbias"][1][0][:, self.sp.Sk:]
            assert torch.equal(pad, torch.full_like(pad, DBIAS_INIT)), "dbias columns [Sk, ld) were written"


def ratio_line(sp, quantity, ratio):
    return f"attn-ratio gpu {sp.route} {shape_of(sp)} {sp.name} {quantity} {ratio:.3g}"


def max_norm_err(got, ref):
    """the measure of tests/test_hip_kernels.py: max |err| / max |ref|"""
    return float((got.double() - ref).abs().max() / ref.abs().max())
