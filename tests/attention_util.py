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
inside a sentinel parent.

Three later sections of this file extend the same machinery: "the bias path" (xfm_bias_tile, xfm_relpos_gather and the three table-gradient
forms: index restatements and the gradient bound), "the dense routes" (no mask, no dropout, no packing: the route restatement
dense_plan, dense_specs, the per-family counts and dense_fwd_ref / dense_bwd_ref) and "ragged rows" (q_start / q_len / k_start / k_len,
o_lo on masked problems: the layout, the per-entry reference, RaggedBuffers, ragged_specs); each has its own header."""
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
        if getattr(sp, "ld", 0):                                # a dense spec: its own row length, the padding never initialised
            c["bias"] = torch.full((H, Sq, sp.ld), NAN)
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


def bwd_ref(c, lse32, M=None, delta_given=None, nq=None):
    """lse32: the fp32 [B*H, Sq] statistics handed to the kernels.  -> (ref, b32) pairs: delta [B*H, Sq], dq [B*Sq, H*64], dk / dv
    [N*Sk, H*64] (N = B per query row for the general kernels, = U folded per source for the grouped ones), dbias [H*Sq, Sk] (with a bias).
    delta_given: (ref, b32) [B*H, Sq] where the kernel takes delta from the forward's output (delta_out_ref), dS is then formed from that
    delta as in dense_bwd_ref; nq: the additions of a dk / dv element where the caller knows better (the ragged section: a source's live
    query rows + 2)."""
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
    if delta_given is not None:
        delta, e_delta = (t.reshape(B, H, Sq) for t in delta_given)
    dmd = dP - delta.unsqueeze(-1)
    dS = P * dmd
    e_dS = e_P * dmd.abs() + P * (e_dP + e_delta.unsqueeze(-1)) + 2 * U32 * dS.abs()
    r16 = U16 * dS.abs() + e_dS
    dq = SCALE * (dS @ K)
    b_dq = SCALE * (r16 @ K.abs()) + (Sk + 2) * U32 * SCALE * (dS.abs() @ K.abs())
    W = P * F
    if nq is None:
        nq = Sq * int(torch.bincount(c["idx"], minlength=sp.U).max()) + 2 if sp.grouped else Sq + 2
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


# ---------------------------------------------------------------------------------------------------------------- the bias path
# What feeds the dense kernels their bias (csrc/attention_aux.hip): the relative-position table is gathered into a dense [H, N, ld] bias
# (xfm_relpos_gather), copied into the MFMA accumulator layout (xfm_bias_tile), and its gradient flows back into the table by one of three
# forms (xfm_relpos_scatter: float atomics; xfm_relpos_scatter_sorted: one workgroup per entry over pre-sorted positions;
# xfm_relpos_grid_grad: the structure of the standard grid index).  The two copies move values and are checked bit for bit against an
# index restatement; the gradients are sums:
#     dtable[e, h] = initial + sum over the n positions (i, j) with index[i, j] == e of ddense[h, i, j]
#     bound        = (n + 1) u32 (|initial| + sum |ddense|)            [n additions of the terms and one onto the initial value, in
#                                                                        whatever order: lanes, wave trees, atomics]
def bias_tile_index(S):
    """The accumulator layout of include/xfm_hip.h as indices: (q, k) int64 [T, T, 64, 4] of `tiled` (tile row a = query tile, column b =
    key tile: query 16a + lr, key 16b + 4lg + r, lane = 16 lg + lr) and (k_t, q_t) int64 [T + 1, T, 64, 4] of `tiled_t` (row a = key tile:
    key 16a + lr, query 16b + 4lg + r)."""
    T = (S + 15) // 16
    lane, r = torch.arange(64)[:, None], torch.arange(4)[None, :]
    on_lane, on_reg = lane % 16, 4 * (lane // 16) + r                                    # [64, 1], [64, 4]

    def grid(rows):
        a, b = torch.arange(rows)[:, None, None, None], torch.arange(T)[None, :, None, None]
        return (16 * a + on_lane).expand(rows, T, 64, 4), (16 * b + on_reg).expand(rows, T, 64, 4)

    q, k = grid(T)
    k_t, q_t = grid(T + 1)
    return q, k, k_t, q_t


def bias_tile_ref(bias, S, scale):
    """bias fp32 [H, S, ld] -> (tiled [H, T, T, 64, 4], tiled_t [H, T + 1, T, 64, 4]) fp32, the exact bits xfm_bias_tile must write:
    fl(bias fl(1 / scale)) with scale and its reciprocal in fp32, -1e30 where the key is past S, 0 where only the query is (the last
    key-tile row of tiled_t lies wholly past S).  Reads nothing of bias's columns [S, ld)."""
    inv = (torch.ones((), dtype=F32) / torch.tensor(scale, dtype=F32)).to(bias.device)
    scaled = bias[:, :, :S] * inv
    H = bias.shape[0]
    neg, zero = torch.full((), -1.0e30, dtype=F32, device=bias.device), torch.zeros((), dtype=F32, device=bias.device)

    def pick(q, k):
        q, k = q.to(bias.device), k.to(bias.device)
        val = scaled[:, q.clamp(max=S - 1), k.clamp(max=S - 1)]
        return torch.where((k >= S).expand((H,) + k.shape), neg, torch.where((q >= S).expand((H,) + q.shape), zero, val))

    q, k, k_t, q_t = bias_tile_index(S)
    return pick(q, k), pick(q_t, k_t)


def relpos_ref(table, index, H, N, ld):
    """(dense, dense_t) fp32 [H, N, ld]: dense[h, i, j] = table[index[i, j], h], dense_t[h, i, j] = dense[h, j, i], columns [N, ld) zero"""
    g = table[index.reshape(-1).long()].reshape(N, N, H).permute(2, 0, 1)
    dense = torch.zeros((H, N, ld), dtype=F32, device=table.device)
    dense_t = torch.zeros_like(dense)
    dense[:, :, :N], dense_t[:, :, :N] = g, g.transpose(1, 2)
    return dense, dense_t


def table_grad_ref(ddense, index, entries, initial):
    """ddense fp32 [H, N, >= N], index [N, N], initial fp32 [entries, H] -> (ref, b32) fp64 [entries, H] as the section's header says"""
    H, N = ddense.shape[0], index.shape[0]
    flat = index.reshape(-1).long().to(ddense.device)
    terms = ddense[:, :, :N].double().reshape(H, N * N).t()                              # [N N, H]
    z = torch.zeros((entries, H), dtype=F64, device=ddense.device)
    count = torch.bincount(flat, minlength=entries).double().unsqueeze(1)
    ref = initial.double() + z.clone().index_add_(0, flat, terms)
    return ref, (count + 1) * U32 * (initial.double().abs() + z.index_add_(0, flat, terms.abs()))


# ------------------------------------------------------------------------------------------------------------- the dense routes
# No mask, no dropout, no packing: attn_fwd_vit_kernel (attention_vit.hip), the PLAIN = true general kernels and DQ_SUMS
# (attention_general.hip), the short pair (attention_short.hip) and the three long kernels with dbias_reduce_kernel (attention_long.hip,
# attention.hip).  The reference is fwd_ref / bwd_ref's (no mask, p = 0, the backward from the GIVEN fp32 lse); what differs per family
# is where the roundings of a score fall.  With raw = scale q.k, mag = scale sum_d |q_d k_d|, b = the bias:
#     e_s = u32 (66 (mag + A_b |b| + A_l |lse|) + (1 - A_b) |b| + 2 L (|raw| + |b| + |lse|))
#   general    A_b = 0, A_l = 0, L = 0   fma(raw, scale, bias), __expf: the masked routes' count without the mask term
#   vit        A_b = 1, A_l = 0, L = 0   the forward starts the MFMA accumulator from fl(bias fl(1 / scale)): the 64 additions carry |b| too
#                                        (64 + that product + the fma = 66); p = exp2(fma(st, c2, fl(-max c2))), c2 = fl(scale log2 e): c2's
#                                        own error and the fma's rounding are relative to |s - max| (e_p's 1.5 |s - rowmax|), the rounding
#                                        of fl(-max c2) is common to the row and cancels in o; in lse it is u |max| <= u32 (|lse| + Sk)
#   short_dq   A_b = 1, A_l = 0, L = 1   the same accumulator; p = exp2(fma(st, c2, fl(-lse log2 e))): c2's error is relative to |raw| + |b|,
#                                        the lse product and its constant to |lse| -- four roundings of at most |raw| + |b| + |lse|: 2 u32
#   short_dkv  A_b = 1, A_l = 1, L = 0   the accumulator starts from fl(fma(-lse, 1 / scale, bias / scale)): the additions carry |b| + |lse|;
#                                        p = exp2(fl(st c2)), relative to |s - lse| (e_P's 1.5 |s - lse|)
#   long       A_b = 0, A_l = 0, L = 1   raw from a zero accumulator; nb = fma(bias, log2 e, fl(-lse log2 e)) (the bias-gradient kernel:
#                                        fl(bias log2 e) + fl(-lse log2 e)), p = exp2(fma(st, c2, nb)): the products with the constants,
#                                        the constants themselves and the sum, each of at most |raw| + |b| + |lse|.  The tiled copy
#                                        adds its own fl(bias fl(1 / scale)), within the same four.
# The rest is the masked routes' (P, o, lse, dP, delta, dS, dq, dk, dv: header), with these differences:
#     o, lse of the ViT forward     no online rescale: (Sk + 4) u32 in place of (Sk + 8 chunks) (the reciprocal, its product, log, the sum)
#     delta from the output         where the kernel takes delta = dO . (O + O_lo) (short PRE, long and general with o_lo) the reference is that
#                                   sum in fp64 from the bf16 O, O_lo it was given, b32 = C u32 sum_d |dO_d| (|O_d| + |Olo_d|), C = 66 for the
#                                   fma chain of delta_from_out (64 terms, o + o_lo, the merge), 130 for the short kernel's packed dot
#                                   products (128 products in fp32, the merges); dS is then formed from THAT delta
#     o + o_lo                      |o + o_lo - ref| <= b32 + u16^2 (|ref| + b32): o_lo = bf16(v - bf16(v)) of the fp32 v, |v - bf16 v| <= u16 |v|
#     dq, dk, dv                    dS (and P) cross LDS as bf16 in the short and long kernels as they enter the MFMA in the general ones:
#                                   the same u16 |dS| term; dq takes the dQ side's e_s, dk / dv the dK/dV side's
#     dbias                         sum_b e_dS + (B + F) u32 sum_b |dS| + F u32 |initial|: B additions of an entry's dS into the running sum
#                                   (registers, nb at a time; planes) and F additions onto dbias -- F = slices for the short kernel
#                                   (atomics or planes folded in order), ceil(B / nb) for DQ_SUMS, slices for the long kernels (1: in
#                                   place), B for the general kernel's atomics
# nb = 8 of DQ_SUMS needs ceil(blocks H ceil(B / 8) / 256) 8 <= the same with 4, i.e. more than 256 workgroups: not reachable at test
# shapes (B = 33 gives 4), and XFM_ATTN_DBIAS_NB is read once per process.
# The opt-in single pass (attn_bwd_vit3_kernel, XFM_ATTN_VIT_BWD = 3 / 4, 13-tile shapes, tiled bias): both sides are short_dkv's (the score
# accumulator starts from fl(bias / scale - lse / scale), p = exp2(fl(sc c2))); delta = dO . O with the bf16 O (the fma chain: C = 66, O_lo = 0
# in delta_out_ref); the dP accumulator starts from -delta, so its 64 additions carry |delta| too: e_dP += 66 u32 |delta|; the bias gradient
# stays in registers across the items of a head: F = ceil(B / c) + 1 flushes at most (c = items per workgroup).  Mode 4 leaves the bias
# gradient to attn_dbias_long_kernel on the delta the single pass wrote: the long family, F = its slices.
#
# Specs (H = 2 unless the case is about the heads).  Where the shapes first planned for a route and the code disagree the code wins:
#     walking workgroup    vit_map is head-major flat by default: c = ceil(B H / 256) items per workgroup, so B = 129, H = 2 (258 items) gives
#                          129 FULL workgroups; B = 87, H = 3 (261 items) gives 130 of two items and a last one of one, and workgroups
#                          that straddle two heads (87 is odd).  Forward only.
#     40 x 20              the short pair with Sk = 20: 2 key tiles, key-range waves 2 and 3 idle
#     70 x 130, ld = 136   below cdiv(Sk, 16) 16 = 144: attn_short_dq_ok fails -> DQ_SUMS + the general dK/dV
def cdiv(a, b):
    return -(-a // b)


RES_MAX = 4       # ATTN_RES_MAX
FAM = {"general": (0, 0, 0), "vit": (1, 0, 0), "short_dq": (1, 0, 1), "short_dkv": (1, 1, 0), "long": (0, 0, 1)}
C_DELTA_CHAIN, C_DELTA_DOT = 66, 130


def attn_geom(S, max_nw=8):
    tiles = cdiv(S, 16)
    blocks = cdiv(tiles, min(tiles, max_nw))
    return cdiv(tiles, blocks), blocks


def attn_resident(S, nw):
    return cdiv(S, 64) <= RES_MAX and nw >= 4


def attn_vit_shape(Sq, Sk, ld):
    return Sq == Sk and 64 < Sq <= 224 and (ld == 0 or (ld >= cdiv(Sk, 16) * 16 and ld % 4 == 0))


def attn_vit3_shape(Sq, Sk, ld, mode, o_lo, tiled):
    return mode != 0 and attn_vit_shape(Sq, Sk, ld) and cdiv(Sq, 16) == 13 and not o_lo and (ld == 0 or tiled)


def attn_long_shape(Sq, Sk, ld, ldt, dbias):
    return (Sk > 64 * RES_MAX and (ld == 0 or (ld % 4 == 0 and ld >= cdiv(Sk, 4) * 4)) and (ldt == 0 or (ldt % 4 == 0 and ldt >= cdiv(Sq, 4) * 4))
            and (not dbias or (ld > 0 and ld <= cdiv(Sk, 128) * 128)))


def attn_long_dkv_ok(ld, bias_t, tiled_square):
    return ld == 0 or bias_t or tiled_square


def attn_short_dq_ok(Sk, ld, dbias):
    return Sk <= 64 * RES_MAX and (ld == 0 or ld >= cdiv(Sk, 16) * 16) and (not dbias or ld >= Sk)


def attn_short_nb(B, H, rows, KT):
    """-> (batch entries per slice, groups)"""
    groups = cdiv(cdiv(rows, 16), KT)
    z = max(1, min(B, 256 // (groups * H)))
    return cdiv(B, z), groups


def attn_short_dq_slices(B, H, Sq):
    """-> (slices, groups, nb)"""
    nb, groups = attn_short_nb(B, H, Sq, 3)
    return cdiv(B, nb), groups, nb


def attn_short_dq_np(Sk):
    return 4 if Sk <= 128 else 7 if Sk <= 224 else 8


def attn_short_planes_ok(Sk, ld):
    return ld <= cdiv(Sk, 16) * 16


def attn_dbias_sums_nb(B, H, blocks):
    nb = 2 if B >= 8 else 1
    if B >= 32:
        c4, c8 = cdiv(blocks * H * cdiv(B, 4), 256) * 4, cdiv(blocks * H * cdiv(B, 8), 256) * 8
        nb = 8 if c8 <= c4 else 4
    return nb


def dbias_long_slices(blocks, B, plane_bytes):
    best, best_cost = 1, -1.0
    for s in range(1, min(16, B) + 1):
        cost = float(cdiv(blocks * s, 256)) * (2.0 * cdiv(B, s) + 3.0) + (s * float(plane_bytes) * 2.0 / 4.0e6 if s > 1 else 0.0)
        if best_cost < 0 or cost < best_cost - 1e-9:
            best, best_cost = s, cost
    return best


def attn_dbias_blocks_slices(B, H, Sq, Sk, ld):
    return dbias_long_slices(cdiv(Sq, 128) * cdiv(Sk, 128) * H, B, H * Sq * ld * 4)


def vit_map(B, H):
    """the default (head-major flat) map -> (items per workgroup, workgroups, items of the last workgroup)"""
    c = cdiv(B * H, 256)
    grid = cdiv(B * H, c)
    return c, grid, B * H - (grid - 1) * c


Route = namedtuple("Route", "fwd dq dkv dbias nb slices planes")


def dense_plan(sp, bias_t=True, tiled=False, o_lo=False, have_ws=True, vit_mode=0, pre=False, det=False):
    """attn_bwd_plan (csrc/attention.hip) and the forward's choice (xfm_attn_fwd_impl) restated for a dense problem: which kernels a call
    runs.  nb / slices: batch entries per workgroup and workgroup slices of the bias-gradient sum (0 where the route has none);
    planes: what xfm_attn_bwd_workspace reports, in [H, Sq, bias_ld] fp32 planes."""
    B, H, Sq, Sk, ld = sp.B, sp.H, sp.Sq, sp.Sk, sp.ld
    has_bias = dbias = ld > 0
    ldt = stat_ld(Sq) if has_bias and bias_t else 0
    tiled = tiled and has_bias and Sq == Sk
    if Sq <= 64 and Sk <= 64 and not has_bias and B >= 2:
        fwd = "packed"
    elif attn_vit_shape(Sq, Sk, ld):
        fwd = "vit13" if cdiv(Sq, 16) == 13 else "vit_rt"
    else:
        fwd = "plain_res" if attn_resident(Sk, attn_geom(Sq)[0]) else "plain_stream"
    ws_ok = have_ws and dbias and ld % 4 == 0 and ld <= cdiv(Sk, 64) * 64
    dq = dkv = dbias_form = None
    nb = slices = planes = 0
    if attn_vit3_shape(Sq, Sk, ld, vit_mode, o_lo, tiled):
        dq, dkv = "vit3", "vit3"
        if dbias:
            dbias_form = "blocks" if vit_mode == 4 and ld <= cdiv(Sk, 128) * 128 else "atomics"
            # the single pass keeps sum_b dS in registers across the items of one head and flushes when the head changes: with c items a
            # workgroup (head-major) a head's B entries lie in at most ceil(B / c) + 1 workgroups
            nb = vit_map(B, H)[0]
            slices = cdiv(B, nb) + 1
    elif attn_long_shape(Sq, Sk, ld, ldt, dbias):
        dq = "long"
        dkv = "long" if attn_long_dkv_ok(ld, ldt > 0, tiled) else "general"
        if dbias:
            dbias_form = "blocks"
    else:
        short_ok = attn_short_dq_ok(Sk, ld, dbias)
        nw, blocks = attn_geom(Sq)
        if short_ok:
            dq = "short_pre" if pre and o_lo else "short"
            slices, _, nb = attn_short_dq_slices(B, H, Sq)
            if dbias:
                dbias_form = "short_planes" if ws_ok and attn_short_planes_ok(Sk, ld) and slices > 1 and det else "atomics"
            if dbias_form == "short_planes":
                planes = slices
        elif dbias and attn_resident(Sk, nw):
            dq, dbias_form = "sums", "sums"
            nb = attn_dbias_sums_nb(B, H, blocks)
            slices = cdiv(B, nb)
        else:
            dq = "general"
            nb, slices = 1, B
            if dbias:
                dbias_form = "entry_ws" if ws_ok and Sk > 64 * RES_MAX else "atomics"
            if dbias_form == "entry_ws":
                planes = B
        dkv = "short" if short_ok and Sq <= 224 else "general"
    if dbias_form == "blocks":
        slices = attn_dbias_blocks_slices(B, H, Sq, Sk, ld) if ws_ok else 1
        nb = cdiv(B, slices)
        planes = slices if slices > 1 else 0
    if not dbias:
        nb = slices = 0
    return Route(fwd, dq, dkv, dbias_form, nb, slices, planes)


# ld: bias row length (0: no bias); bwd: the backward runs too; want: the Route of the default call (transposed bias copy and a workspace
# offered, no tiled copies, no o_lo, every knob at its default)
DenseSpec = namedtuple("DenseSpec", "route B H Sq Sk U idx grouped mask causal p score bias name ld bwd want")


def _dense(group, B, H, Sq, Sk, ld, want, score="randn", bwd=True):
    name = (f"ld{ld}" if ld else "nobias") + ("" if score == "randn" else "+" + score)
    return DenseSpec(group, B, H, Sq, Sk, B, None, False, None, False, 0.0, score, ld > 0, name, ld, bwd, Route(*want))


def dense_specs():
    S, A, G, L = "short", "atomics", "general", "long"
    return [
        # 1. the ViT forward with run-time tiles (backward: the short pair)
        _dense("vit_rt", 2, 2, 65, 65, 0, ("vit_rt", S, S, None, 0, 0, 0)),
        _dense("vit_rt", 2, 2, 65, 65, 80, ("vit_rt", S, S, A, 1, 2, 0)),
        _dense("vit_rt", 2, 2, 130, 130, 144, ("vit_rt", S, S, A, 1, 2, 0)),
        _dense("vit_rt", 2, 2, 224, 224, 224, ("vit_rt", S, S, A, 1, 2, 0)),
        # 2. the 13-tile form
        _dense("vit13", 2, 2, 197, 197, 0, ("vit13", S, S, None, 0, 0, 0)),
        _dense("vit13", 2, 2, 197, 197, 208, ("vit13", S, S, A, 1, 2, 0)),
        _dense("vit13", 2, 2, 197, 197, 208, ("vit13", S, S, A, 1, 2, 0), score="steep"),
        _dense("vit13", 2, 2, 208, 208, 208, ("vit13", S, S, A, 1, 2, 0)),
        # 3. walking workgroups: 261 items, two per workgroup, the last workgroup one; the second K / V image
        _dense("vit_walk", 87, 3, 70, 70, 80, ("vit_rt", S, S, A, 3, 29, 0), bwd=False),
        _dense("vit_walk", 87, 3, 197, 197, 208, ("vit13", S, S, A, 6, 15, 0), bwd=False),
        # 4. the general plain forward
        _dense("plain", 1, 2, 30, 197, 0, ("plain_stream", S, S, None, 0, 0, 0)),
        _dense("plain", 2, 2, 30, 197, 0, ("plain_stream", S, S, None, 0, 0, 0)),
        _dense("plain", 2, 2, 16, 16, 16, ("plain_stream", S, S, A, 1, 2, 0)),
        _dense("plain", 2, 2, 40, 300, 0, ("plain_stream", L, L, None, 0, 0, 0), score="steep"),
        _dense("plain", 2, 2, 130, 321, 0, ("plain_stream", L, L, None, 0, 0, 0)),
        _dense("plain", 2, 2, 70, 130, 0, ("plain_res", S, S, None, 0, 0, 0)),
        # 5. the short pair: Sk = 20 (two key-range waves idle), NP = 4 / 7 / 8, the longest query side of the short dK/dV, short dQ + general dK/dV
        _dense("short", 2, 2, 40, 20, 32, ("plain_stream", S, S, A, 1, 2, 0)),
        _dense("short", 2, 2, 100, 128, 128, ("plain_res", S, S, A, 1, 2, 0)),
        _dense("short", 2, 2, 100, 256, 260, ("plain_res", S, S, A, 1, 2, 0)),
        _dense("short", 2, 2, 250, 250, 256, ("plain_res", S, G, A, 1, 2, 0)),
        _dense("short", 2, 2, 300, 256, 0, ("plain_res", S, G, None, 0, 0, 0)),
        # 6. several entries per workgroup, a ragged last slice
        _dense("short_nb", 11, 4, 250, 250, 256, ("plain_res", S, G, A, 2, 6, 0)),
        # 7. more than one slice; with XFM_DETERMINISTIC=1 one plane per slice
        _dense("short_slices", 9, 2, 40, 40, 48, ("plain_stream", S, S, A, 1, 9, 0)),
        # 8. DQ_SUMS: nb = 1, 2 (ragged), 4 (ragged)
        _dense("sums", 3, 2, 70, 130, 136, ("plain_res", "sums", G, "sums", 1, 3, 0)),
        _dense("sums", 9, 2, 70, 130, 136, ("plain_res", "sums", G, "sums", 2, 5, 0)),
        _dense("sums", 33, 2, 70, 130, 136, ("plain_res", "sums", G, "sums", 4, 9, 0)),
        # 9. the long kernels (B = 2: the cost model of dbias_long_slices already takes two one-entry slices; 577 tokens take one, in place)
        _dense("long", 2, 2, 40, 300, 304, ("plain_stream", L, L, "blocks", 1, 2, 2)),
        _dense("long", 2, 2, 260, 260, 264, ("plain_stream", L, L, "blocks", 1, 2, 2)),
        _dense("long", 2, 2, 300, 700, 704, ("plain_stream", L, L, "blocks", 1, 2, 2)),
        _dense("long", 2, 2, 700, 300, 304, ("plain_stream", L, L, "blocks", 1, 2, 2)),
        # 10. / 11. single-entry and two-entry slices of the bias-gradient kernel; 12. 577 tokens
        _dense("long_slices", 3, 2, 260, 260, 264, ("plain_stream", L, L, "blocks", 1, 3, 3)),
        _dense("long_slices", 17, 1, 260, 260, 264, ("plain_stream", L, L, "blocks", 2, 9, 9)),
        _dense("long", 2, 2, 577, 577, 580, ("plain_stream", L, L, "blocks", 2, 1, 0)),
    ]


def dense_families(rt):
    """(forward family, dQ-side family, dK/dV-side family) of a Route"""
    side = {"short": "short_dq", "short_pre": "short_dq", "long": "long", "sums": "general", "general": "general", "vit3": "short_dkv"}
    return ("vit" if rt.fwd.startswith("vit") else "general", side[rt.dq],
            {"short": "short_dkv", "long": "long", "general": "general", "vit3": "short_dkv"}[rt.dkv])


def dense_flushes(sp, rt):
    """F of the dbias bound: additions onto dbias"""
    return {"atomics": sp.B if rt.dq == "general" else rt.slices, "short_planes": rt.slices, "sums": rt.slices, "blocks": rt.slices,
            "entry_ws": sp.B, None: 0}[rt.dbias]


def dense_scores(c, fam, lse=None):
    """(s, e_s) fp64 [B, H, Sq, Sk] for a dense case; lse fp64 [B, H, Sq] where the family's scores carry it"""
    a_b, a_l, l2 = FAM[fam]
    sp = c["sp"]
    Q, K = _heads(c["q"]), _heads(c["k"])
    raw = SCALE * (Q @ K.transpose(-1, -2))
    mag = SCALE * (Q.abs() @ K.abs().transpose(-1, -2))
    b = 0.0 * raw if c["bias"] is None else (c["bias"][:, :, :sp.Sk].double().unsqueeze(0) + 0.0 * raw)
    lm = 0.0 if lse is None else lse.abs().unsqueeze(-1)
    assert lse is not None or (a_l == 0 and l2 == 0)
    e = C_K * (mag + a_b * b.abs() + a_l * lm) + (1 - a_b) * b.abs() + 2 * l2 * (raw.abs() + b.abs() + lm)
    return raw + b, U32 * e


def dense_fwd_ref(c, fam):
    """-> {"o": (ref [B*Sq, H*64], b32), "lse": (ref [B*H, Sq], b32)}"""
    sp = c["sp"]
    s, e_s = dense_scores(c, fam)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.unsqueeze(-1))
    e_p = e_s + U32 * (1.5 * (s - s.max(-1, keepdim=True).values).abs() + E_EXP)
    V = _heads(c["v"])
    o, mag = P @ V, P @ V.abs()
    nsum = sp.Sk + (4 if fam == "vit" else 8 * chunks(sp.Sk))
    lerr = (P * e_p).sum(-1)
    b_o = (P * (U16 + e_p)) @ V.abs() + (o.abs() + mag) * (lerr + nsum * U32).unsqueeze(-1)
    b_lse = lerr + U32 * (lse.abs() + nsum)
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(sp.B * sp.Sq, sp.H * 64)   # noqa: E731
    return {"o": (rows(o), rows(b_o)), "lse": (lse.reshape(sp.B * sp.H, sp.Sq), b_lse.reshape(sp.B * sp.H, sp.Sq))}


def check_o_lo(o, o_lo, ref, b32, what="o + o_lo"):
    """o + o_lo against the fp64 o: the fp32 evaluation plus one bf16 rounding of the residual; returns the worst ratio"""
    from gemm_strided_util import _check
    return _check(o.double() + o_lo.double(), ref, b32 + U16 * U16 * (ref.abs() + b32), what)


def delta_out_ref(c, o16, o_lo16, count):
    """delta = dO . (O + O_lo) from the bf16 halves [B*Sq, H*64] the kernel is given -> (ref, b32) fp64 [B*H, Sq]"""
    sp = c["sp"]
    DO = c["do"].double().reshape(sp.B, sp.Sq, sp.H, 64)
    O, L = (t.double().reshape(sp.B, sp.Sq, sp.H, 64) for t in (o16, o_lo16))
    ref = (DO * (O + L)).sum(-1).permute(0, 2, 1)
    mag = (DO.abs() * (O.abs() + L.abs())).sum(-1).permute(0, 2, 1)
    return ref.reshape(sp.B * sp.H, sp.Sq), (count * U32 * mag).reshape(sp.B * sp.H, sp.Sq)


def dense_bwd_ref(c, lse32, fam_q, fam_k, flushes, delta_given=None, fam_b=None, delta_in_acc=False):
    """bwd_ref for a dense case whose dQ side (delta, dq, dbias) and dK/dV side (dk, dv) belong to the families fam_q / fam_k; flushes: F of
    the header; delta_given: (ref, b32) [B*H, Sq] where the kernel takes delta from the forward's output; fam_b: the family of the kernel
    that forms the bias gradient where that is not the dQ kernel; delta_in_acc: the dP accumulator starts from -delta (the single pass)."""
    sp = c["sp"]
    B, H, Sq, Sk = sp.B, sp.H, sp.Sq, sp.Sk
    lse = lse32.double().reshape(B, H, Sq)
    (s, e_sq), (_, e_sk) = dense_scores(c, fam_q, lse), dense_scores(c, fam_k, lse)
    d = s - lse.unsqueeze(-1)
    P = torch.exp(d)
    e_Pq, e_Pk = (P * (e + U32 * (1.5 * d.abs() + E_EXP)) for e in (e_sq, e_sk))
    Q, K, V, DO = _heads(c["q"]), _heads(c["k"]), _heads(c["v"]), _heads(c["do"])
    dP = DO @ V.transpose(-1, -2)
    e_dP = C_K * U32 * (DO.abs() @ V.abs().transpose(-1, -2))
    if delta_given is None:
        PdP = P * dP
        delta = PdP.sum(-1)
        e_delta = (e_Pq * dP.abs() + P * e_dP).sum(-1) + Sk * U32 * PdP.abs().sum(-1)
    else:
        delta, e_delta = (t.reshape(B, H, Sq) for t in delta_given)
    dmd = dP - delta.unsqueeze(-1)
    dS = P * dmd
    if delta_in_acc:      # the 64 additions of dP carry |delta| as well
        e_dP = e_dP + C_K * U32 * delta.abs().unsqueeze(-1)
    e_dSq, e_dSk = (e * dmd.abs() + P * (e_dP + e_delta.unsqueeze(-1)) + 2 * U32 * dS.abs() for e in (e_Pq, e_Pk))
    r16q, r16k = U16 * dS.abs() + e_dSq, U16 * dS.abs() + e_dSk
    dq = SCALE * (dS @ K)
    b_dq = SCALE * (r16q @ K.abs()) + (Sk + 2) * U32 * SCALE * (dS.abs() @ K.abs())
    dk = SCALE * (dS.transpose(-1, -2) @ Q)
    b_dk = SCALE * (r16k.transpose(-1, -2) @ Q.abs()) + (Sq + 2) * U32 * SCALE * (dS.abs().transpose(-1, -2) @ Q.abs())
    dv = P.transpose(-1, -2) @ DO
    b_dv = (U16 * P + e_Pk).transpose(-1, -2) @ DO.abs() + (Sq + 2) * U32 * (P.transpose(-1, -2) @ DO.abs())
    rows = lambda t, S: t.permute(0, 2, 1, 3).reshape(B * S, H * 64)   # noqa: E731
    out = {"delta": (delta.reshape(B * H, Sq), e_delta.reshape(B * H, Sq)), "dq": (rows(dq, Sq), rows(b_dq, Sq)),
           "dk": (rows(dk, Sk), rows(b_dk, Sk)), "dv": (rows(dv, Sk), rows(b_dv, Sk))}
    if c["bias"] is not None:
        ref = DBIAS_INIT + dS.sum(0)
        e_dSb = e_dSq
        if fam_b is not None:
            e_Pb = P * (dense_scores(c, fam_b, lse)[1] + U32 * (1.5 * d.abs() + E_EXP))
            e_dSb = e_Pb * dmd.abs() + P * (e_dP + e_delta.unsqueeze(-1)) + 2 * U32 * dS.abs()
        b = e_dSb.sum(0) + (B + flushes) * U32 * dS.abs().sum(0) + flushes * U32 * DBIAS_INIT
        out["dbias"] = (ref.reshape(H * Sq, Sk), b.reshape(H * Sq, Sk))
    return out


# ------------------------------------------------------------------------------------------------------------------ ragged rows
# Unpadded token rows (q_start / q_len / k_start / k_len of xfm_attn_args), the way xfm_rlayer_fwd / bwd call the kernels
# (csrc/encoder.hip): self-attention with both pairs (q_start == k_start), range-mode cross-attention with the query pair and dense
# keys (B = sources), grouped cross-attention with the query pair; and o_lo on masked / dropped / grouped problems, ragged or not.
# Ragged rows never leave the general kernels (attention_general.hip; the packed forward xattn_fwd_kernel<true, ...> up to 64 x 64 with
# B >= 2) and the grouped ones: attn_vit_shape, attn_long_shape and attn_short_dq_ok all require q_start == k_start == NULL.
#
# Reference.  The semantics are EXCLUSION: entry b is fwd_ref / bwd_ref on the sliced operands, queries [0, q_len[b]), keys [0, k_len[b])
# of its source (entry_case), so every Sk and Sq of the header's counts -- (Sk + 8 chunks), Sk + 2, Sq + 2 -- is the entry's own length,
# key_keep and the causal mask apply on local indices, and the dropout mask is the [:q_len, :k_len] corner of the padded [B, H, Sq, Sk]
# array (the counters stay laid out for the padded Sq: drop_key in attention_common.h).  A key past k_len gets EXCL_NEG = -1e30 in
# score_masked, exp(-1e30 - m) is exactly 0: no rounding to count, and no -10000 -- a row whose live keys are all masked is a softmax over
# its LIVE keys alone.  Grouped dk / dv are the sum over the source's entries of the entries' own references; a source's element is the sum
# of sum(q_len of its entries) products, so the addition count of every entry's term is that sum + 2 (bwd_ref's nq), for a bound of
# (sum q_len + 2) u32 sum |terms| on the whole.  No constant is new.
# delta from the output (o_lo given): attn_bwd_dq_kernel, xattn_dq_kernel and xattn_dq_stream_kernel all call delta_from_out
# (attention_common.h), the fma chain counted at C_DELTA_CHAIN = 66 in the dense section; the reference is delta_out_ref on the entry's
# rows of the bf16 o / o_lo the kernel was given, and dS, dq, dk, dv are formed from THAT delta (bwd_ref's delta_given).  Without o_lo
# delta stays sum_j P dP of the dropped dP.
# Statistics.  attn_fwd_kernel (`if (!wave_active || qi >= sq) return`), xattn_fwd_kernel (`if (qi < sq)`), xattn_fwd_stream_kernel
# (`ok && qi < sq`) store lse only for qi < q_len[b], the three dQ kernels store delta under `qvalid`: columns [q_len[b], stat_ld) of
# entry b's rows of lse / delta keep their bits on every route.  The dK/dV kernels LOAD them (16-byte loads up to the padded Sq) and
# select them away, so the given lse and the delta buffer hold NaN there before the backward.
#
# Layout (ragged_layout, "shuffled"): entry b's live rows sit at start[b] of the row buffer; entries are stored in the order 1, 0, 2,
# 3, ... (starts not monotone in b) with two slack rows in front and 1 + b % 3 behind each; in self-attention q, k, v are column slices of
# one parent and q_start == k_start, an entry taking max(q_len, k_len) rows.  Slack rows of the inputs are NaN; slack rows of o, o_lo, dq,
# dk, dv are the sentinel inside the sentinel parents and must keep their bits (RaggedBuffers.check_outside).  A dense side is b * S rows.
RaggedSpec = namedtuple("RaggedSpec", Spec._fields + ("q_len", "k_len", "layout"))
Layout = namedtuple("Layout", "q_start q_len q_rows k_start k_len k_rows")


def _place(lens):
    order = ([1, 0] + list(range(2, len(lens)))) if len(lens) > 1 else [0]
    start, row = [0] * len(lens), 2
    for b in order:
        start[b] = row
        row += lens[b] + 1 + b % 3
    return tuple(start), row


def ragged_layout(sp):
    """Where the rows of every entry sit: (q_start, q_len, q_rows, k_start, k_len, k_rows); the key side has U entries.  dk / dv rows
    follow the key side (per query entry in self-attention and range mode, where U == B; per source when grouped)."""
    dense_q = (tuple(b * sp.Sq for b in range(sp.B)), (sp.Sq,) * sp.B, sp.B * sp.Sq)
    dense_k = (tuple(u * sp.Sk for u in range(sp.U)), (sp.Sk,) * sp.U, sp.U * sp.Sk)
    if sp.q_len is None:
        assert sp.k_len is None
        return Layout(*dense_q, *dense_k)
    assert sp.layout == "shuffled" and len(sp.q_len) == sp.B and all(1 <= n <= sp.Sq for n in sp.q_len)
    if sp.k_len is None:
        start, rows = _place(sp.q_len)
        return Layout(start, tuple(sp.q_len), rows, *dense_k)
    assert sp.U == sp.B and sp.idx is None and len(sp.k_len) == sp.B and all(1 <= n <= sp.Sk for n in sp.k_len)
    start, rows = _place([max(a, b) for a, b in zip(sp.q_len, sp.k_len)])
    return Layout(start, tuple(sp.q_len), rows, start, tuple(sp.k_len), rows)


def ragged_live(sp, device="cpu"):
    """bool masks of what the kernels own: "q" [q_rows], "k" [k_rows] (rows of a sequence), "stat" [B*H, Sq] (columns below q_len[b])"""
    lay = ragged_layout(sp)
    q, k = torch.zeros(lay.q_rows, dtype=torch.bool), torch.zeros(lay.k_rows, dtype=torch.bool)
    for s, n in zip(lay.q_start, lay.q_len):
        q[s:s + n] = True
    for s, n in zip(lay.k_start, lay.k_len):
        k[s:s + n] = True
    stat = (torch.arange(sp.Sq)[None, :] < torch.tensor(lay.q_len)[:, None]).repeat_interleave(sp.H, 0)
    return {"q": q.to(device), "k": k.to(device), "stat": stat.to(device)}


def make_ragged_case(sp):
    """make_case on the padded shape (so a ragged case and its padded twin share every operand); steep: the planted key 8 e also at every
    source's last kept LIVE key, so the running maximum of a shorter entry ends in ITS last chunk too."""
    c = make_case(sp)
    if sp.score == "steep" and sp.k_len is not None:
        for u, n in enumerate(sp.k_len):
            kept = torch.ones(n, dtype=torch.bool) if c["keep"] is None else c["keep"][u, :n] != 0
            if bool(kept.any()):      # (holes mask key 0 of the even sources: an entry of one key has no kept key, and nothing planted)
                c["k"][u, int(kept.nonzero().max())] = 1.0
    return c


def entry_case(c, b, M=None, q_len=None, k_len=None):
    """(case, mask) of entry b alone on its sliced operands: B = U = 1, Sq = q_len[b], Sk = k_len of its source (q_len / k_len: other
    lengths, for a planted fault)"""
    sp = c["sp"]
    lay = ragged_layout(sp)
    src = int(c["idx"][b])
    ql = lay.q_len[b] if q_len is None else q_len
    kl = lay.k_len[src] if k_len is None else k_len
    spb = Spec(sp.route, 1, sp.H, ql, kl, 1, None, sp.grouped, sp.mask, sp.causal, sp.p, sp.score, False, sp.name)
    cb = {"sp": spb, "q": c["q"][b:b + 1, :ql], "do": c["do"][b:b + 1, :ql], "k": c["k"][src:src + 1, :kl], "v": c["v"][src:src + 1, :kl],
          "bias": None, "keep": None if c["keep"] is None else c["keep"][src:src + 1, :kl],
          "idx": torch.zeros(1, dtype=torch.int64, device=c["q"].device)}
    return cb, (None if M is None else M[b:b + 1, :, :ql, :kl])


def _stat_rows(t, sp, b, ql):
    """entry b's [H, ql] corner of a [B*H, Sq] statistic"""
    return t.reshape(sp.B, sp.H, sp.Sq)[b, :, :ql]


def ragged_fwd_ref(c, M=None):
    """-> {"o": (ref, b32) [q_rows, H*64] in the buffer's row layout, "lse": (ref, b32) [B*H, Sq]}; compare where ragged_live says so
    (slack rows and dead columns hold 0 here)"""
    sp = c["sp"]
    lay = ragged_layout(sp)
    dev = c["q"].device
    o = [torch.zeros((lay.q_rows, sp.H * 64), dtype=F64, device=dev) for _ in range(2)]
    lse = [torch.zeros((sp.B * sp.H, sp.Sq), dtype=F64, device=dev) for _ in range(2)]
    for b in range(sp.B):
        cb, Mb = entry_case(c, b, M)
        fr = fwd_ref(cb, Mb)
        s, n = lay.q_start[b], lay.q_len[b]
        for i in range(2):
            o[i][s:s + n] = fr["o"][i]
            _stat_rows(lse[i], sp, b, n).copy_(fr["lse"][i])
    return {"o": tuple(o), "lse": tuple(lse)}


def ragged_lse32(fr, sp):
    """the statistics handed to the backward: fp32 of the reference's lse, NaN in the dead columns"""
    return torch.where(ragged_live(sp, fr["lse"][0].device)["stat"], fr["lse"][0].float(), torch.full((), NAN, device=fr["lse"][0].device))


def ragged_bwd_ref(c, lse32, M=None, o16=None, o_lo16=None):
    """-> (ref, b32) pairs: delta [B*H, Sq], dq [q_rows, H*64], dk / dv [k_rows, H*64] in the buffers' row layouts (grouped: summed per
    source).  o16, o_lo16 [q_rows, H*64]: the bf16 halves the kernel is given; delta is then delta_out_ref's (C_DELTA_CHAIN)."""
    sp = c["sp"]
    lay = ragged_layout(sp)
    dev = c["q"].device
    D = sp.H * 64
    out = {"delta": [torch.zeros((sp.B * sp.H, sp.Sq), dtype=F64, device=dev) for _ in range(2)],
           "dq": [torch.zeros((lay.q_rows, D), dtype=F64, device=dev) for _ in range(2)],
           "dk": [torch.zeros((lay.k_rows, D), dtype=F64, device=dev) for _ in range(2)],
           "dv": [torch.zeros((lay.k_rows, D), dtype=F64, device=dev) for _ in range(2)]}
    for b in range(sp.B):
        cb, Mb = entry_case(c, b, M)
        src = int(c["idx"][b])
        s, n = lay.q_start[b], lay.q_len[b]
        given = None if o16 is None else delta_out_ref(cb, o16[s:s + n], o_lo16[s:s + n], C_DELTA_CHAIN)
        nq = 2 + sum(lay.q_len[i] for i in range(sp.B) if int(c["idx"][i]) == src) if sp.grouped else None
        br = bwd_ref(cb, _stat_rows(lse32, sp, b, n).reshape(sp.H, n), Mb, delta_given=given, nq=nq)
        ks, kn = lay.k_start[src], lay.k_len[src]
        for i in range(2):
            _stat_rows(out["delta"][i], sp, b, n).copy_(br["delta"][i].reshape(sp.H, n))
            out["dq"][i][s:s + n] = br["dq"][i]
            out["dk"][i][ks:ks + kn] += br["dk"][i]      # (one entry per source unless grouped)
            out["dv"][i][ks:ks + kn] += br["dv"][i]
    return {k: tuple(v) for k, v in out.items()}


class RaggedBuffers(AttnBuffers):
    """AttnBuffers for a RaggedSpec: the live rows of every entry at the layout's starts, NaN in the inputs' slack rows, the sentinel in
    the outputs'; q_start / q_len / k_start / k_len as int32 device vectors (None for a dense side)."""

    def __init__(self, c, device):
        sp = c["sp"]
        self.sp, self.dev = sp, device
        lay = self.lay = ragged_layout(sp)
        self.live = ragged_live(sp, device)
        D = sp.H * 64
        self.D, self.ld_stat = D, stat_ld(sp.Sq)
        self.qkv = torch.full((max(lay.q_rows, lay.k_rows) + 7, 3 * D + 8), NAN, dtype=BF16, device=device)
        self.q = self.qkv[4:4 + lay.q_rows, 8:8 + D]
        self.k = self.qkv[4:4 + lay.k_rows, 8 + D:8 + 2 * D]
        self.v = self.qkv[4:4 + lay.k_rows, 8 + 2 * D:8 + 3 * D]
        self.do, self.do_parent = embed(torch.full((lay.q_rows, D), NAN, dtype=BF16, device=device), D + 8, 8, 4, 3, NAN)
        for b, (s, n) in enumerate(zip(lay.q_start, lay.q_len)):
            self.q[s:s + n] = c["q"][b, :n].reshape(n, D).to(device)
            self.do[s:s + n] = c["do"][b, :n].reshape(n, D).to(device)
        for u, (s, n) in enumerate(zip(lay.k_start, lay.k_len)):
            self.k[s:s + n] = c["k"][u, :n].reshape(n, D).to(device)
            self.v[s:s + n] = c["v"][u, :n].reshape(n, D).to(device)
        self.keep = None if c["keep"] is None else c["keep"].to(device).contiguous()
        self.bias = self.bias_parent = self.bias_t = self.bias_t_parent = None
        self.kv_index = self.grp_start = self.grp_rows = None
        if sp.grouped:
            order = torch.sort(c["idx"].cpu(), stable=True).indices
            start = torch.zeros(sp.U + 1, dtype=torch.int64)
            start[1:] = torch.cumsum(torch.bincount(c["idx"].cpu(), minlength=sp.U), 0)
            self.grp_start, self.grp_rows = start.to(I32).to(device), order.to(I32).to(device)
        vec = lambda t: torch.tensor(t, dtype=I32, device=device)   # noqa: E731
        self.q_start = self.q_len = self.k_start = self.k_len = None
        if sp.q_len is not None:
            self.q_start, self.q_len = vec(lay.q_start), vec(lay.q_len)
        if sp.k_len is not None:
            self.k_start, self.k_len = vec(lay.k_start), vec(lay.k_len)
        self.begin()

    def begin(self):
        self.outs, self.given, self.sides, self.dead = {}, {}, {}, {}

    def rows_out(self, name, side):
        """a sentinel-filled bf16 output over the whole row buffer of the query ("q") or key ("k") side"""
        self.sides[name] = side
        return self.out16(name, self.lay.q_rows if side == "q" else self.lay.k_rows)

    def stat(self, name, given=None, nan_padding=False):
        """as AttnBuffers.stat; the kernels own columns [0, q_len[b]) only: the dead columns [q_len[b], Sq) hold what the padding holds
        (given: the caller's values, NaN there by ragged_lse32)"""
        v = AttnBuffers.stat(self, name, given, nan_padding)
        if given is None:
            if nan_padding:
                v[:, :self.sp.Sq].masked_fill_(~self.live["stat"], NAN)
            self.dead[name] = (v, nan_padding)
        return v

    def check_outside(self):
        """AttnBuffers.check_outside, the statistics' dead columns and the slack rows of every row output kept their bits"""
        AttnBuffers.check_outside(self)
        for name, (v, is_nan) in self.dead.items():
            dead = v[:, :self.sp.Sq][~self.live["stat"]]
            ok = _nan_bits(dead) if is_nan else torch.equal(dead, torch.full_like(dead, SENTINEL))
            assert ok, f"{name}: columns [q_len, Sq) were written"
        for name, side in self.sides.items():
            slack = self.outs[name][1][0][~self.live[side]]
            assert torch.equal(slack, torch.full_like(slack, SENTINEL)), f"{name}: rows outside every sequence were written"


RAGGED_VARIANTS = {"none": {}, "holes": {"mask": "holes"}, "holes+p0.1": {"mask": "holes", "p": 0.1}, "tail": {"mask": "tail"},
                   "causal+holes+p0.1": {"mask": "holes", "p": 0.1, "causal": True}, "steep": {"mask": "holes", "score": "steep"}}
# self-attention, both sides ragged: (route, B, Sq, Sk, q_len, k_len).  Each the padded shape of SHAPES that reaches the route, with
# the lengths that reach the edge named
RAGGED_SELF = [
    ("packed", 3, 30, 30, (30, 3, 17), (30, 3, 17)),        # packed forward: a second tile of one row; an entry shorter than a tile
    ("packed", 2, 64, 64, (64, 1), (64, 1)),                # the full chunk beside a single token
    ("small", 1, 30, 30, (7,), (7,)),                       # B = 1: general kernels, 2 waves, the second wholly past q_len
    ("resident", 2, 70, 130, (70, 33), (130, 64)),          # an entry with one chunk fewer than the padded shape; waves wholly past q_len
    ("resident", 2, 70, 130, (1, 65), (1, 65)),             # one token; a second chunk of one key
    ("streamed", 2, 40, 300, (40, 16), (300, 257)),         # last chunk of one key
    ("causal", 3, 65, 65, (65, 64, 1), (65, 64, 1)),
    ("causal", 2, 130, 130, (130, 17), (130, 17)),
]
RAGGED_RANGE = [("range", 3, 70, 130, (70, 5, 48)), ("range", 2, 40, 300, (40, 16))]      # queries ragged, keys dense, B = sources
RAGGED_GROUPED = [
    ("grouped", 5, 30, 130, 2, (1, 0, 1, 1, 0), (30, 1, 16, 17, 9)),
    ("grouped_stream", 5, 40, 300, 2, (0, 1, 1, 0, 1), (40, 3, 33, 16, 1)),
    ("grouped", 5, 30, 130, 3, (1, 0, 1, 1, 0), (30, 1, 16, 17, 9)),      # a third source that no row reads: its dk / dv are zeros
]
# o_lo on the non-ragged masked routes (the dense suite has o_lo on PLAIN problems only): dense rows, holes + p0.1
O_LO_DENSE = [("resident", 2, 70, 130, 2, None, False), ("streamed", 2, 40, 300, 2, None, False),
              ("grouped", 5, 30, 130, 2, (1, 0, 1, 1, 0), True), ("grouped_stream", 5, 40, 300, 2, (0, 1, 1, 0, 1), True)]


def _lens_tag(q_len, k_len):
    tag = "" if q_len is None else ":q" + ".".join(str(n) for n in q_len)
    return tag + ("" if k_len is None or k_len == q_len else ":k" + ".".join(str(n) for n in k_len))


def ragged_spec(route, B, Sq, Sk, U, idx, grouped, variant, q_len, k_len):
    v = RAGGED_VARIANTS[variant]
    name = variant + _lens_tag(q_len, k_len) + (f":U{U}" if grouped and U != 2 else "") + ("" if q_len is not None else ":dense")
    return RaggedSpec(route, B, 2, Sq, Sk, U, idx, grouped, v.get("mask"), v.get("causal", False), v.get("p", 0.0), v.get("score", "randn"),
                      False, name, q_len, k_len, "shuffled" if q_len is not None else "dense")


def ragged_specs():
    """Every case of the ragged suite (H = 2).  Self-attention: no mask, holes, holes + p0.1, steep per shape, causal + holes + p0.1 on the
    squares; range mode: no mask, holes, holes + p0.1; grouped: holes, holes + p0.1, tail; the four dense o_lo cases: holes + p0.1."""
    out = []
    for route, B, Sq, Sk, ql, kl in RAGGED_SELF:
        for variant in ("none", "holes", "holes+p0.1") + (("causal+holes+p0.1",) if Sq == Sk else ()) + ("steep",):
            out.append(ragged_spec(route, B, Sq, Sk, B, None, False, variant, ql, kl))
    for route, B, Sq, Sk, ql in RAGGED_RANGE:
        for variant in ("none", "holes", "holes+p0.1"):
            out.append(ragged_spec(route, B, Sq, Sk, B, None, False, variant, ql, None))
    for route, B, Sq, Sk, U, idx, ql in RAGGED_GROUPED:
        for variant in ("holes", "holes+p0.1", "tail"):
            out.append(ragged_spec(route, B, Sq, Sk, U, idx, True, variant, ql, None))
    for route, B, Sq, Sk, U, idx, grouped in O_LO_DENSE:
        out.append(ragged_spec(route, B, Sq, Sk, U, idx, grouped, "holes+p0.1", None, None))
    return out


def norm_rel(got, ref):
    """the measure of tests/test_hip_packing.py: ||got - ref|| / ||ref||"""
    return float((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-30))
