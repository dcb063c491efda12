"""fp64 references, elementwise error bounds and shared cases of the kernels that carry tokens into and out of the towers (test
infrastructure; any device; no GPU code): embedding.hip, rows.hip, vit_input.hip and the loss half of mim.hip.  Poison, sentinels and the
checkers are gemm_strided_util's, poisoned_in / Outs and the LayerNorm bounds rowwise_util's.  The host test runs an fp32 emulation of every
formula through the check_* functions below, the GPU tests run the kernels' outputs through the same functions: `got` is a dict of tensors
either way, `rep(kernel, case, width, quantity, ratio, kind)` takes each worst err / bound ratio (kind "f32" or "bf16").

u32 = 2^-23 = two fp32 unit roundoffs, one term per rounding; a sum of n terms is charged n roundings relative to sum |term|, whatever its
order (atomics, per-wave accumulators, block partials and ordered folds alike).

Embedding forward: x = word[id] + type + pos[p] is two fp32 adds, x_err = 2 u32 (|word| + |type| + |pos|), handed to rowwise_util.ln_fwd_ref
    as the input perturbation of the row it normalises (the POST / LS mechanism): mean, rstd and y carry that function's bounds.
    Dropout: y' = keep ? y * scale : 0 is one more product, b' = scale b + u32 |y'| on kept elements, 0 +- 0 on dropped ones.
Embedding backward, from the GIVEN mean / rstd / pos_ids: dz is rowwise_util.ln_bwd_ref's dx with dy = dy16 (+ dy32: one add, the (parts - 1)
    u32 of that function) (* scale on kept elements: one product, dy_err = u32 |dy'|).  The kernel forms xh from its own fp32 x, off by
    e_xh = rstd x_err from the exact row's: dz moves by at most rstd (e_xh |c2| + |xh| mean(|g| e_xh)), a dgamma term by |dy| e_xh.
    dword[v] = dword0[v] + sum of dz over the live tokens with id v (v != pad), dpos likewise by position id (the pad row excluded unless
    pos_mode = 1): count adds onto the running value, (count + 1) u32 (|initial| + sum |dz|) + sum (the dz bounds); a row no token adds
    to is the initial value +- 0.  dgamma, dbeta, dtype: rowwise_util.colsum_bound over the live rows, adds = 1.
rows_scatter_add / rows_segment_sum: exact terms summed in fp32 onto the initial value: (hits + 1) u32 (|initial| + sum |term|); no hits
    (a skipped, negative or absent key): the initial value +- 0.  rows_gather: a copy, compared with torch.equal.
vit_tokens: forward a copy.  dtok[s, i] sums the kept rows b = s (mod Bt): reps u32 sum |term|.  dcls / dmask_token pass through chunk
    partials and the set fold and are added onto the caller's value: (terms + 64) u32 sum |term| + u32 |initial|.
patchify: fp32 -> bf16 round-to-nearest-even of a gather, compared with torch.equal.
pool_rows forward: the fp32 mean of N - 1 exact bf16 values, (N + 2) u32 mean |v| (N - 2 adds, the product with a rounded 1 / (N - 1)),
    then one bf16 rounding.  Backward: fma(dy[b, 0], inv, dy[b, n]) with inv = fp32(1 / (N - 1)): one rounding, u32 |result|, then one bf16
    rounding.  (inv is itself rounded, by at most u32 / 2 relative to |dy[b, 0]| / (N - 1) and not to the result; where the two terms
    nearly cancel that is more than u32 |result| -- up to 1.2e3 u32 |result| before the bf16 rounding on these cases -- and is carried by the
    2^15 u32 |result| of the bf16 rounding, which an element uses up only when it lies on a rounding boundary.  None here does: the host
    test's emulation, which rounds inv the same way, stays at 0.996 of this bound.)
MIM loss: sums[0] / sums[1] are sums of squares, every term >= 0: (terms + 64) u32 sum (terms = rows * D); sums[2] is a count, exact.
    dx = k (x - t), k in fp64 from the sums[2] the kernel is given: x - t is one rounding, k two (the denominator's product is exact below
    2^24, the division, 2 g is exact), the product one: 4 u32 |ref| covers them twice; then one bf16 rounding.  Unmasked patch rows, and
    cls rows without the cls term, are exactly zero."""
import math

import torch

from gemm_strided_util import NAN, SENTINEL, U32, assert_outside_untouched, check_bf16, check_f32, embed_vec  # noqa: F401
from rowwise_util import BF16, EPS, F32, F64, Outs, colsum_bound, ln_bwd_ref, ln_fwd_ref, ln_stats, poisoned_in, randn  # noqa: F401

PAD = 1
I32, U8 = torch.int32, torch.uint8


def cdiv(a, b):
    return -(-a // b)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def dev(c, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


def bits_equal(a, b):
    it = {F32: I32, BF16: torch.int16}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def check_equal(got, ref, what):
    """bit equality (the sign of a zero counts); returns 0.0 so the reporters can treat it as a ratio"""
    assert bits_equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.numel()} elements differ from the exact result"
    return 0.0


def reporter(where, limits=None):
    """rep(kernel, case, width, quantity, ratio, kind): prints one `token-ratio <where> ...` line; limits = {"f32": .., "bf16": ..} makes
    it assert the ratio by kind as well (the host test's condition on the emulation)"""
    def rep(kernel, case, width, what, ratio, kind):
        print(f"token-ratio {where} {kernel} {case} {width} {what} {ratio:.3g}")
        if limits is not None:
            assert ratio <= limits[kind], f"{kernel} {case} {width} {what}: at {ratio:.3g} of the {kind} bound (limit {limits[kind]})"
    return rep


def tags_of(cases, key):
    """the `reaches` tags of the entry of a case list whose leading fields are key"""
    return next(c[-1] for c in cases if c[:len(key)] == key)


# ------------------------------------------------------------------------------------------- launch arithmetic (copied from the host sides)
def emb_fwd_grid(rows):
    return min(cdiv(rows, 4), 2048)               # embedding.hip: one wave per token, four per workgroup, 2048 workgroups at most


def emb_bwd_grid(rows):
    return max(1, min(cdiv(rows, 16), 256))       # emb_grid


def vit_chunks(Bt, Bx, P):
    """chunks of vit_tokens_bwd, or 0 where the call is rejected"""
    chunks = 4
    while chunks > 1 and Bx * chunks * 2 > Bt * P:
        chunks >>= 1
    return chunks if Bx * chunks * 2 <= Bt * P else 0


def vit_fwd_grid(Bx, P, D):
    return min(cdiv(Bx * (P + 1) * (D // 4), 256), 8192)


def vit_bwd_grid(Bt, P, D):
    return min(cdiv(Bt * P * (D // 4), 256), 8192)


def patchify_threads(B, C, H, W, P):
    return B * (H // P) * (W // P) * (C * P * P // 8)


MIM_PARTIALS = 512                                  # XFM_MIM_PARTIALS: workgroups of the forward, four waves each
REDUCE_GROUPS_FROM = 512                            # reduce_sets_groups: 64 * REDUCE_SETS_GROUPS partial rows and more are folded in 8 groups


# ------------------------------------------------------------------------------------------------------------------------- embedding
# name: (D, B, T, V, pos_mode, row_map, what the case is there to reach)
EMB_CASES = {
    "small768": (768, 3, 5, 200, 0, False, ("bwd one workgroup", "head pad", "tail pad", "all-pad row")),                  # 15 rows < 16
    "small1024_bert": (1024, 3, 5, 200, 1, False, ("bwd one workgroup", "D 1024", "pos_mode 1")),
    "t64_1024": (1024, 4, 64, 200, 0, False, ("D 1024", "T 64", "head pad", "tail pad", "all-pad row")),
    "t65_768": (768, 5, 65, 200, 0, False, ("T > 64", "pad straddles 64", "single token in the second ballot")),
    "t130_1024": (1024, 6, 130, 200, 0, False, ("D 1024", "T > 64", "pad straddles 64", "valid token after a pad past 64", "third ballot partial")),
    "t130_768_map": (768, 6, 130, 200, 0, True, ("T > 64", "row_map", "valid token after a pad past 64", "third ballot partial")),
    "t130_1024_bert_map": (1024, 6, 130, 200, 1, True, ("D 1024", "pos_mode 1", "row_map")),
    # 64 * 65 = 4160 > 256 workgroups * 16 rows = 4096: some backward waves take a fifth row; 0.6 * 4160 live rows / 12 ids = 200 hits a table row
    "bwd_stride_1024": (1024, 64, 65, 12, 0, True, ("D 1024", "bwd grid-stride", "hundreds of hits", "row_map", "pad straddles 64")),
    # 64 * 130 = 8320 > 2048 workgroups * 4 waves = 8192: the first 128 forward waves take a second row; 8320 / 50 = 166 hits
    "fwd_stride_768": (768, 64, 130, 50, 0, False, ("fwd grid-stride", "bwd grid-stride", "hundreds of hits", "T > 64")),
}


def emb_case(name):
    """CPU tensors of one embedding case.  Sequence 0 ends in pads, 1 starts with them, 2 is all pad, 3 has pads on positions 62 ... 66,
    4 a pad on 63 alone, 5 pads on 100 ... 110 (those that exist); ids are uniform in [0, V), so a few more pads lie anywhere.
    row_map: about 60 % of the rows live, sequence 0 (with it the first row) and the last row skipped, packed in order from output row 1
    on, with three output rows nothing maps to (0 and the last two)."""
    D, B, T, V, pos_mode, mapped, reaches = EMB_CASES[name]
    seed = 7000 + 37 * sorted(EMB_CASES).index(name)
    g = _gen(seed)
    ids = torch.randint(0, V, (B, T), generator=g)
    ids[0, T - max(1, T // 4):] = PAD
    ids[1, :max(1, T // 5)] = PAD
    ids[1, max(1, T // 5)] = 5
    ids[2] = PAD
    if B > 3 and T >= 64:
        ids[3, 62:min(T, 67)] = PAD
    if B > 4 and T > 64:
        ids[4, 60:T] = 7
        ids[4, 63] = PAD
    if B > 5 and T > 110:
        ids[5, 100:111] = PAD
        ids[5, 111:] = 9
    rows = B * T
    c = {"name": name, "D": D, "B": B, "T": T, "V": V, "pos_mode": pos_mode, "rows": rows, "reaches": reaches, "ids": ids,
         "word": randn((V, D), 0.1, seed + 1), "pos": randn((T + 2, D), 0.1, seed + 2), "typ": randn((D,), 0.1, seed + 3),
         "w": 1.0 + randn((D,), 0.3, seed + 4), "b": randn((D,), 0.2, seed + 5), "row_map": None, "out_rows": rows}
    if mapped:
        live = torch.rand((rows,), generator=g) < 0.62
        live[:T] = False
        live[-1] = False
        rank = torch.cumsum(live.int(), 0) - 1
        c["row_map"] = torch.where(live, rank + 1, torch.full_like(rank, -1)).to(I32)
        c["out_rows"] = int(live.sum()) + 3
    orows = c["out_rows"]
    c["dy"], c["dy32"] = randn((orows, D), 1.0, seed + 6).to(BF16), randn((orows, D), 0.5, seed + 7)
    if mapped:      # the rows of dy no token maps to are never read
        unm = torch.ones(orows, dtype=torch.bool)
        unm[c["row_map"][c["row_map"] >= 0].long()] = False
        c["dy"][unm], c["dy32"][unm] = NAN, NAN
    c["dword0"], c["dpos0"] = randn((V, D), 0.5, seed + 8), randn((T + 2, D), 0.5, seed + 9)
    c["dword0"][PAD] = 0.0
    if pos_mode == 0:
        c["dpos0"][PAD] = 0.0
    c["dgamma0"], c["dbeta0"], c["dtype0"] = torch.full((D,), 0.5), torch.full((D,), 0.25), torch.full((D,), -0.5)
    return c


def emb_live(c):
    """(live unpacked rows [n] int64, their output rows [n] int64)"""
    if c["row_map"] is None:
        r = torch.arange(c["rows"], device=c["ids"].device)
        return r, r
    lr = (c["row_map"] >= 0).nonzero()[:, 0]
    return lr, c["row_map"][lr].long()


def emb_pos_ids(c):
    """[B, T] int64: oracle.xfm_oracle.roberta_position_ids, or arange(T) for pos_mode 1"""
    from oracle.xfm_oracle import roberta_position_ids
    if c["pos_mode"]:
        return torch.arange(c["T"], device=c["ids"].device).unsqueeze(0).expand(c["B"], -1).contiguous()
    return roberta_position_ids(c["ids"], PAD)


def emb_reaches(c, tag):
    """whether case c has the property a `reaches` tag names (the host test asserts every one)"""
    ids, T, rows = c["ids"], c["T"], c["rows"]
    pad = ids == PAD
    if tag == "bwd one workgroup":
        return rows < 16 and emb_bwd_grid(rows) == 1
    if tag == "bwd grid-stride":
        return emb_bwd_grid(rows) == 256 and rows > 256 * 4 * 4
    if tag == "fwd grid-stride":
        return emb_fwd_grid(rows) == 2048 and rows > 2048 * 4
    if tag == "D 1024":
        return c["D"] == 1024
    if tag == "pos_mode 1":
        return c["pos_mode"] == 1
    if tag == "T 64":
        return T == 64
    if tag == "T > 64":
        return T > 64
    if tag == "head pad":
        return bool((pad[:, 0] & ~pad[:, -1]).any())
    if tag == "tail pad":
        return bool((~pad[:, 0] & pad[:, -1]).any())
    if tag == "all-pad row":
        return bool(pad.all(1).any())
    if tag == "pad straddles 64":
        return T > 64 and bool((pad[:, 63] & pad[:, 64] & ~pad.all(1)).any())
    if tag == "single token in the second ballot":      # t = 64: the second 64-token ballot holds one position, j <= t cuts the rest
        return T == 65 and bool((~pad[:, 64]).any())
    if tag == "valid token after a pad past 64":
        later = torch.flip(torch.cumsum(torch.flip((~pad).int(), [1]), 1), [1]) > 0     # a valid token at or after t
        return T > 66 and bool((pad[:, 65:-1] & later[:, 66:]).any())
    if tag == "third ballot partial":
        return 128 < T < 192 and bool((~pad[:, 128:]).any())
    if tag == "hundreds of hits":
        return int(torch.bincount(ids.reshape(-1)).max()) >= 150
    if tag == "row_map":
        rm = c["row_map"]
        live = rm >= 0
        frac = float(live.float().mean())
        return (0.5 < frac < 0.7 and not bool(live[0]) and not bool(live[-1]) and not bool(live[:T].any())
                and c["out_rows"] > int(live.sum()) and int(rm.max()) < c["out_rows"])
    raise KeyError(tag)


def emb_rows64(c, pid):
    """(X fp64 [rows, D], x_err): the row the kernel normalises and the bound on its two fp32 adds"""
    a = c["word"].double()[c["ids"].reshape(-1)]
    p = c["pos"].double()[pid.reshape(-1)]
    t = c["typ"].double().unsqueeze(0)
    return a + t + p, 2 * U32 * (a.abs() + t.abs() + p.abs())


def emb_rows32(c, pid):
    """the same row in fp32, in the kernel's order: (word + type) + pos"""
    return (c["word"][c["ids"].reshape(-1)] + c["typ"].unsqueeze(0)) + c["pos"][pid.reshape(-1)]


def emb_stats(c):
    """fp32 (mean, rstd, pos_ids int32) handed to the backward: the statistics of the fp32 rows; NaN / 0 on rows the row_map skips, which
    the kernel must not read"""
    pid = emb_pos_ids(c)
    mean, rstd = ln_stats(emb_rows32(c, pid))
    pid32 = pid.reshape(-1).to(I32)
    if c["row_map"] is not None:
        dead = c["row_map"] < 0
        mean[dead], rstd[dead], pid32[dead] = NAN, NAN, 0
    return mean, rstd, pid32


def _sent(shape, dtype, device):
    return torch.full(shape, SENTINEL, dtype=dtype, device=device)


def check_emb_fwd(c, got, rep, keep=None, drop_scale=1.0, tag=""):
    """got: y [out_rows, D] bf16, y32 fp32, mean / rstd [rows] fp32, pos_ids [rows] int32 (7.0's bits where nothing was written).
    keep: [rows, D] bool by UNPACKED row, or None."""
    name, D = c["name"], c["D"]
    pid = emb_pos_ids(c)
    lr, orow = emb_live(c)
    X, x_err = emb_rows64(c, pid)
    ref = ln_fwd_ref(X[lr], c["w"], c["b"], EPS, x_err[lr])
    sent_i = _sent((1,), F32, pid.device).view(I32)
    want_pid = sent_i.expand(c["rows"]).clone()
    want_pid[lr] = pid.reshape(-1)[lr].to(I32)
    assert torch.equal(got["pos_ids"], want_pid), f"{name}: pos_ids differ from the reference (or a skipped row was written)"
    for q in ("mean", "rstd"):
        rep("emb_fwd", name, D, tag + q, check_f32(got[q][lr].contiguous(), *ref[q], q), "f32")
        if lr.numel() < c["rows"]:
            dead = c["row_map"] < 0
            check_equal(got[q][dead], _sent((int(dead.sum()),), F32, pid.device), f"{q} of skipped rows")
    y, by = ref["y"]
    if keep is not None:
        s = float(torch.tensor(drop_scale, dtype=F32))
        k = keep[lr]
        y = torch.where(k, y * s, torch.zeros_like(y))
        by = torch.where(k, by * s + U32 * y.abs(), torch.zeros_like(by))
    assert bool(torch.isfinite(got["y32"][orow]).all()), "y32 not finite"
    rep("emb_fwd", name, D, tag + "y32", check_f32(got["y32"][orow], y, by, "y32"), "f32")
    rep("emb_fwd", name, D, tag + "y16", check_bf16(got["y"][orow], y, by, "y"), "bf16")
    if lr.numel() < c["rows"]:       # output rows nothing maps to keep every bit
        unm = torch.ones(c["out_rows"], dtype=torch.bool, device=pid.device)
        unm[orow] = False
        n = int(unm.sum())
        assert n >= 3
        check_equal(got["y32"][unm], _sent((n, D), F32, pid.device), "y32 rows no token maps to")
        check_equal(got["y"][unm], _sent((n, D), BF16, pid.device), "y rows no token maps to")


def table_sum(keys, valid, dz, bdz, init):
    """(ref, bound) of init + the rows of dz added to row keys[r] where valid[r] (see the header)"""
    k = keys[valid]
    n = init.shape[0]
    z = torch.zeros(init.shape, dtype=F64, device=dz.device)
    S, A, Bz = z.clone().index_add_(0, k, dz[valid]), z.clone().index_add_(0, k, dz[valid].abs()), z.clone().index_add_(0, k, bdz[valid])
    cnt = torch.bincount(k, minlength=n).unsqueeze(1)
    i0 = init.double()
    bound = (cnt + 1) * U32 * (A + i0.abs()) + Bz
    return i0 + S, torch.where(cnt > 0, bound, torch.zeros_like(bound)), cnt[:, 0]


def emb_bwd_ref(c, mean, rstd, pid32, use_dy32, keep=None, drop_scale=1.0):
    """-> dict of (ref, bound): dz ([live rows, D]), dword, dpos, dgamma, dbeta, dtype; plus "hits": the largest count of a table row"""
    lr, orow = emb_live(c)
    pid = pid32.long()
    X, x_err = emb_rows64(c, pid)
    X, x_err = X[lr], x_err[lr]
    parts = [c["dy"][orow].double()] + ([c["dy32"][orow].double()] if use_dy32 else [])
    dy_err = None
    if keep is not None:
        s = float(torch.tensor(drop_scale, dtype=F32))
        k = keep[lr]
        parts = [torch.where(k, p * s, torch.zeros_like(p)) for p in parts]
        dy_err = U32 * sum(parts).abs()
    r = ln_bwd_ref(parts, X, mean[lr], rstd[lr], c["w"], dy_err=dy_err)
    dz, bdz = r["dx"]
    DY, e_dy = r["dy"]
    xh = r["xh"]
    rs = rstd[lr].double().unsqueeze(1)
    e_xh = rs * x_err
    g = DY * c["w"].double()
    c2 = (g * xh).mean(1, keepdim=True)
    bdz = bdz + rs * (e_xh * c2.abs() + xh.abs() * (g.abs() * e_xh).mean(1, keepdim=True))
    ids = c["ids"].reshape(-1)[lr]
    pl = pid[lr]
    out = {"dz": (dz, bdz)}
    out["dword"] = table_sum(ids, ids != PAD, dz, bdz, c["dword0"])[:2]
    pvalid = torch.ones_like(pl, dtype=torch.bool) if c["pos_mode"] else pl != PAD
    ref, bound, cnt = table_sum(pl, pvalid, dz, bdz, c["dpos0"])
    out["dpos"], out["hits"] = (ref, bound), int(torch.bincount(ids[ids != PAD]).max())
    out["dgamma"] = colsum_bound(DY * xh, e_dy * xh.abs() + DY.abs() * e_xh, c["dgamma0"])
    out["dbeta"] = colsum_bound(DY, e_dy, c["dbeta0"])
    out["dtype"] = colsum_bound(dz, bdz, c["dtype0"])
    return out


def check_emb_bwd(c, got, ref, rep, tag=""):
    """got: dword, dpos, dgamma, dbeta, dtype fp32 (and dz [live rows, D] where the caller has it)"""
    name, D = c["name"], c["D"]
    if "dz" in got:
        rep("emb_bwd", name, D, tag + "dz", check_f32(got["dz"], *ref["dz"], "dz"), "f32")
    for q in ("dword", "dpos", "dgamma", "dbeta", "dtype"):
        rep("emb_bwd", name, D, tag + q, check_f32(got[q], *ref[q], q), "f32")
    assert float(got["dword"][PAD].abs().max()) == 0.0, "the word table's pad row took a gradient"
    if not c["pos_mode"]:
        assert float(got["dpos"][PAD].abs().max()) == 0.0, "the position table's pad row took a gradient"


DROP_P, DROP_SEED, DROP_CASE = 0.1, 0x1234567890ABCDEF, "t130_768_map"


def binomial_window(p, n, sigmas=5.0):
    """(lo, hi) of the kept fraction of n independent elements kept with probability 1 - p"""
    s = sigmas * math.sqrt(p * (1.0 - p) / n)
    return 1.0 - p - s, 1.0 - p + s


def check_keep_fraction(keep, p):
    lo, hi = binomial_window(p, keep.numel())
    frac = float(keep.double().mean())
    assert lo <= frac <= hi, f"kept fraction {frac:.5f} outside [{lo:.5f}, {hi:.5f}] (p = {p}, {keep.numel()} elements)"
    return frac


# -------------------------------------------------------------------------------------------------------------------------- rows.hip
def rows_threads(R, D):
    return R * (D >> 3)                           # rows.hip: one 16-byte chunk (8 bf16) a thread, cpr = D >> 3 chunks a row


def rows_grid(R, D):
    return cdiv(rows_threads(R, D), 256)


def seg_passes(D):
    return cdiv(D, 1024)                          # rows_segment_sum_kernel: c = threadIdx.x * 4; c < D; c += 1024


# (R, D, S, index pattern, what the case is there to reach): R index entries, S rows on the indexed side.  R * D / 8 threads: 1, 255, 256,
# 257 at D = 8; D = 1032: 129 chunks a row (no power of two)
ROWS_CASES = [(1, 8, 3, "mixed", ("1 thread", "D 8")),
              (255, 8, 40, "mixed", ("255 threads", "-1 entries", "repeats", "a destination never named")),
              (256, 8, 40, "mixed", ("256 threads", "-1 entries", "repeats")),
              (257, 8, 40, "mixed", ("257 threads", "-1 entries", "repeats")),
              (37, 64, 11, "mixed", ("D 64", "-1 entries", "repeats", "a destination never named")),
              (21, 768, 9, "mixed", ("D 768", "-1 entries", "repeats")),
              (300, 1032, 5, "one", ("cpr 129", "every row onto one destination")),
              (300, 64, 7, "one", ("D 64", "every row onto one destination")),
              (19, 2048, 6, "mixed", ("D 2048", "-1 entries", "repeats")),
              (33, 1032, 12, "mixed", ("cpr 129", "-1 entries", "repeats", "a destination never named"))]
ROWS_SHAPES = [c[:4] for c in ROWS_CASES]
# every path of the issue's list; the host test asserts that the tags of ROWS_CASES cover them
ROWS_PATHS = {"1 thread", "255 threads", "256 threads", "257 threads", "D 8", "D 64", "D 768", "cpr 129", "D 2048", "-1 entries", "repeats",
              "a destination never named", "every row onto one destination"}


def rows_case(R, D, S, pattern, seed=0):
    """index: "mixed" = uniform in [-1, S) with entries 0 and R - 1 set to -1 when R > 2 and one destination never named (S - 1, when
    S > 2); "one" = every row mapped to row 2.  The same index serves the gather (rows of src16 / src32, [S, D]) and the scatter (rows of
    dst0, [S, D], from upd16 [R, D])."""
    g = _gen(9100 + seed + R * 7 + D)
    if pattern == "one":
        index = torch.full((R,), 2, dtype=I32)
    else:
        hi = S - 1 if S > 2 else S
        index = torch.randint(-1, hi, (R,), generator=g).to(I32)
        if R > 2:
            index[0], index[R - 1] = -1, -1
    return {"R": R, "D": D, "S": S, "pattern": pattern, "reaches": tags_of(ROWS_CASES, (R, D, S, pattern)), "index": index,
            "src16": randn((S, D), 1.0, 9200 + seed + D).to(BF16), "src32": randn((S, D), 1.0, 9300 + seed + D),
            "upd16": randn((R, D), 1.0, 9400 + seed + R).to(BF16), "dst0": randn((S, D), 2.0, 9500 + seed + D)}


def rows_reaches(c, tag):
    """whether case c has the property a `reaches` tag names: the launch from the host side's arithmetic, the index pattern from the index"""
    R, D, idx = c["R"], c["D"], c["index"]
    if tag.endswith(" thread") or tag.endswith(" threads"):
        n = int(tag.split()[0])       # n threads: cdiv(n, 256) workgroups, the last with n - 256 (cdiv(n, 256) - 1) threads past its guard
        return rows_threads(R, D) == n and rows_grid(R, D) == cdiv(n, 256) and D % 8 == 0
    if tag == "cpr 129":
        return D >> 3 == 129 and rows_threads(R, D) > 256
    if tag.startswith("D "):
        return D == int(tag[2:]) and D % 8 == 0
    hit = torch.bincount(idx[idx >= 0].long(), minlength=c["S"])
    if tag == "-1 entries":
        return bool((idx == -1).any()) and bool((idx >= 0).any())
    if tag == "repeats":
        return int(hit.max()) > 1 and int((hit > 0).sum()) > 1
    if tag == "a destination never named":
        return c["S"] > 2 and int(hit[-1]) == 0 and int(hit.sum()) > 0
    if tag == "every row onto one destination":
        return R >= 300 and int(hit.max()) == R
    raise KeyError(tag)


def gather_ref(src, index):
    out = src[index.clamp(min=0).long()]
    return torch.where((index >= 0).unsqueeze(1), out, torch.zeros_like(out))


def hits_sum(terms, keys, valid, init):
    """(ref, bound) of init[k] += terms[r] for keys[r] = k, valid[r]: (hits + 1) u32 (|init| + sum |term|), 0 where nothing is added"""
    T = terms.double()
    zero = torch.zeros_like(T)
    return table_sum(keys.long(), valid, T, zero, init)[:2]


# (R, D, n keys, skip key, what the case is there to reach): int64 keys in [-2, n keys), sorted by the caller.  One workgroup per position,
# 256 threads * 4 columns = 1024 columns a pass: D = 8 keeps two threads busy, D = 1032 two in the second pass, D = 2048 all of them
_SEG_KEYS = ("negative keys", "skip key", "run ending at R")
SEG_CASES = [(1, 8, 1, 5, ("one row", "one column pass")),
             (300, 8, 12, 3, _SEG_KEYS + ("one column pass", "D 8")),
             (257, 64, 20, 7, _SEG_KEYS + ("one column pass", "D 64")),
             (90, 768, 9, 2, _SEG_KEYS + ("one column pass", "D 768")),
             (300, 1032, 3, 1, _SEG_KEYS + ("second column pass", "second column pass partial", "long runs")),
             (40, 2048, 6, 0, _SEG_KEYS + ("second column pass", "second column pass full", "D 2048"))]
SEG_SHAPES = [c[:4] for c in SEG_CASES]
SEG_PATHS = set(_SEG_KEYS) | {"one row", "one column pass", "second column pass", "second column pass partial", "second column pass full",
                              "D 8", "D 64", "D 768", "D 2048", "long runs"}


def seg_case(R, D, nk, skip, seed=0):
    g = _gen(9600 + seed + R + D)
    keys = torch.randint(-2, nk, (R,), generator=g)
    if R > 3:
        keys[0], keys[1], keys[2] = -1, skip, nk - 1
    return {"R": R, "D": D, "nk": nk, "skip": skip, "reaches": tags_of(SEG_CASES, (R, D, nk, skip)), "keys": keys,
            "src": randn((R, D), 1.0, 9700 + seed + D), "out0": randn((nk, D), 2.0, 9800 + seed + D)}


def seg_reaches(c, tag):
    """whether case c has the property a `reaches` tag names: column passes from the kernel's loop, the key pattern from the sorted keys"""
    R, D = c["R"], c["D"]
    skey = torch.sort(c["keys"], stable=True)[0]
    if tag == "one row":
        return R == 1
    if tag == "one column pass":
        return seg_passes(D) == 1 and D % 4 == 0
    if tag == "second column pass":
        return D > 1024 and seg_passes(D) == 2
    if tag == "second column pass partial":      # 0 < threads of the second pass < 256
        return seg_passes(D) == 2 and 0 < (D - 1024) // 4 < 256
    if tag == "second column pass full":
        return seg_passes(D) == 2 and (D - 1024) // 4 == 256
    if tag.startswith("D "):
        return D == int(tag[2:])
    if tag == "negative keys":
        return int(skey[0]) < 0 and int(skey[-1]) >= 0
    if tag == "skip key":
        return bool((skey == c["skip"]).any()) and 0 <= c["skip"] < c["nk"]
    if tag == "run ending at R":                 # the last run is summed: its loop ends on j < R, not on a change of key
        return int(skey[-1]) >= 0 and int(skey[-1]) != c["skip"]
    if tag == "long runs":
        return int(torch.bincount(skey[skey >= 0]).max()) >= 40
    raise KeyError(tag)


# ------------------------------------------------------------------------------------------------------------------------ ViT tokens
# name: (D, Bt, reps, P, mask pattern, chunks the host side picks)
VIT_CASES = {
    "chunks4_ragged": (768, 3, 2, 21, "clean_view", 4),      # Bx * 8 = 48 <= 63; per = 6: chunks 0-6, 6-12, 12-18, 18-21
    "chunks4_empty": (64, 2, 1, 9, "random", 4),            # Bx * 8 = 16 <= 18; per = 3: the fourth chunk starts at 9 = P
    "chunks2": (1024, 2, 2, 9, "all", 2),                   # Bx * 8 = 32 > 18 >= Bx * 4 = 16; per = 5: 0-5, 5-9
    "chunks1": (768, 3, 2, 5, "random", 1),                 # Bx * 4 = 24 > 15 >= Bx * 2 = 12
    "chunks1_nomask": (64, 1, 2, 4, "none", 1),             # 8 > 4 >= 4
    "nomask_768": (768, 3, 1, 20, "none", 4),
    "fold_groups": (64, 64, 2, 16, "random", 4),            # Bx * chunks = 512 partial rows: the set fold splits them into 8 groups
    # 42 * 197 * 256 = 2 118 144 > 8192 * 256 = 2 097 152 float4s forward, 42 * 196 * 256 = 2 107 392 backward: both grid-stride loops
    "grid_stride": (1024, 42, 1, 196, "random", 4),
}
VIT_REJECTED = (64, 1, 3, 5)                                # Bt * P = 5 < 2 * Bx = 6


def vit_case(name):
    D, Bt, reps, P, pattern, chunks = VIT_CASES[name] if name != "rejected" else VIT_REJECTED + ("random", 0)
    seed = 9900 + 13 * (sorted(VIT_CASES).index(name) if name in VIT_CASES else 99)
    Bx = Bt * reps
    g = _gen(seed)
    if pattern == "none":
        mask = None
    elif pattern == "all":
        mask = torch.ones((Bx, P), dtype=U8)
    else:
        mask = (torch.rand((Bx, P), generator=g) < 0.4).to(U8)
        if pattern == "clean_view":
            mask[0], mask[Bx - 1] = 0, 1           # a clean view and a fully masked one among them
    return {"name": name, "D": D, "Bt": Bt, "Bx": Bx, "reps": reps, "P": P, "pattern": pattern, "chunks": chunks, "mask": mask,
            "tok": randn((Bt * P, D), 1.0, seed + 1), "cls": randn((D,), 1.0, seed + 2), "mtok": randn((D,), 1.0, seed + 3),
            "dx0": randn((Bx * (P + 1), D), 1.0, seed + 4), "dcls0": randn((D,), 1.0, seed + 5), "dmtok0": randn((D,), 1.0, seed + 6)}


def vit_reaches(c):
    Bt, Bx, P, D = c["Bt"], c["Bx"], c["P"], c["D"]
    ch = vit_chunks(Bt, Bx, P)
    ok = ch == c["chunks"]
    per = cdiv(P, ch) if ch else 0
    n = c["name"]
    if n == "chunks4_ragged":
        ok = ok and P % ch != 0 and (ch - 1) * per < P and bool((c["mask"][0] == 0).all()) and bool(c["mask"][1:].any())
    if n == "chunks4_empty":
        ok = ok and (ch - 1) * per >= P and D < 1024
    if n in ("chunks2", "chunks1"):
        ok = ok and P % max(ch, 2) != 0
    if n == "fold_groups":
        ok = ok and Bx * ch >= REDUCE_GROUPS_FROM
    if n == "grid_stride":
        ok = ok and Bx * (P + 1) * (D // 4) > 8192 * 256 and Bt * P * (D // 4) > 8192 * 256 and vit_fwd_grid(Bx, P, D) == 8192 and vit_bwd_grid(Bt, P, D) == 8192
    if n == "rejected":
        ok = ch == 0 and Bt * P < 2 * Bx
    return ok


def vit_fwd_ref(c):
    """x0 [Bx * (P + 1), D] fp32, exact"""
    Bt, Bx, P, D = c["Bt"], c["Bx"], c["P"], c["D"]
    x = c["tok"].view(Bt, P, D).repeat(c["reps"], 1, 1)
    if c["mask"] is not None:
        x = torch.where(c["mask"].bool().unsqueeze(-1), c["mtok"].view(1, 1, D).expand(Bx, P, D), x)
    return torch.cat([c["cls"].view(1, 1, D).expand(Bx, 1, D), x], 1).reshape(Bx * (P + 1), D)


def vit_bwd_ref(c):
    """{dtok, dcls, dmtok: (ref, bound)}; without a mask dmtok is its initial value +- 0"""
    Bt, Bx, P, D, reps = c["Bt"], c["Bx"], c["P"], c["D"], c["reps"]
    G = c["dx0"].double().view(Bx, P + 1, D)
    gp = G[:, 1:]
    m = c["mask"].bool().unsqueeze(-1) if c["mask"] is not None else torch.zeros((Bx, P, 1), dtype=torch.bool, device=G.device)
    kept = torch.where(m, torch.zeros_like(gp), gp).view(reps, Bt, P, D)
    out = {"dtok": (kept.sum(0).reshape(Bt * P, D), reps * U32 * kept.abs().sum(0).reshape(Bt * P, D))}
    c0 = c["dcls0"].double()
    out["dcls"] = (c0 + G[:, 0].sum(0), (Bx + 64) * U32 * G[:, 0].abs().sum(0) + U32 * c0.abs())
    m0 = c["dmtok0"].double()
    if c["mask"] is None:
        out["dmtok"] = (m0, torch.zeros_like(m0))
    else:
        msk = torch.where(m, gp, torch.zeros_like(gp))
        out["dmtok"] = (m0 + msk.sum((0, 1)), (int(m.sum()) + 64) * U32 * msk.abs().sum((0, 1)) + U32 * m0.abs())
    return out


def check_vit_bwd(c, got, rep):
    ref = vit_bwd_ref(c)
    for q in ("dtok", "dcls", "dmtok"):
        rep("vit_tokens_bwd", c["name"], c["D"], q, check_f32(got[q], *ref[q], q), "f32")
    if c["mask"] is None:
        check_equal(got["dmtok"], c["dmtok0"], "dmask_token without a mask")


# --------------------------------------------------------------------------------------------------------------------------- patchify
# (B, C, P, H, W); the last: 56 * 196 patches * 96 threads = 1 053 696 > 4096 * 256 = 1 048 576 threads
PATCH_CASES = [(2, 3, 16, 32, 48), (3, 3, 8, 16, 8), (2, 1, 16, 16, 16), (2, 3, 32, 64, 32), (56, 3, 16, 224, 224)]


def patchify_ref(img, P):
    B, C, H, W = img.shape
    return img.view(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), C * P * P).to(BF16)


# -------------------------------------------------------------------------------------------------------------------------- pool_rows
POOL_D, POOL_N, POOL_B = (8, 64, 768, 1024), (2, 3, 50, 197), 3


# what each width and each row count is there to reach.  pool_rows_fwd: one workgroup a sample, 2 * (D / 8) threads, column group
# threadIdx % (D / 8), row phase threadIdx / (D / 8); phase ph adds rows 1 + ph, 3 + ph, ...
POOL_D_TAGS = {8: ("smallest workgroup",), 64: ("part of a wave a phase",), 768: ("three waves a phase",), 1024: ("full workgroup",)}
POOL_N_TAGS = {2: ("row phase 1 idle", "even N"), 3: ("one row a phase", "odd N"), 50: ("even N", "phases differ by a row"),
               197: ("odd N", "phases alike")}
POOL_PATHS = {t for tags in list(POOL_D_TAGS.values()) + list(POOL_N_TAGS.values()) for t in tags}


def pool_fwd_block(D):
    return 2 * (D // 8)


def pool_phase_rows(N, ph):
    return len(range(1 + ph, N, 2))


def pool_case(D, N, seed=0):
    s = 10100 + seed + D + 3 * N
    return {"D": D, "N": N, "B": POOL_B, "reaches": POOL_D_TAGS[D] + POOL_N_TAGS[N], "y": (randn((POOL_B * N, D), 1.0, s) + 0.25).to(BF16),
            "dy": randn((POOL_B * N, D), 1.0, s + 1).to(BF16)}


def pool_reaches(c, tag):
    D, N = c["D"], c["N"]
    blk, p0, p1 = pool_fwd_block(D), pool_phase_rows(N, 0), pool_phase_rows(N, 1)
    return {"smallest workgroup": blk == 2 and D == 8, "part of a wave a phase": 2 < blk < 64, "three waves a phase": blk == 192,
            "full workgroup": blk == 256 and D == 1024, "row phase 1 idle": N == 2 and (p0, p1) == (1, 0),
            "one row a phase": (p0, p1) == (1, 1), "even N": N % 2 == 0 and p0 == p1 + 1, "odd N": N % 2 == 1 and p0 == p1,
            "phases differ by a row": p0 == p1 + 1 and p1 > 1, "phases alike": p0 == p1 and p1 > 1}[tag] and p0 + p1 == N - 1


def pool_fwd_ref(c):
    """(ref, b32) of row 0 of every sample, [B, D]"""
    v = c["y"].double().view(c["B"], c["N"], c["D"])[:, 1:]
    return v.mean(1), (c["N"] + 2) * U32 * v.abs().mean(1)


def pool_bwd_ref(c):
    """(ref, b32) [B * N, D]; row 0 of every sample 0 +- 0"""
    B, N, D = c["B"], c["N"], c["D"]
    g = c["dy"].double().view(B, N, D)
    g0 = g[:, :1] / (N - 1)
    ref = g + g0
    b = U32 * ref.abs()
    ref[:, 0], b[:, 0] = 0.0, 0.0
    return ref.reshape(B * N, D), b.expand(B, N, D).reshape(B * N, D)


def check_pool(c, got_fwd, got_bwd, rep):
    B, N, D = c["B"], c["N"], c["D"]
    case = f"N{N}"
    f = got_fwd.view(B, N, D)
    rep("pool_rows_fwd", case, D, "row0", check_bf16(f[:, 0].contiguous(), *pool_fwd_ref(c), "pooled row"), "bf16")
    check_equal(f[:, 1:].contiguous(), c["y"].view(B, N, D)[:, 1:].contiguous(), "rows 1 .. N - 1 of pool_rows_fwd_")
    rep("pool_rows_bwd", case, D, "out", check_bf16(got_bwd, *pool_bwd_ref(c), "pool_rows_bwd"), "bf16")
    assert float(got_bwd.view(B, N, D)[:, 0].float().abs().max()) == 0.0, "row 0 of pool_rows_bwd is not zero"


# --------------------------------------------------------------------------------------------------------------------------- MIM loss
# D = 8: one lane busy; 512: one pass of the wave; 520: a second pass of one lane; (B, N): 4 rows; 185; 57 * 37 = 2109 > 512 workgroups * 4
# waves = 2048: the first 61 waves take a second row
MIM_D, MIM_BN = (8, 512, 520, 768, 1024), ((2, 2), (5, 37), (57, 37))
MIM_MASKS = ("random", "none", "all", "one_image")
MIM_GOUT = 3.0
# what each width, row count and mask is there to reach (forward: lane l of a row's wave takes columns 8 l + 512 k)
MIM_D_TAGS = {8: ("one lane busy", "D <= 512"), 512: ("one full pass", "D <= 512"), 520: ("second pass of one lane",),
              768: ("second pass of half the wave",), 1024: ("two full passes", "D 1024")}
MIM_BN_TAGS = {(2, 2): ("one workgroup", "4 rows"), (5, 37): ("185 rows", "below the forward cap"), (57, 37): ("forward grid-stride",)}
MIM_MASK_TAGS = {"random": ("some patches masked",), "none": ("no patch masked",), "all": ("every patch masked",),
                 "one_image": ("one image masked next to clean ones",)}
MIM_PATHS = {t for tags in list(MIM_D_TAGS.values()) + list(MIM_BN_TAGS.values()) + list(MIM_MASK_TAGS.values()) for t in tags}


def mim_fwd_grid(B, N):
    return min(cdiv(B * N, 4), MIM_PARTIALS)      # mim.hip: one wave per row, four per workgroup, XFM_MIM_PARTIALS workgroups at most


def mim_lanes(D, k):
    """lanes of a wave with columns in pass k of the forward's `c = lane * 8; c < D; c += 512` loop"""
    return max(0, min(64, cdiv(D - 512 * k, 8)))


def mim_case(D, B, N, pattern, seed=0):
    s = 10500 + seed + D + 7 * B
    g = _gen(s)
    if pattern == "none":
        mask = torch.zeros((B, N - 1), dtype=U8)
    elif pattern == "all":
        mask = torch.ones((B, N - 1), dtype=U8)
    elif pattern == "one_image":
        mask = torch.zeros((B, N - 1), dtype=U8)
        mask[B // 2] = 1
    else:
        mask = (torch.rand((B, N - 1), generator=g) < 0.4).to(U8)
        mask[0, 0] = 1
    return {"D": D, "B": B, "N": N, "pattern": pattern, "reaches": MIM_D_TAGS[D] + MIM_BN_TAGS[(B, N)] + MIM_MASK_TAGS[pattern], "mask": mask,
            "x": randn((B * N, D), 1.0, s + 1).to(BF16), "t": randn((B * N, D), 1.0, s + 2).to(BF16), "gout": torch.tensor([MIM_GOUT])}


def mim_reaches(c, tag):
    """whether case c has the property a `reaches` tag names: passes and grid from the host side's arithmetic, the rest from the mask"""
    m, B, N, D = c["mask"], c["B"], c["N"], c["D"]
    rows, grid, l0, l1 = B * N, mim_fwd_grid(B, N), mim_lanes(D, 0), mim_lanes(D, 1)
    n = int(m.sum())
    return {"one lane busy": (l0, l1) == (1, 0), "D <= 512": D <= 512 and l1 == 0, "one full pass": (l0, l1) == (64, 0),
            "second pass of one lane": D > 512 and D % 512 == 8 and (l0, l1) == (64, 1), "second pass of half the wave": (l0, l1) == (64, 32),
            "two full passes": (l0, l1) == (64, 64) and mim_lanes(D, 2) == 0, "D 1024": D == 1024,
            "one workgroup": grid == 1, "4 rows": rows == 4, "185 rows": rows == 37 * 5,
            "below the forward cap": 1 < grid < MIM_PARTIALS and rows <= 4 * grid,
            "forward grid-stride": grid == MIM_PARTIALS and 4 * MIM_PARTIALS < rows < 8 * MIM_PARTIALS,
            "some patches masked": 0 < n < B * (N - 1) or (B * (N - 1) <= 4 and n > 0), "no patch masked": n == 0 and max(n * D, 1) == 1,
            "every patch masked": n == B * (N - 1),
            "one image masked next to clean ones": B > 1 and bool(m[B // 2].all()) and n == N - 1}[tag]


def _mim_rows(c):
    B, N = c["B"], c["N"]
    d = (c["x"].double() - c["t"].double()).view(B, N, -1)
    m = c["mask"].bool()
    return d, m


def mim_fwd_ref(c):
    """([3] fp64, [3] bounds): masked-patch sum of squares, cls sum of squares, masked count"""
    d, m = _mim_rows(c)
    D = d.shape[2]
    sp = (d[:, 1:] ** 2 * m.unsqueeze(-1)).sum()
    sc = (d[:, 0] ** 2).sum()
    cnt = m.sum().double()
    ref = torch.stack([sp, sc, cnt])
    bound = torch.stack([(cnt * D + 64) * U32 * sp, (c["B"] * D + 64) * U32 * sc, torch.zeros_like(cnt)])
    return ref, bound


def mim_bwd_ref(c, sums2, cls_term):
    """(ref, b32) [B * N, D] from the sums[2] the kernel is given"""
    d, m = _mim_rows(c)
    B, N, D = d.shape
    g = float(c["gout"][0])
    kp = 2.0 * g / max(float(sums2) * D, 1.0)
    kc = 2.0 * g / (B * D) if cls_term else 0.0
    k = torch.cat([torch.full((B, 1), kc, dtype=F64, device=d.device), m.double() * kp], 1).unsqueeze(-1)
    ref = (k * d).reshape(B * N, D)
    return ref, 4 * U32 * ref.abs()


def check_mim(c, sums, dx, cls_term, rep):
    """sums: [3] fp32 as the forward left them; dx [B * N, D] bf16 of a backward that was given them"""
    D, B, N = c["D"], c["B"], c["N"]
    case = f"{B}x{N}:{c['pattern']}:cls{int(cls_term)}"
    ref, bound = mim_fwd_ref(c)
    rep("mim_loss_fwd", case, D, "sums", check_f32(sums, ref, bound, "sums"), "f32")
    assert float(sums[2]) == float(c["mask"].sum()), "sums[2] is not the number of masked patches"
    r, b = mim_bwd_ref(c, float(sums[2]), cls_term)
    rep("mim_loss_bwd", case, D, "dx", check_bf16(dx, r, b, "dx"), "bf16")
    g = dx.view(B, N, D)
    un = ~c["mask"].bool()
    if bool(un.any()):
        assert float(g[:, 1:][un].float().abs().max()) == 0.0, "an unmasked patch row carries a gradient"
    if not cls_term:
        assert float(g[:, 0].float().abs().max()) == 0.0, "cls rows carry a gradient without the cls term"
