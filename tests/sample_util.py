"""fp64 restatement of xfm_sample_token (csrc/decode.hip; xbert.py:1434-1441 and top_k_top_p_filtering :1487-1519) on CPU tensors, built
on decode_util.penalised64 and next_token_ref (test infrastructure; any device; neither is edited).

Per row:  z = penalised logit / temperature (fp64 from the fp32 inputs; the kernel's z is that value after one fp32 product or quotient
of the penalty and the fp32 divide by the temperature:
    b_z = U32 |z| [penalised] + U32/2 |z| [temperature != 1]          decode_util's "U32 |x'| covers a rounding and a one-ulp division" for the
                                                                     penalty, and the half-ulp of the correctly rounded temperature divide)
  top-k   t = the k'-th largest z with multiplicity, z >= t stays;
  top-p   order = descending z, equal values in ascending column order; c = the inclusive running softmax over that order; position i stays
          iff i == 0 or c[i - 1] <= top_p (top_p as the fp32 the kernel holds).  n = the count that stays; n_lo / n_hi = the counts with
          top_p - DELTA / top_p + DELTA: a row is SHARP when n_lo == n_hi, and only then is the kept set of an fp32 summation determined.
  draw    over a kept set: m = max z, w = exp(z - m), Z = sum w, C = the inclusive running sum of w in ascending COLUMN order;
          tok = the lowest kept column with C > u Z (none: the highest kept column with w > 0);  lp = z_tok - m - log Z.
  b_lp    next_token_ref's bound on the filtered row (its ce_fwd_ref lse bound + U32 (|z_tok| + |lp|)), plus what the kernel adds:
          3 max_kept b_z (the lse and the maximum each move by at most the largest column error, z_tok by its own), U32 |z_tok - m| (the
          kernel rounds that difference before it subtracts log Z) and U32 for the 2^-44 fixed-point floors of the weights (V 2^-44 of
          Z >= 1, below 2^-27 = U32 / 16: rounded up to one U32)."""
import torch

from decode_util import next_token_ref, penalised64
from gemm_strided_util import U32

F64 = torch.float64
DELTA = 1e-4
NEG = -float("inf")


def f32(v):
    """The fp32 value the kernel holds for a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def tempered64(logits, V, ids, cur_len, penalty, temperature):
    """-> (z fp64 [B, V], b_z fp64 [B, V])."""
    raw = logits[:, :V].double()
    x = penalised64(logits[:, :V], ids, cur_len, penalty)
    T = f32(temperature)
    z = x / T
    b_z = (U32 * (x != raw).double() + (0.5 * U32 if T != 1.0 else 0.0)) * z.abs() * (1 + 2.0 ** -20)
    b_z = torch.where(torch.isfinite(z), b_z, torch.zeros_like(b_z))
    return z, b_z


def row_is_bad(z):
    """The rows the kernel gives up on: a NaN, a +inf, or no finite value -> tok 0, lp NaN."""
    return bool(torch.isnan(z).any() or (z == float("inf")).any() or not torch.isfinite(z).any())


def filter_ref(z, top_k, top_p):
    """One row z fp64 [V] -> dict(order, c, kept, n, n_lo, n_hi, topk): order = the columns top-k keeps, under the tie rule; c = the
    inclusive running softmax over it; kept = bool [V] of the final set (the first n of order); topk = bool [V] after top-k alone."""
    V = z.numel()
    topk = torch.ones(V, dtype=torch.bool)
    if top_k > 0:
        k = min(max(top_k, 1), V)
        topk = z >= torch.topk(z, k).values[-1]
    idx = topk.nonzero().squeeze(1)
    order = idx[torch.sort(-z[idx], stable=True).indices]   # stable: equal values keep their ascending columns
    c = torch.cumsum(torch.softmax(z[order], 0), 0)
    prev = torch.cat([torch.zeros(1, dtype=F64), c[:-1]])
    if top_p < 1.0:
        P = f32(top_p)
        n, n_lo, n_hi = (max(1, int((prev <= P + d).sum())) for d in (0.0, -DELTA, DELTA))
    else:
        n = n_lo = n_hi = order.numel()
    kept = torch.zeros(V, dtype=torch.bool)
    kept[order[:n]] = True
    return dict(order=order, c=c, kept=kept, n=n, n_lo=n_lo, n_hi=n_hi, topk=topk)


def draw_ref(z, kept, u):
    """One row: the draw over `kept` (bool [V]) with the uniform u -> dict(tok, lp, C (normalised by Z, [V]), m, Z)."""
    zk = torch.where(kept, z, torch.full_like(z, NEG))
    m = zk.max()
    w = torch.exp(zk - m)
    C = torch.cumsum(w, 0)
    Z = C[-1]
    hit = (kept & (C > u * Z)).nonzero()
    tok = int(hit[0]) if hit.numel() else int((kept & (w > 0)).nonzero()[-1])
    return dict(tok=tok, lp=float(z[tok] - m - torch.log(Z)), C=C / Z, m=float(m), Z=float(Z))


def token_accepted(C, kept, tok, u, delta=DELTA):
    """The kernel's token against the fp64 running sum: kept, and C[tok - 1] - delta <= u <= C[tok] + delta (C of the last kept column
    before tok; 0 before the first)."""
    if not bool(kept[tok]):
        return False
    before = C[:tok][kept[:tok]]
    lo = float(before[-1]) if before.numel() else 0.0
    return lo - delta <= u <= float(C[tok]) + delta


def lp_bound(z, b_z, kept, tok, unfinished_row=1):
    """(lp, b_lp) fp64 of log_softmax(filtered row)[tok] for the kernel's arithmetic (module docstring)."""
    filt = torch.where(kept, z, torch.full_like(z, NEG)).view(1, -1)
    r = next_token_ref(filt, z.numel(), torch.zeros(1, 1, dtype=torch.int64), 0, 1.0, torch.tensor([unfinished_row]), 0, [],
                       next_token=torch.tensor([tok]))
    m = float(filt.max())
    extra = 3 * float(b_z[kept].max()) + U32 * (abs(float(z[tok]) - m) + 1.0)
    return float(r["lp"][0]), float(r["b_lp"][0]) + extra


def sample_ref(logits, V, ids, cur_len, penalty, temperature, top_k, top_p, u, unfinished, pad_id, eos_ids):
    """The whole step on CPU tensors (u: fp32 [B]) -> dict(z, b_z, rows (per row: filter_ref's dict + draw_ref's + lp, b_lp, bad),
    tok, add, flag, unfinished, count): the bookkeeping is next_token_ref's for the drawn tokens."""
    z, b_z = tempered64(logits, V, ids, cur_len, penalty, temperature)
    rows, toks = [], []
    for b in range(z.shape[0]):
        if row_is_bad(z[b]):
            rows.append(dict(bad=True, tok=0, lp=float("nan"), b_lp=0.0, kept=torch.ones(V, dtype=torch.bool)))
        else:
            f = filter_ref(z[b], top_k, top_p)
            f.update(draw_ref(z[b], f["kept"], float(u[b])))
            f["lp"], f["b_lp"] = lp_bound(z[b], b_z[b], f["kept"], f["tok"])
            f["bad"] = False
            rows.append(f)
        toks.append(rows[-1]["tok"])
    tok = torch.tensor(toks)
    book = next_token_ref(torch.zeros(z.shape[0], V), V, ids, cur_len, 1.0, unfinished, pad_id, eos_ids, next_token=tok)
    return dict(z=z, b_z=b_z, rows=rows, tok=tok, add=book["add"], flag=book["flag"], unfinished=book["unfinished"], count=book["count"])
