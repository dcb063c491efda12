"""fp64 restatements, elementwise error bounds and the generation-loop restatement for the decoding kernels (csrc/decode.hip) and
xfm_amd.decode (test infrastructure; any device).  The error model is attention_util's (C_K, E_EXP, MASK_NEG) and rowwise_util's ce_fwd_ref;
both are imported, neither is edited.

decode_attn, per (b, h), head_dim 64, n keys:   s_j = scale q.k_j + (keep_j == 0 ? -10000 : 0),  P = softmax(s),  o = P.V
    score   e_s = u32 (C_K scale sum_d |q_d k_d| + 10000 masked)        C_K = 66 = 64 + 2: the kernel's 8 fmas and 3 shuffle adds of exact
            bf16 products are fewer roundings than the 64 additions the constant grants; the product with the scale and the mask add are the 2.
    P       relative e_p = e_s + u32 (1.5 |s - rowmax| + E_EXP)          __expf and the online softmax over 64-key chunks, as attention_util.
    o       sum_j P_j |v_jd| e_p,j + (|o_d| + sum_j P_j |v_jd|) (sum_j P_j e_p,j + (n + 8 chunks) u32), then check_bf16.
            attention_util's forward bound WITHOUT its u16 term: this kernel never rounds P to bf16.  n additions of the P.V sum (the 8
            partial sums met through LDS are 8 of them), per chunk one alpha multiplied into l and into the accumulator and -- one wave
            walks a chunk -- that wave's exp, product and addition where the waves meet (5 of the 8 per chunk), the division by l.

next_token, per row:  x' = penalised logits (fp64 from the fp32 inputs), tok = argmax (lowest index), lp = x'_tok - logsumexp(x')
    b_lp = b_lse(ce_fwd_ref on x') + u32 (2 max_j |x'_j| over the penalised columns + |x'_tok| + |lp|)
            ce_fwd_ref's lse bound holds for the kernel's two passes (they are ce_fwd_kernel's); the penalty is one fp32 product or
            quotient per column (u32 |x'| covers a rounding and a one-ulp division), which moves the lse by at most the largest such
            error and x'_tok by its own; the final subtraction is one rounding of |lp|."""
import torch

from attention_util import C_K, E_EXP, MASK_NEG
from gemm_strided_util import U32
from rowwise_util import ce_fwd_ref

F64 = torch.float64


def decode_attn_ref(q, K, V, keep, scale):
    """q [B, H, 64], K / V [B, n, H, 64] (the keys each row attends to, the new one last), keep int [B, n] or None -> (ref, b32) fp64
    [B, H * 64]."""
    B, H, _ = q.shape
    n = K.shape[1]
    Q, Kh, Vh = q.double().unsqueeze(2), K.double().permute(0, 2, 1, 3), V.double().permute(0, 2, 1, 3)   # [B,H,1,64], [B,H,n,64]
    s = scale * (Q @ Kh.transpose(-1, -2)).squeeze(2)                                                        # [B,H,n]
    mag = C_K * scale * (Q.abs() @ Kh.abs().transpose(-1, -2)).squeeze(2)
    if keep is not None:
        masked = (keep == 0).double().unsqueeze(1)
        s, mag = s + MASK_NEG * masked, mag - MASK_NEG * masked
    e_s = U32 * mag
    P = torch.softmax(s, -1)
    e_p = e_s + U32 * (1.5 * (s - s.max(-1, keepdim=True).values).abs() + E_EXP)
    o = (P.unsqueeze(2) @ Vh).squeeze(2)
    omag = (P.unsqueeze(2) @ Vh.abs()).squeeze(2)
    nsum = n + 8 * ((n + 63) // 64)
    lerr = (P * e_p).sum(-1, keepdim=True)
    b = ((P * e_p).unsqueeze(2) @ Vh.abs()).squeeze(2) + (o.abs() + omag) * (lerr + nsum * U32)
    return o.reshape(B, H * 64), b.reshape(B, H * 64)


def penalised64(logits, ids, cur_len, penalty):
    """xbert.py:1425-1432 in fp64: every distinct id of ids[b, :cur_len] once."""
    x = logits.double().clone()
    if penalty != 1.0:
        pen = float(torch.tensor(penalty, dtype=torch.float32))   # the kernel holds the penalty in fp32
        for b in range(x.shape[0]):
            for t in set(ids[b, :cur_len].tolist()):
                if 0 <= t < x.shape[1]:
                    x[b, t] = x[b, t] * pen if x[b, t] < 0 else x[b, t] / pen
    return x


def next_token_ref(logits, V, ids, cur_len, penalty, unfinished, pad_id, eos_ids, next_token=None):
    """fp64 restatement of xfm_next_token on CPU tensors -> dict(tok, lp, b_lp, add, flag, unfinished, count)."""
    raw = logits[:, :V].double()
    x = penalised64(logits[:, :V], ids, cur_len, penalty)
    tok = torch.argmax(x, dim=1) if next_token is None else next_token.clone()   # torch.argmax: the first of equal maxima
    for b in range(x.shape[0]):   # (spelled out: the lowest index among equal maxima)
        if next_token is None:
            tok[b] = int((x[b] == x[b].max()).nonzero()[0])
    onehot = torch.zeros_like(x)
    lse, b_lse, _, _ = ce_fwd_ref(x, onehot, torch.ones(x.shape[0], dtype=F64))
    xt = x.gather(1, tok.view(-1, 1)).squeeze(1)
    lp = xt - lse
    changed = x != raw
    pen_mag = torch.where(changed, x.abs(), torch.zeros_like(x)).max(dim=1).values
    b_lp = b_lse + U32 * (2 * pen_mag + xt.abs() + lp.abs())
    u = unfinished.long()
    add = tok * u + pad_id * (1 - u)
    new = u.clone()
    for e in eos_ids:
        new = new * add.ne(e).long()
    return dict(tok=tok, lp=lp, b_lp=b_lp, add=add, flag=u, unfinished=new, count=int(new.sum()))


def generate_ref(logits_fn, input_ids, cur_len, max_length, repetition_penalty, pad_token_id, eos_token_ids, batch_size):
    """xbert.py:1418-1484, greedy, restated in torch on CPU tensors and driven by `logits_fn(input_ids so far) -> fp32 [B, V]` (the
    last-position logits), with the reference's early break -> (input_ids [B, max_length], mean log-probabilities)."""
    input_ids = input_ids.clone()
    unfinished_sents, logprobs = [], []
    cur_unfinished = input_ids.new_ones(batch_size)
    while cur_len < max_length:
        next_token_logits = logits_fn(input_ids).float().cpu().clone()
        if repetition_penalty != 1.0:
            for i in range(batch_size):
                for previous_token in set(input_ids[i].tolist()):
                    if next_token_logits[i, previous_token] < 0:
                        next_token_logits[i, previous_token] *= repetition_penalty
                    else:
                        next_token_logits[i, previous_token] /= repetition_penalty
        next_token = torch.argmax(next_token_logits, dim=-1)
        scores = torch.log_softmax(next_token_logits, dim=-1).gather(-1, next_token.unsqueeze(-1))
        logprobs.append(scores)
        unfinished_sents.append(cur_unfinished)
        tokens_to_add = next_token * cur_unfinished + pad_token_id * (1 - cur_unfinished)
        input_ids = torch.cat([input_ids, tokens_to_add.unsqueeze(-1)], dim=-1)
        cur_len += 1
        for eos in eos_token_ids:
            cur_unfinished = cur_unfinished.mul(tokens_to_add.ne(eos).long())
        if cur_unfinished.max() == 0:
            break
    if cur_len == max_length:
        input_ids[:, -1].masked_fill_(cur_unfinished.to(dtype=torch.bool), eos_token_ids[0])
    logprobs = torch.cat(logprobs, dim=1)
    unfinished_sents = torch.stack(unfinished_sents, dim=1).float()
    mean = (logprobs * unfinished_sents).sum(dim=1) / unfinished_sents.sum(dim=1)
    pad_len = max_length - input_ids.shape[1]
    if pad_len > 0:
        input_ids = torch.cat([input_ids, input_ids.new_full((batch_size, pad_len), pad_token_id)], dim=1)
    return input_ids, mean


def finishing_invariants(ids, prompt_len, pad_id, eos_ids):
    """What every output of _generate_no_beam_search satisfies: only pads follow the first eos of a row, and a row without an eos before
    the last column ends in eos_ids[0]."""
    for row in ids.tolist():
        new = row[prompt_len:]
        hit = [i for i, t in enumerate(new) if t in eos_ids]
        if hit and hit[0] < len(new) - 1:
            assert all(t == pad_id for t in new[hit[0] + 1:]), row
        else:
            assert new[-1] == eos_ids[0], row


def decisive(z):
    """bool [steps, B] of a generation fixture: margin >= 4 e (either contender can move by e in the reference's own 16-bit arithmetic,
    so a flip needs margin < 2 e; the factor 2 over that is the margin)."""
    return torch.from_numpy(z["margin"]).double() >= 4 * torch.from_numpy(z["e"]).double()

