"""Time greedy generation at the captioning shape (configs/xfm-ft/Captioning.yaml of the reference: batch 32, 384 px = 577 encoder tokens,
max_length 20) on the RoBERTa causal decoder with cross-attention in all 12 layers: the cached path (RobertaForCausalLM.
_generate_no_beam_search: one token per step through xfm_decode_attn, one xfm_next_token launch per step) against a loop over the
uncached forward (the whole prefix and the K | V projection of all 32 x 577 encoder rows in every layer at every step), which is all
a caller could do before the cache existed.

    python tools/bench_generate.py [--batch 32] [--enc-tokens 577] [--max-length 20] [--layers 12] [--rounds 7] [--out FILE.json]

Same process, the variants interleaved round by round (cached at several sync_every values, then uncached), every round ends in a device
synchronise and is timed with the host clock; the first round of each variant is warm-up and dropped.  Random initial weights, seeded
encoder states; with them no row emits --eos, so every variant runs all the steps.  Also reported: the library launches of one cached
generation (counted by wrapping xfm_amd.functional's entry points), and how many rows of the two loops part and the largest uncached
top-1 margin at the step where one does (before it both saw the same prefix, so that margin says whether the parting is a near-tie of the
16-bit arithmetic).  --only NAME runs one variant alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/bench_generate.py
--only uncached)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def uncached_greedy(m, prompt, max_length, enc, pad, eos):
    """Greedy decoding on the full forward: what the parent of the cache could do.  Device ops only; no host read in the loop."""
    ids = prompt.clone()
    unfinished = torch.ones(ids.shape[0], dtype=torch.long, device=ids.device)
    margins = []
    while ids.shape[1] < max_length:
        logits = m(ids, encoder_hidden_states=enc).logits[:, -1, :]
        top = logits.topk(2, dim=-1)
        margins.append(top.values[:, 0] - top.values[:, 1])
        add = top.indices[:, 0] * unfinished + pad * (1 - unfinished)
        ids = torch.cat([ids, add.unsqueeze(1)], dim=1)
        unfinished = unfinished * add.ne(eos).long()
    ids[:, -1].masked_fill_(unfinished.bool(), eos)   # xbert.py:1469-1470
    return ids, torch.stack(margins, dim=1)


def count_library_calls(fn):
    """Calls into xfm_amd.functional's launching wrappers while fn() runs -> {name: calls}."""
    from xfm_amd import functional as Fx
    names = ("gemm_nt", "ln_fwd", "ln_post_fwd", "attn_fwd", "decode_attn", "next_token", "embed_ln_fwd")
    counts, saved = {}, {}
    for n in names:
        saved[n] = getattr(Fx, n)

        def wrap(*a, _n=n, **kw):
            counts[_n] = counts.get(_n, 0) + 1
            return saved[_n](*a, **kw)
        setattr(Fx, n, wrap)
    try:
        fn()
    finally:
        for n in names:
            setattr(Fx, n, saved[n])
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--enc-tokens", type=int, default=577)
    ap.add_argument("--max-length", type=int, default=20)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sync-every", type=int, nargs="*", default=[1, 4, 8, 100])
    ap.add_argument("--eos", type=int, default=2)
    ap.add_argument("--only", default=None, help="run the variants whose name starts with this (cached / uncached)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate needs the GPU (there is no CPU timing to report)")
    from xfm_amd.xroberta import RobertaConfig, RobertaForCausalLM
    torch.manual_seed(0)
    m = RobertaForCausalLM(RobertaConfig(num_hidden_layers=a.layers, fusion_layer=0, encoder_width=768)).cuda().finalize().eval()
    B, pad = a.batch, m.config.pad_token_id
    enc = (0.7 * torch.randn(B, a.enc_tokens, 768, device="cuda")).to(torch.bfloat16)
    prompt = torch.zeros((B, 1), dtype=torch.int64, device="cuda")   # <s>

    def cached(sync_every):
        return m._generate_no_beam_search(prompt, 1, a.max_length, False, 1.0, 0, 1.0, 1.0, pad, [a.eos], B, sync_every=sync_every,
                                          encoder_hidden_states=enc)

    variants = [(f"cached sync_every={s}", (lambda s=s: cached(s))) for s in a.sync_every]
    variants.append(("uncached loop", lambda: uncached_greedy(m, prompt, a.max_length, enc, pad, a.eos)))
    if a.only:
        variants = [v for v in variants if v[0].startswith(a.only)]
    times = {name: [] for name, _ in variants}
    with torch.no_grad():
        for r in range(a.rounds + 1):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r > 0:   # round 0 is warm-up
                    times[name].append(time.perf_counter() - t0)
        ids_c, _ = cached(a.sync_every[0])
        ids_u, margins = uncached_greedy(m, prompt, a.max_length, enc, pad, a.eos)
        calls = count_library_calls(lambda: cached(100))
    steps = a.max_length - 1
    # the first step at which a row's tokens part; before it both loops saw the same prefix, so the margin there says whether the
    # difference is a near-tie of the 16-bit arithmetic or a defect
    differ = (ids_c != ids_u)
    first = torch.where(differ.any(1), differ.float().argmax(1), torch.full((B,), -1, device="cuda"))
    worst = 0.0
    for b in range(B):
        if int(first[b]) > 0:
            worst = max(worst, float(margins[b, int(first[b]) - 1]))
    res = {"shape": {"batch": B, "enc_tokens": a.enc_tokens, "max_length": a.max_length, "layers": a.layers, "steps": steps},
           "rounds": a.rounds,
           "ms": {k: {"median": 1e3 * statistics.median(v), "min": 1e3 * min(v), "max": 1e3 * max(v)} for k, v in times.items()},
           "ms_per_step": {k: 1e3 * statistics.median(v) / steps for k, v in times.items()},
           "library_calls_per_generation": calls, "library_calls_per_step": sum(calls.values()) / steps,
           "rows_that_part": int(differ.any(1).sum()), "largest_margin_where_they_part": worst,
           "rows_closed_by_the_forced_eos": int((ids_c[:, -1] == a.eos).sum())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
