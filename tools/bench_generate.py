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
--only uncached).

    python tools/bench_generate.py --sampling [--batch 32] [--samples 5] ...

times SAMPLED generation at the captioning-with-samples shape (32 images x 5 samples = 160 rows over 32 encoder states through
encoder_batch_index, 577 encoder tokens, max_length 20, 12 layers): fused_sampling on (one xfm_sample_token launch per step) and off
(the torch sampling lines) alternately in one process, at (top_k, top_p) = (0, 1) and (50, 0.9), temperature 1, no penalty; seven rounds
after a warm-up, as above.  --only NAME runs one variant alone (for a kernel trace of the sampler: --sampling --only "fused (50")."""
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
    names = ("gemm_nt", "ln_fwd", "ln_post_fwd", "attn_fwd", "decode_attn", "next_token", "sample_token", "embed_ln_fwd")
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


def time_rounds(variants, rounds):
    """Every variant once per round, interleaved; round 0 is warm-up -> {name: [seconds]}."""
    times = {name: [] for name, _ in variants}
    for r in range(rounds + 1):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r > 0:
                times[name].append(time.perf_counter() - t0)
    return times


def sampling(a, m):
    """fused_sampling on / off at two filter settings -> the result dict."""
    B, n, pad = a.batch, a.samples, m.config.pad_token_id
    rows = B * n
    enc = (0.7 * torch.randn(B, a.enc_tokens, 768, device="cuda")).to(torch.bfloat16)
    index = torch.arange(B, device="cuda").repeat_interleave(n)
    prompt = torch.zeros((rows, 1), dtype=torch.int64, device="cuda")   # <s>

    def run(fused, top_k, top_p):
        return m._generate_no_beam_search(prompt, 1, a.max_length, True, 1.0, top_k, top_p, 1.0, pad, [a.eos], rows, sync_every=8,
                                          fused_sampling=fused, encoder_hidden_states=enc, encoder_batch_index=index)

    variants = []
    for top_k, top_p in ((0, 1.0), (50, 0.9)):
        for fused in (True, False):
            variants.append((f"{'fused' if fused else 'torch'} ({top_k}, {top_p})", (lambda f=fused, k=top_k, p=top_p: run(f, k, p))))
    if a.only:
        variants = [v for v in variants if v[0].startswith(a.only)]
    with torch.no_grad():
        times = time_rounds(variants, a.rounds)
        calls = {name: count_library_calls(fn) for name, fn in variants}
    steps = a.max_length - 1
    return {"mode": "sampling", "shape": {"images": B, "samples": n, "rows": rows, "enc_tokens": a.enc_tokens, "max_length": a.max_length,
                                          "layers": a.layers, "steps": steps},
            "rounds": a.rounds,
            "ms": {k: {"median": 1e3 * statistics.median(v), "min": 1e3 * min(v), "max": 1e3 * max(v)} for k, v in times.items()},
            "ms_per_step": {k: 1e3 * statistics.median(v) / steps for k, v in times.items()},
            "library_calls_per_generation": calls}


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
    ap.add_argument("--sampling", action="store_true", help="time sampled generation, fused_sampling on and off")
    ap.add_argument("--samples", type=int, default=5, help="--sampling: samples per image")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate needs the GPU (there is no CPU timing to report)")
    from xfm_amd.xroberta import RobertaConfig, RobertaForCausalLM
    torch.manual_seed(0)
    m = RobertaForCausalLM(RobertaConfig(num_hidden_layers=a.layers, fusion_layer=0, encoder_width=768)).cuda().finalize().eval()
    if a.sampling:
        line = json.dumps(sampling(a, m))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
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
    with torch.no_grad():
        times = time_rounds(variants, a.rounds)
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
