"""The nearest-code step of the VQ-KD tokenizer at the pre-training shape -- B = 64 images x 196 patches = 12544 rows against 8192 codes of
32 components -- as one `xfm_vq_assign` launch against the reference's ATen lines (norm_ema_quantizer.py:153-162: F.normalize, the
[M, n_code] fp32 distance matrix, argmin; plus the one-hot histogram of :166-170), and `VQKD.get_codebook_indices` at B = 64 with a 12-block
encoder; then what the token branch adds to a pre-training step's MIM loss: the lm_head GEMMs and cross-entropy over every patch row with
the unmasked ones labelled -100 (the shipped form) against the same node over the 75 masked rows per image gathered beforehand
(profiles/vq_tokenizer.md).  `--step` adds the pre-training step itself -- bench.py's model, batch and forward call, forward + backward
without the optimizer, dropout on -- with the flag off and on, alternating.

Device events around `--iters` back-to-back calls after `--warmup` calls of the same form, the forms alternating over `--rounds`, median
reported; peak allocated memory per form (reset before its timed calls); the box's clocks are read under the kernel's load after the timed
rounds (bench.sample_clocks).  Recorded, not gated.

    python tools/bench_vq_assign.py [--iters 20] [--warmup 5] [--rounds 5] [--batch 64] [--codes 8192] [--dim 32] [--depth 12]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import sample_clocks  # noqa: E402
from xfm_amd import functional as Fx  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402


def timed(fn, iters, warmup):
    """(milliseconds per call by device events, peak bytes allocated above the level before the calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, torch.cuda.max_memory_allocated() - base


def aten_lines(z, weight, n_code):
    zf = F.normalize(z, p=2, dim=-1)
    d = zf.pow(2).sum(dim=1, keepdim=True) + weight.pow(2).sum(dim=1) - 2 * torch.einsum('bd,nd->bn', zf, weight)
    idx = torch.argmin(d, dim=1)
    return idx, F.one_hot(idx, n_code).type(z.dtype).sum(0)


def step_forms(B, n, K, depth):
    """bench.py's pre-training step (its config, batch and forward call; forward + backward, no optimizer) without and with the flag."""
    from bench import FULL_CFG
    from xfm_amd.model_pretrain import XFM
    hb = syn.pretrain_batch(B, seed=1234)
    b = {k: v.cuda() for k, v in hb.items()}
    lens = hb["text_atts"].sum(1)
    forms = {}
    for name, extra in (("step_flag_off", {}),
                        ("step_flag_on", dict(use_vision_tokenizer=True, tokenizer_model="vqkd_encoder_base_decoder_3x768x12_clip",
                                              tokenizer_weight=None, codebook_size=n, codebook_dim=K, tokenizer_depth=depth))):
        torch.manual_seed(1234)
        m = XFM(dict(FULL_CFG, **extra))
        if extra:   # a trained codebook: unit rows, `initted` set
            q = m.vqkd.quantize.embedding
            q.weight.data.copy_(F.normalize(syn.gaussian("bench.vq.code", (n, K)), dim=-1))
            q.initted.fill_(1.0)
        m.cuda().finalize().train()

        def step(m=m):
            losses = m(b["image"], b["text_ids"], b["text_atts"], text_ids_masked=b["text_ids_masked"], masked_pos=b["masked_pos"],
                       masked_ids=b["masked_ids"], ret_mim_loss=True, data_source="image", text_lens=lens)
            (losses["loss_itc"] + losses["loss_itm"] + losses["loss_mlm"] + losses["loss_mim"]).backward()
            m.zero_grad()
        forms[name] = step
    return forms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--codes", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--step", action="store_true", help="also time the pre-training step (forward + backward) with use_vision_tokenizer off / on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vq_assign: needs the GPU (no fallback)")
    from xfm_amd.arena import LinearSlot, ParamArena
    from xfm_amd.model_vqkd import vqkd_encoder_base_decoder_3x768x12_clip
    from xfm_amd.ops import linear_ce
    B, n, K = a.batch, a.codes, a.dim
    M = B * 196
    z = syn.gaussian("bench.vq.z", (M, K)).cuda()
    code = F.normalize(syn.gaussian("bench.vq.code", (n, K)), dim=-1).cuda()
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.empty(M, dtype=torch.int64, device="cuda")
    forms = {"xfm_vq_assign": lambda: Fx.vq_assign(z, code, counts=counts, out=out), "aten_lines": lambda: aten_lines(z, code, n)}
    agree = float((forms["xfm_vq_assign"]() == forms["aten_lines"]()[0]).double().mean())

    tok = vqkd_encoder_base_decoder_3x768x12_clip(pretrained=True, as_tokenzer=True, n_code=n, code_dim=K, encoder_depth=a.depth)
    sd = syn.formula_state_dict(tok.state_dict())
    sd["quantize.embedding.weight"] = F.normalize(sd["quantize.embedding.weight"].float(), dim=-1)
    sd["quantize.embedding.initted"] = torch.ones(1)
    tok.load_state_dict(sd)
    tok.cuda().finalize()
    image = syn.gaussian("bench.vq.image", (B, 3, 224, 224)).cuda()
    forms["get_codebook_indices"] = lambda: tok.get_codebook_indices(image)

    # the token head of the MIM loss: every patch row with -100 on the unmasked ones, against the masked rows gathered beforehand
    head = torch.nn.Linear(768, n).cuda()
    slot = LinearSlot("lm_head", [head.weight], [head.bias])
    arena = ParamArena(head, [slot], torch.device("cuda"))
    x = syn.gaussian("bench.vq.x", (B, 196, 768)).cuda().to(torch.bfloat16)
    mask = syn.mim_block_mask(B, 14, 75, seed=1).cuda().bool()
    tokens = forms["xfm_vq_assign"]().view(B, 196).clone()
    rows = mask.reshape(-1).nonzero().flatten()   # (outside the timed region: a fixed-capacity device compaction would produce it)

    def head_all():
        xx = x.detach().requires_grad_(True)
        linear_ce(xx, slot, torch.where(mask, tokens, -100)).backward()

    def head_masked():
        xx = x.detach().requires_grad_(True)
        linear_ce(xx.reshape(-1, 768).index_select(0, rows), slot, tokens.reshape(-1).index_select(0, rows)).backward()
    forms["lm_head_all_rows"], forms["lm_head_masked_rows"] = head_all, head_masked

    if a.step:
        forms.update(step_forms(B, n, K, a.depth))
    ms = {k: [] for k in forms}
    peak = {k: 0 for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            t, p = timed(fn, a.iters * (20 if k in ("xfm_vq_assign", "aten_lines") else 1), a.warmup)   # (a window of tens of ms for each form)
            ms[k].append(t)
            peak[k] = max(peak[k], p)
            arena.zero_grad()
    res = {k: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "peak_MiB": round(peak[k] / 2 ** 20, 1)} for k, v in ms.items()}
    print(json.dumps({"shape": {"M": M, "n_code": n, "K": K, "batch": B, "encoder_depth": a.depth}, "agree_with_aten": agree, **res}))
    print(json.dumps({"clocks_under_vq_assign": sample_clocks(forms["xfm_vq_assign"], n_steps=400)}))


if __name__ == "__main__":
    main()
