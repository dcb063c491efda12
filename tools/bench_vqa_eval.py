"""One VQA evaluation pass (XFMForVQA.forward(train=False) -> rank_answer, VQA.py:89-98) with the fused answer ranking
(xfm_answer_shortlist / xfm_answer_rerank, the question K/V shared through encoder_batch_index, one device read per pass) and with the
ATen path (tile(), softmax / index_select / topk, two host reads per question), side by side on one box (profiles/vqa_eval.md).
Shape of configs/xfm-ft/VQA.yaml: 32 questions per batch, 3 128 candidates of 8 tokens, k_test = 128, 480 px, 12 + 12 layers and a
12-layer answer decoder.

Both forms run in one process, alternating: HIP events around `--iters` passes after `--warmup` passes of the same form, median over
`--rounds`; the peak allocated memory of each form is taken in a pass of its own after a reset of the allocator's statistics; the box's
clocks are read under the fused form's load after the timed rounds (bench.sample_clocks) and printed as a third line.

    python tools/bench_vqa_eval.py [--iters 5] [--warmup 2] [--rounds 3] [--depth 12]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import sample_clocks  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402
from xfm_amd.model_generation import XFMForVQA  # noqa: E402

Q, A, K, RES, ANSWER_LEN, MAX_TOKENS = 32, 3128, 128, 480, 8, 40


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vqa_eval: needs the GPU (no fallback)")
    cfg = {"use_beit_v2": True, "image_res": RES, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": a.depth, "text_fusion_start_at": a.depth, "fusion_num_hidden_layers": a.depth,
           "fusion_fusion_start_at": 0, "embed_dim": 256, "temp": 0.07, "vision_depth": a.depth, "pad_token_id": 1,
           "decoder_fusion_start_at": 0, "num_dec_layers": a.depth}
    m = XFMForVQA(cfg)
    m.load_state_dict(syn.formula_state_dict(m.state_dict()), strict=True)
    m.cuda().finalize().eval()
    image, question, _ = syn.vqa_eval_batch(Q, seed=480, image_res=RES, max_tokens=MAX_TOKENS)
    image, question = image.cuda(), tuple(t.cuda() for t in question)
    c_ids, c_atts, names = syn.vqa_answer_list(A, seed=481, answer_len=ANSWER_LEN)
    answers = (c_ids.cuda(), c_atts.cuda())
    result = torch.zeros(Q, dtype=torch.int64, device="cuda")

    @torch.no_grad()
    def one_pass(fused):
        if fused:   # vqa_loop.evaluation: the winners land in a device buffer, read once per pass
            m(image, question, answers, train=False, k=K, fused=True, result=result, result_offset=0)
            return [names[i] for i in result.tolist()]
        topk_ids, topk_probs = m(image, question, answers, train=False, k=K)
        out = []
        for topk_id, topk_prob in zip(topk_ids, topk_probs):   # VQA.py:95-98
            _, pred = topk_prob.max(dim=0)
            out.append(names[topk_id[pred]])
        return out

    same = sum(x == y for x, y in zip(one_pass(True), one_pass(False)))
    times = {True: [], False: []}
    for _ in range(a.rounds):
        for fused in (False, True):
            times[fused].append(timed(lambda: one_pass(fused), a.iters, a.warmup))
    peak = {}
    for fused in (False, True):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        one_pass(fused)
        torch.cuda.synchronize()
        peak[fused] = torch.cuda.max_memory_allocated() / 2 ** 30
    for fused in (False, True):
        t = sorted(times[fused])
        print(json.dumps({"name": "vqa_eval/" + ("fused" if fused else "aten"), "ms_median": round(t[len(t) // 2] * 1e3, 3),
                          "ms_min": round(t[0] * 1e3, 3), "ms_max": round(t[-1] * 1e3, 3), "peak_allocated_gib": round(peak[fused], 3),
                          "questions": Q, "candidates": A, "k": K, "image_res": RES, "depth": a.depth, "same_winner": f"{same}/{Q}"}),
              flush=True)
    print(json.dumps({"name": "vqa_eval/clocks_under_load", **sample_clocks(lambda: one_pass(True), n_steps=4)}), flush=True)


if __name__ == "__main__":
    main()
