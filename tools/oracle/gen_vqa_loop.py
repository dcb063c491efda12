"""Generate tests/golden/vqa_loop_small.npz from the REAL reference (behind ref_shim, as gen_golden.py does).

Run in the build container only:   python tools/oracle/gen_vqa_loop.py

VQA.py itself cannot be imported here (ruamel, the dataset package, a tokenizer), so, as for imagenet_loop_small: the MODEL is the
reference's XFMForVQA, the schedule is the reference's scheduler.create_scheduler, the four optimizer groups are formed by the
reference's optim.create_optimizer (its `AdamW` import is bound to the rule below when this transformers no longer ships one), and the
loop of VQA.py:35-100 is restated call for call around them on token-id batches.  The model stays in eval mode (dropout and drop-path
off), which is how the other task fixtures make the run reproducible.

Stored (data only): the learning rate of every group at every iteration, the losses, probes of a few updated parameters (a record only:
no test reads them, see where they are packed), and ONE
evaluation pass at the formula weights (the state both sides can build exactly): 5 questions, 24 candidates, k = 8 -- the candidate
token ids, the first-token probabilities, the shortlist, the re-ranked ids / probabilities and the {"question_id", "answer"} records.
The candidate list is CHOSEN from the model's own first-token distribution so that (a) the 8th and 9th first-token probabilities of every
question are apart by a recorded margin -- the shortlist does not depend on torch's unspecified tie order, nor on 16-bit towers -- and
(b) two candidates that share a first token (a tie) lie inside every shortlist."""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402  (puts the repository root on sys.path and installs nothing by itself)
import ref_shim  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

VQA_LOOP = {"B": 3, "train_seeds": [501, 502], "max_answers": 3, "answer_len": 7, "max_tokens": 30, "image_res": 224,
            "eval_B": 5, "eval_seed": 611, "A": 24, "k_test": 8, "cand_len": 6, "pad_token_id": 1,
            "optimizer": {"opt": "adamW", "lr": 1e-4, "weight_decay": 0.01, "lr_mult": 2},
            "schedular": {"sched": "linear", "lr": 1e-4, "epochs": 2, "num_warmup_steps": 0.25},
            "state_of": ["text_decoder.lm_head.dense.weight", "text_decoder.roberta.encoder.layer.1.crossattention.self.key.weight",
                         "fusion_encoder.roberta.encoder.layer.0.output.dense.weight", "text_encoder.encoder.layer.1.attention.self.query.bias",
                         "vision_encoder.blocks.1.mlp.fc2.weight"]}


class HFAdamW(torch.optim.Optimizer):
    """transformers.optimization.AdamW's rule (correct_bias=True), written out for installs that dropped the class: eps is added to
    sqrt(v) BEFORE the bias correction and the decoupled weight decay follows the update."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"], state["exp_avg"], state["exp_avg_sq"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                b1, b2 = group["betas"]
                state["step"] += 1
                state["exp_avg"].mul_(b1).add_(p.grad, alpha=1.0 - b1)
                state["exp_avg_sq"].mul_(b2).addcmul_(p.grad, p.grad, value=1.0 - b2)
                denom = state["exp_avg_sq"].sqrt().add_(group["eps"])
                step_size = group["lr"] * math.sqrt(1.0 - b2 ** state["step"]) / (1.0 - b1 ** state["step"])
                p.addcdiv_(state["exp_avg"], denom, value=-step_size)
                if group["weight_decay"] > 0.0:
                    p.add_(p, alpha=-group["lr"] * group["weight_decay"])


def _reference_optim():
    """The reference's optim.create_optimizer; `from transformers.optimization import AdamW` resolves to HFAdamW where the class is gone."""
    import transformers.optimization as to
    if not hasattr(to, "AdamW"):
        to.AdamW = HFAdamW
    sys.path.insert(0, ref_shim.REF_ROOT)
    import optim
    import scheduler
    return optim.create_optimizer, scheduler.create_scheduler


class AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def choose_candidates(first_logp, L):
    """first_logp [Q, V] log-probabilities of the first answer token.  -> (first tokens [A], report).  Seven tokens every question rates
    high (the first of them twice: the tie), sixteen it rates low (four of them twice: ties outside the shortlist)."""
    Q, V = first_logp.shape
    worst = first_logp.min(dim=0).values                       # a token's log-probability for the question that likes it least
    worst[:3] = -float("inf")                                  # <s>, <pad>, </s> start no answer
    order = torch.argsort(worst, descending=True, stable=True)
    high = order[:7].tolist()
    best = first_logp.max(dim=0).values
    low_pool = torch.argsort(best, descending=False, stable=True)   # tokens no question rates high
    low_pool = [int(t) for t in low_pool.tolist() if int(t) >= 3][:12]
    low = low_pool + low_pool[:4]
    first = [high[0], high[0]] + high[1:] + low
    assert len(first) == L["A"], len(first)
    # interleave so that candidate index does not sort by probability (the tied pair is NOT adjacent, the shortlist is not 0..7)
    perm = syn.uniform01("vqa_loop.perm", L["A"]).argsort(kind="stable")
    return torch.tensor(first)[torch.from_numpy(perm)], {"high": high, "low": low_pool}


def main():
    from types import SimpleNamespace as NS

    def build_tokenizer(*a, **kw):
        raise RuntimeError("dataset.build_tokenizer is stubbed: the reference's dataset package needs torchvision / PIL")

    ref_shim.install()
    ref_shim._stub("dataset", build_tokenizer=build_tokenizer)
    from models.model_generation import XFMForVQA
    create_optimizer, create_scheduler = _reference_optim()
    ref_shim.init_single_process_group()
    L = VQA_LOOP
    torch.manual_seed(0)
    cfg = ref_shim.pretrain_config(text_layers=2, fusion_layers=2, overrides={"pad_token_id": L["pad_token_id"], "decoder_fusion_start_at": 0,
                                                                             "num_dec_layers": 2, "image_res": L["image_res"]})
    with G.shallow_vit():
        m = XFMForVQA(cfg)
    G.load_formula(m)
    m.eval()
    out = {}

    # ---- one evaluation pass at the formula weights (VQA.py:75-100) ----
    image, (q_ids, q_atts), question_id = syn.vqa_eval_batch(L["eval_B"], seed=L["eval_seed"], image_res=L["image_res"],
                                                             max_tokens=L["max_tokens"], first_question_id=1000)
    # first-token distribution: the model's own first decoder pass (model_generation.py:150-156), on a throw-away candidate list
    probe_c = syn.pretrain_batch(2, seed=93, max_tokens=L["cand_len"], min_len=3, with_image=False)
    captured = {}
    orig_softmax = torch.nn.functional.softmax

    def spy(x, dim=None, **kw):
        r = orig_softmax(x, dim=dim, **kw)
        if x.dim() == 2 and x.shape[1] > 50000:
            captured["logits"] = x.detach().clone()
        return r

    import models.model_generation as mg
    mg.F.softmax = spy
    try:
        with torch.no_grad():
            m(image, NS(input_ids=q_ids, attention_mask=q_atts), NS(input_ids=probe_c["text_ids"], attention_mask=probe_c["text_atts"]),
              k=2, train=False)
    finally:
        mg.F.softmax = orig_softmax
    first_logp = torch.log_softmax(captured["logits"].double(), dim=1)
    first, report = choose_candidates(first_logp.clone(), L)

    best = None
    for seed in range(700, 740):   # the continuation tokens: among the first seeds, the widest winner margin
        c = syn.pretrain_batch(L["A"], seed=seed, max_tokens=L["cand_len"], min_len=3, with_image=False)
        c_ids, c_atts = c["text_ids"].clone(), c["text_atts"]
        c_ids[:, 1] = first
        with torch.no_grad():
            topk_ids, topk_probs = m(image, NS(input_ids=q_ids, attention_mask=q_atts), NS(input_ids=c_ids, attention_mask=c_atts),
                                     k=L["k_test"], train=False)
        winner_margin = float((topk_probs[:, 0] - topk_probs[:, 1]).min())
        if best is None or winner_margin > best[0]:
            best = (winner_margin, seed, c_ids, c_atts, topk_ids, topk_probs)
    winner_margin, cand_seed, c_ids, c_atts, topk_ids, topk_probs = best
    p_first = torch.softmax(captured["logits"], dim=1).index_select(1, c_ids[:, 1])          # [Q, A], fp32 as the reference forms it
    srt = torch.sort(p_first, dim=1, descending=True, stable=True)
    k = L["k_test"]
    margin = float(((srt.values[:, k - 1] - srt.values[:, k]) / srt.values[:, k - 1]).min())   # relative gap between the 8th and the 9th
    shortlist = srt.indices[:, :k]
    assert margin > 0.3, f"8th / 9th first-token probabilities too close: {margin}"
    for r in range(L["eval_B"]):
        toks = c_ids[shortlist[r], 1].tolist()
        assert len(set(toks)) < len(toks), f"question {r}: no tied pair inside the shortlist"
        assert sorted(topk_ids[r].tolist()) == sorted(shortlist[r].tolist())
    assert winner_margin > 0.2, f"winner decided by {winner_margin}"
    answer_list = [f"answer{i}" for i in range(L["A"])]
    records = [{"question_id": int(qid), "answer": answer_list[int(topk_ids[r, int(topk_probs[r].argmax())])]}
               for r, qid in enumerate(question_id)]
    print("first tokens", c_ids[:, 1].tolist(), "\nshortlist", shortlist.tolist(), "\nmargin", margin, "winner margin", winner_margin,
          "\ntopk_ids", topk_ids.tolist(), "\nrecords", records, flush=True)
    out["eval/cand_ids"], out["eval/cand_atts"] = c_ids.numpy(), c_atts.numpy()
    out["eval/p_first"] = p_first.numpy()
    out["eval/shortlist"] = shortlist.numpy()
    out["eval/topk_ids"], out["eval/topk_probs"] = topk_ids.numpy(), topk_probs.numpy()

    # ---- 2 epochs x 2 iterations (VQA.py:35-72 inside :233-238) ----
    arg_opt = AttrDict(L["optimizer"])
    optimizer = create_optimizer(arg_opt, m)
    arg_sche = AttrDict(L["schedular"])
    arg_sche['step_per_epoch'] = len(L["train_seeds"])
    lr_scheduler = create_scheduler(arg_sche, optimizer)
    names = {id(p): n for n, p in m.named_parameters()}
    groups = [[names[id(p)] for p in g["params"]] for g in optimizer.param_groups]
    loader = [syn.vqa_batch(L["B"], seed=s, image_res=L["image_res"], max_tokens=L["max_tokens"], max_answers=L["max_answers"],
                            answer_len=L["answer_len"]) for s in L["train_seeds"]]
    lrs, losses = [], []
    for epoch in range(L["schedular"]["epochs"]):
        for i, x in enumerate(loader):
            lrs.append([g["lr"] for g in optimizer.param_groups])
            loss = m(x.image, NS(input_ids=x.q_ids, attention_mask=x.q_atts), NS(input_ids=x.a_ids, attention_mask=x.a_atts), train=True,
                     k=x.k, weights=x.weights)
            loss.backward()
            optimizer.step()
            lr_scheduler.step()
            optimizer.zero_grad()
            losses.append(loss.item())
    print("lr", lrs, "\nloss", losses, flush=True)
    out["train/lr"] = np.asarray(lrs, dtype=np.float64)
    out["train/loss"] = np.asarray(losses, dtype=np.float64)
    # a record of where the reference's parameters stood after the four steps; NO test compares them across implementations (Adam's
    # first updates are sign-like: a 1e-7 gradient difference on a near-zero entry moves it by a full lr) -- the losses carry the update
    for n, p in m.named_parameters():
        if n in L["state_of"]:
            G.pack(f"train/param/{n}", p, out, 256)
    stepped = sum(1 for p in m.parameters() if p in optimizer.state)
    meta = {"spec": G.spec_of(m), "text_layers": 2, "fusion_layers": 2, "vit_depth": G.SHALLOW, "dec_layers": 2, "dec_fusion_start": 0,
            "groups": [len(g) for g in groups], "group_first": [g[0] if g else None for g in groups], "stepped": stepped,
            "betas": [0.9, 0.98], "eps": 1e-8, "num_warmup_steps": arg_sche["num_warmup_steps"],
            "num_training_steps": arg_sche["num_training_steps"], "question_ids": [int(q) for q in question_id],
            "records": records, "answer_list": answer_list, "margin_8_9": margin, "winner_margin": winner_margin, "cand_seed": cand_seed,
            **VQA_LOOP}
    G.save("vqa_loop_small", out, meta)
    print(json.dumps({k: v for k, v in meta.items() if k != "spec"})[:2000])


if __name__ == "__main__":
    main()
