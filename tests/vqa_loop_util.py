"""Shared helpers of the VQA-loop tests (test infrastructure): the fixture's configuration and batches, the CPU model path -- the oracle's
VQA forward behind an nn.Module with the reference's call form -- and the input cases of the answer-ranking kernel tests."""
from types import SimpleNamespace as NS

import torch

from golden_util import load, state_from_spec
from oracle import xfm_oracle as O
from xfm_amd import synthetic as syn


def fixture():
    return load("vqa_loop_small")


def loop_config(meta, **kw):
    cfg = {"use_beit_v2": True, "image_res": meta["image_res"], "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": meta["text_layers"], "text_fusion_start_at": meta["text_layers"],
           "fusion_num_hidden_layers": meta["fusion_layers"], "fusion_fusion_start_at": 0, "embed_dim": 256, "temp": 0.07,
           "learnable_temp": True, "max_temp": 0.5, "min_temp": 0.001, "vision_depth": meta["vit_depth"],
           "pad_token_id": meta["pad_token_id"], "decoder_fusion_start_at": meta["dec_fusion_start"], "num_dec_layers": meta["dec_layers"],
           "k_test": meta["k_test"], "start_eval": 0, "batch_size_train": meta["B"], "batch_size_test": meta["eval_B"],
           "schedular": dict(meta["schedular"]), "optimizer": dict(meta["optimizer"])}
    cfg.update(kw)
    return cfg


def train_batches(meta):
    """The fixture's two training batches in the loop's layout: (image, (q_ids, q_atts), (a_ids, a_atts), weights, n)."""
    out = []
    for s in meta["train_seeds"]:
        x = syn.vqa_batch(meta["B"], seed=s, image_res=meta["image_res"], max_tokens=meta["max_tokens"], max_answers=meta["max_answers"],
                          answer_len=meta["answer_len"])
        out.append((x.image, (x.q_ids, x.q_atts), (x.a_ids, x.a_atts), x.weights, x.k))
    return out


class TestLoader(list):
    """A list of (image, question, question_id) batches with the `dataset` the evaluation reads."""
    __test__ = False

    def __init__(self, batches, dataset):
        super().__init__(batches)
        self.dataset = dataset


def eval_loader(z, meta, splits=(2, 3)):
    """The fixture's five questions as len(splits) batches, with its candidate list."""
    image, (q_ids, q_atts), qid = syn.vqa_eval_batch(meta["eval_B"], seed=meta["eval_seed"], image_res=meta["image_res"],
                                                     max_tokens=meta["max_tokens"], first_question_id=meta["question_ids"][0])
    assert qid.tolist() == meta["question_ids"] and sum(splits) == meta["eval_B"]
    dataset = NS(answer_list=meta["answer_list"], answer_input=(torch.from_numpy(z["eval/cand_ids"]), torch.from_numpy(z["eval/cand_atts"])),
                 ann=[{"question_id": q} for q in meta["question_ids"]])
    batches, o = [], 0
    for n in splits:
        batches.append((image[o:o + n], (q_ids[o:o + n], q_atts[o:o + n]), qid[o:o + n]))
        o += n
    return TestLoader(batches, dataset)


class OracleVQA(torch.nn.Module):
    """XFMForVQA on the CPU: oracle arithmetic, the reference's forward(image, question, answer, k=, weights=, train=)."""

    def __init__(self, state, meta):
        super().__init__()
        self.names = list(state)
        self.cfg = O.default_cfg(text_layers=meta["text_layers"], fusion_layers=meta["fusion_layers"], vit_depth=meta["vit_depth"])
        self.cfg.update(dec_layers=meta["dec_layers"], dec_fusion_start=meta["dec_fusion_start"])
        self.pad = meta["pad_token_id"]
        self.init_params = []
        self._flat = {k: f"p{i}" for i, k in enumerate(self.names)}
        for k in self.names:   # `<head>.decoder.bias` IS `<head>.bias` in the reference (tied, xroberta.py:1322-1323): one parameter
            if k.endswith("decoder.bias"):
                self._flat[k] = self._flat[k[: -len("decoder.bias")] + "bias"]
        for k, v in state.items():
            if k.endswith("decoder.bias"):
                continue
            if v.dtype.is_floating_point:
                self.register_parameter(self._flat[k], torch.nn.Parameter(v.clone()))
            else:
                self.register_buffer(self._flat[k], v.clone())

    def table(self):
        return {k: getattr(self, a) for k, a in self._flat.items()}

    def named_parameters(self, *a, **kw):   # under the reference's names: the optimizer groups go by them
        back = {a: k for k, a in self._flat.items() if not k.endswith("decoder.bias")}
        for n, p in super().named_parameters(*a, **kw):
            yield back[n], p

    def forward(self, image, quesiton, answer=None, k=None, weights=None, train=True, fused=False):
        if fused:
            raise RuntimeError("rank_answer(fused=True) runs on HIP kernels: it needs GPU tensors")
        (q_ids, q_atts), (a_ids, a_atts) = quesiton, answer
        if train:
            return O.vqa_train_loss(self.table(), self.cfg, image, q_ids, q_atts, a_ids, a_atts, list(k), weights, self.pad)
        ids, probs, _ = O.vqa_rank_answer(self.table(), self.cfg, image, q_ids, q_atts, a_ids, a_atts, k, self.pad)
        return ids, probs


def oracle_model(meta):
    return OracleVQA(state_from_spec(meta["spec"]), meta)


# ------------------------------------------------------------------------------------------------ answer-ranking kernel cases
# (Q, V, ld, A, k, kind).  kind: "plain"; "wide" = logits over +-80; "ties" = half the candidates share two first tokens, boosted so that
# their tie groups straddle the cut; "aligned" = plain values in rows that start on 16 bytes (where ld != V the other kinds start them
# one float into the allocation): the model's own layout, V = 50265 in a padded ld -- 16-byte loads, then one scalar tail column
SHORTLIST_CASES = [(1, 37, 37, 1, 1, "plain"), (3, 37, 41, 7, 7, "plain"), (2, 50265, 50272, 300, 128, "wide"),
                   (5, 50265, 50265, 3128, 128, "ties"), (2, 1000, 1000, 8192, 256, "plain"), (2, 50265, 50272, 300, 128, "aligned")]


def shortlist_case(Q, V, ld, A, k, kind, seed=0):
    """-> (logits fp32 [Q, ld] (columns [V, ld) hold a huge value that must never be read), first_tok int64 [A]).
    Candidates with DIFFERENT first tokens get logits on a grid of step >= 2^-8, shuffled per question: their probabilities are then
    >= 0.39 % apart, far above the fp32 arithmetic's error, so the order of distinct values is decided; candidates that share a first
    token tie exactly, and the tie rule decides."""
    g = torch.Generator().manual_seed(1000 * seed + A + V)
    span = 80.0 if kind == "wide" else 6.0
    logits = (torch.rand(Q, ld, generator=g) * 2 - 1) * span
    n_tok = min(A, V)
    if kind == "ties":
        n_tok = A // 2 + 2
    toks = torch.randperm(V, generator=g)[:n_tok]
    if kind == "ties":
        first = torch.cat([toks[:A // 2], toks[A // 2].repeat(A // 4), toks[A // 2 + 1].repeat(A - A // 2 - A // 4)])
    else:
        first = torch.cat([toks, toks[torch.randint(0, n_tok, (A - n_tok,), generator=g)]])
    first = first[torch.randperm(A, generator=g)]
    step = max(2.0 * span / n_tok, 2.0 ** -8)
    assert step * n_tok <= 2.0 * span + 1e-6 or step == 2.0 ** -8
    for q in range(Q):
        grid = span - step * torch.randperm(n_tok, generator=g).float()
        logits[q, toks] = grid
        if kind == "ties":   # the two shared tokens sit 40 and 90 distinct candidates below the top: their groups (782 each) cross k = 128
            logits[q, toks[A // 2]] = span - step * (40 + q) - step / 2
            logits[q, toks[A // 2 + 1]] = span - step * (90 + q) - step / 2
    logits[:, V:] = 3.0e38
    return logits, first.contiguous()


def shortlist_reference(logits, V, first, k):
    """softmax -> index_select -> torch.sort(stable=True, descending=True)[:k], fp64 then fp32."""
    p = torch.softmax(logits[:, :V].double(), dim=1).index_select(1, first).float()
    s = torch.sort(p, dim=1, descending=True, stable=True)
    return s.values[:, :k], s.indices[:, :k], p
