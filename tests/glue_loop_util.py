"""Shared helpers of the GLUE-loop tests (test infrastructure): the fixture's configuration and batches, the CPU model path -- the oracle's
text-only classification forward behind an nn.Module with the reference's call form -- and the fp64 restatement of the correlations."""
import numpy as np
import torch

from golden_util import load, state_from_spec
from oracle import xfm_oracle as O
from xfm_amd import synthetic as syn


def fixture():
    return load("glue_loop_small")


def run_spec(meta, task):
    """The fixture's state_dict spec with the head's output width of this run (the three runs differ in nothing else)."""
    L = meta["runs"][task]["num_labels"]
    spec = dict(meta["spec"])
    spec["cls_head.3.weight"] = [[L, spec["cls_head.3.weight"][0][1]], "float32"]
    spec["cls_head.3.bias"] = [[L], "float32"]
    return spec


def used_state(meta, task):
    """Formula weights of the entries the text-only branch reads (the vision tower is built and never used)."""
    return state_from_spec({k: v for k, v in run_spec(meta, task).items() if k.startswith(("text_encoder.", "cls_head."))})


def loop_config(meta, task, **kw):
    R = meta["runs"][task]
    cfg = {"use_beit_v2": True, "image_res": 224, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": meta["text_layers"], "text_fusion_start_at": meta["text_layers"],
           "fusion_num_hidden_layers": meta["fusion_layers"], "fusion_fusion_start_at": 0, "embed_dim": 256, "temp": 0.07,
           "learnable_temp": True, "max_temp": 0.5, "min_temp": 0.001, "vision_depth": meta["vit_depth"],
           "task_name": task, "num_labels": R["num_labels"], "max_length": meta["max_length"],
           "per_device_train_batch_size": meta["B"], "per_device_eval_batch_size": meta["B"], "learning_rate": meta["learning_rate"],
           "weight_decay": meta["weight_decay"], "num_train_epochs": meta["num_train_epochs"], "max_train_steps": None,
           "gradient_accumulation_steps": R["gradient_accumulation_steps"], "num_warmup_steps": meta["num_warmup_steps"],
           "lr_scheduler_type": meta["lr_scheduler_type"], "ckpt_frequent": 1, "use_huggingface_models": False}
    cfg.update(kw)
    return cfg


def _batches(meta, seeds, num_labels):
    return [syn.glue_batch(meta["B"], seed=s, max_length=meta["max_length"], min_len=meta["min_len"], num_labels=num_labels) for s in seeds]


def train_batches(meta, task):
    return _batches(meta, meta["runs"][task]["train_seeds"], meta["runs"][task]["num_labels"])


def eval_batches(meta, task, tag="eval"):
    return _batches(meta, meta["runs"][task][tag]["seeds"], meta["runs"][task]["num_labels"])


class OracleTextClassifier(torch.nn.Module):
    """XFMForClassification's text-only branch on the CPU: oracle arithmetic, the reference's forward(None, ids, atts, targets, train)."""

    def __init__(self, state, text_layers):
        super().__init__()
        self.names = list(state)
        self.cfg = O.default_cfg(text_layers=text_layers, fusion_layers=0)
        self.init_params = []
        for i, k in enumerate(self.names):
            v = state[k]
            if v.dtype.is_floating_point:
                self.register_parameter(f"p{i}", torch.nn.Parameter(v.clone()))
            else:
                self.register_buffer(f"p{i}", v.clone())

    def table(self):
        return {k: getattr(self, f"p{i}") for i, k in enumerate(self.names)}

    def named_parameters(self, *a, **kw):   # under the reference's names: the optimizer groups go by them
        back = {f"p{i}": k for i, k in enumerate(self.names)}
        for n, p in super().named_parameters(*a, **kw):
            yield back[n], p

    def forward(self, image, text_ids, text_atts, targets, train=True):
        assert image is None
        prediction = O.classification_forward(self.table(), self.cfg, None, text_ids, text_atts, deep_head=False)
        if not train:
            return prediction
        if prediction.shape[-1] == 1:
            return torch.nn.functional.mse_loss(prediction.view(-1), targets.view(-1))
        return torch.nn.functional.cross_entropy(prediction, targets)


def oracle_model(meta, task):
    return OracleTextClassifier(used_state(meta, task), meta["text_layers"])


# ------------------------------------------------------------------------------------------------ fp64 restatement of the correlations
def ranks_restated(v):
    """scipy.stats.rankdata(method='average') written out: a STABLE sort, then every run of equal values shares the mean of its 1-based
    positions.  (-0.0 == +0.0 under numpy's comparison, as under the kernel's key.)"""
    v = np.asarray(v, dtype=np.float64)
    order = np.argsort(v, kind="stable")
    ranks = np.empty(v.size, dtype=np.float64)
    i = 0
    while i < v.size:
        j = i
        while j + 1 < v.size and v[order[j + 1]] == v[order[i]]:
            j += 1
        ranks[order[i:j + 1]] = (i + 1 + j + 1) / 2.0
        i = j + 1
    return ranks


def pearson_restated(a, b):
    """Two passes in fp64: means, then centred sums; a zero denominator gives NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    da, db = a - a.mean(), b - b.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return float((da * db).sum() / den) if den > 0 else float("nan")


def correlations_restated(x, y):
    if np.isnan(np.asarray(x)).any() or np.isnan(np.asarray(y)).any():
        return float("nan"), float("nan")
    return pearson_restated(x, y), pearson_restated(ranks_restated(x), ranks_restated(y))
