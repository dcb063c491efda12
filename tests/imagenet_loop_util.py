"""Shared helpers of the ImageNet-loop tests (test infrastructure): the fixture's configuration, its batches, and the CPU model path --
the oracle's classification forward behind an nn.Module with the reference's call form."""
import torch

from golden_util import load, state_from_spec
from oracle import xfm_oracle as O
from xfm_amd import synthetic as syn


def fixture():
    return load("imagenet_loop_small")


def loop_config(meta, is_lp, **kw):
    cfg = {"use_beit_v2": True, "image_res": 224, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": meta["text_layers"], "text_fusion_start_at": meta["text_layers"],
           "fusion_num_hidden_layers": meta["fusion_layers"], "fusion_fusion_start_at": 0, "embed_dim": 256, "temp": 0.07,
           "learnable_temp": True, "max_temp": 0.5, "min_temp": 0.001, "vision_depth": meta["vit_depth"],
           "task_name": "imagenet", "num_labels": meta["num_labels"], "is_lp": is_lp, "smoothing": meta["smoothing"],
           "mixup": 0.0, "cutmix": 0.0, "cutmix_minmax": None, "mixup_prob": 1.0, "mixup_switch_prob": 0.5, "mixup_mode": "batch",
           "schedular": dict(meta["schedular"]), "optimizer": dict(meta["optimizer"])}
    cfg.update(kw)
    return cfg


def train_batches(meta):
    return [syn.imagenet_batch(meta["B"], seed=s, num_labels=meta["num_labels"]) for s in meta["train_seeds"]]


def eval_batch(meta):
    return syn.imagenet_batch(meta["eval_B"], seed=meta["eval_seed"], num_labels=meta["num_labels"])


def used_state(spec):
    """Formula weights of the entries the image-only branch reads (the text towers' 160 M unused elements are not generated)."""
    return state_from_spec({k: v for k, v in spec.items() if k.startswith(("vision_encoder.", "cls_head."))})


class OracleClassifier(torch.nn.Module):
    """XFMForClassification's image-only branch on the CPU: oracle arithmetic, the reference's forward(image, None, None, None, False)."""

    def __init__(self, state, vit_depth, is_lp=False):
        super().__init__()
        self.names = list(state)
        self.cfg = O.default_cfg(vit_depth=vit_depth)
        self.is_lp = is_lp
        for i, k in enumerate(self.names):
            v = state[k]
            if v.dtype.is_floating_point:
                self.register_parameter(f"p{i}", torch.nn.Parameter(v.clone()))
            else:
                self.register_buffer(f"p{i}", v.clone())

    def table(self):
        return {k: getattr(self, f"p{i}") for i, k in enumerate(self.names)}

    def forward(self, image, text_ids, text_atts, targets, train=True):
        assert text_ids is None and train is False
        P = self.table()
        if self.is_lp:   # model_classification.py:64-74: the tower under no_grad
            P = {k: (v.detach() if k.startswith("vision_encoder.") else v) for k, v in P.items()}
        return O.classification_forward(P, self.cfg, image, None, None, deep_head=True)
