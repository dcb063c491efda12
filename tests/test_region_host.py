"""Host side of the region pre-training step: the new C symbols are declared and bound, run_region_iter / train() call the model in
the reference's order (Pretrain.py:94-121, 211-243) without an optimizer step of their own, and the synthetic region batch has the
layout run_region_iter unpacks.  Runs without a GPU."""
import os
import re

import pytest
import torch

from xfm_amd import pretrain_loop as PL
from xfm_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("xfm_region_pool_fwd", "xfm_region_pool_bwd", "xfm_box_loss_fwd", "xfm_box_loss_bwd")


def test_region_symbols_are_declared_bound_and_wrapped():
    from xfm_amd import _lib, functional as Fx
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xfm_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/xfm_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(Fx, name[len("xfm_"):])
    assert _lib.ABI_VERSION >= 11
    lib = _lib.load()
    assert lib.xfm_region_pool_fwd(None, None, None, 1, 1, 1, 8, None, None, None) == -1 and b"null operand" in lib.xfm_last_error()
    assert lib.xfm_box_loss_fwd(None, None, None, 1, None, None, None) == -1 and b"null operand" in lib.xfm_last_error()


def test_fused_region_glue_refuses_cpu_tensors():
    """fused=True is the HIP path: no quiet fall-back to the ATen form on the CPU."""
    from xfm_amd import _lib
    from xfm_amd.xfm import XFMBase
    co = torch.tensor([[0.5, 0.5, 0.2, 0.2]])
    with pytest.raises(_lib.XfmHipError):
        XFMBase.get_bbox_loss(None, co, co, fused=True)
    l1, giou = XFMBase.get_bbox_loss(None, co, co)   # the ATen form stays for CPU tensors
    assert float(l1) == 0.0 and abs(float(giou)) < 1e-6


class _Model(torch.nn.Module):
    def __init__(self, log):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(()))
        self.log = log

    def forward(self, image, text_ids, text_atts, text_ids_masked=None, masked_pos=None, masked_ids=None, image_atts=None,
                idx_to_group_img=None, target_bbox=None, is_image=None, ret_match_loss=True, ret_mim_loss=True, ret_mlm_loss=True,
                ret_itc_loss=True, ret_bbox_loss=False, ret_bbox_giou=False, data_source=None):
        src = data_source if image is not None else "text"
        entry = ("fwd", src, ret_itc_loss, ret_match_loss, ret_mlm_loss, ret_mim_loss)
        if src == "region":
            entry += (ret_bbox_loss, ret_bbox_giou, is_image is None, tuple(idx_to_group_img.tolist()), tuple(image_atts.shape),
                      tuple(target_bbox.shape))
        self.log.append(entry)
        one = self.p * 0 + 1.0
        return {"loss_itc": one * 1, "loss_itm": one * 2, "loss_mlm": one * 3, "loss_mim": one * 4, "loss_bbox": one * 5, "loss_giou": one * 6}


class _Acc:
    def __init__(self, log):
        self.log = log

    def backward_step(self, loss, optimizer):
        self.log.append(("bwd", float(loss)))

    def optimizer_step(self, optimizer, model):
        self.log.append(("opt",))


def _batches(n, with_image=True):
    t = torch.zeros(2, 4, dtype=torch.long)
    for _ in range(n):
        yield ([torch.zeros(2, 3, 8, 8)] if with_image else []) + [t, t, t, t, t]


def _region_batches(n):
    t = torch.zeros(3, 4, dtype=torch.long)
    for _ in range(n):
        yield [torch.zeros(2, 3, 8, 8), torch.tensor([0, 0, 1]), t, t, t, t, t, torch.ones(3, 5, dtype=torch.long), torch.zeros(3, 4),
               torch.tensor([0, 1, 0])]


@pytest.mark.parametrize("calc_image_bbox_loss", [False, True])
def test_train_runs_text_then_region_then_image_without_a_region_optimizer_step(calc_image_bbox_loss):
    log = []
    m, acc = _Model(log), _Acc(log)
    opt = torch.optim.SGD([{"params": [m.p], "lr": 0.5}, {"params": [], "lr": 0.5}, {"params": [], "lr": 1.0}, {"params": [], "lr": 1.0}])
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    cfg = {"train_dataset_size": 100, "batch_size": 2, "stop_calc_itm": 2, "ckpt_frequent": 1, "ckpt_frequent_step": 10 ** 9,
           "ret_bbox_loss": True, "ret_bbox_giou": True, "calc_image_bbox_loss": calc_image_bbox_loss}
    out = PL.train(m, _batches(3), (None, None, None, _region_batches(3), _batches(3, with_image=False)), opt, (0, 1), "cpu", sch, cfg, acc,
                   print_freq=2)
    want = []
    for gs in range(1, 4):
        itm = gs < 2
        want += [("fwd", "text", True, True, True, True), ("bwd", 3.0), ("opt",)]
        # itc + itm + mlm + bbox + giou = 17 (MIM is not part of the region total), and no ("opt",) before the image iteration
        want += [("fwd", "region", True, itm, True, True, True, True, calc_image_bbox_loss, (0, 0, 1), (3, 5), (3, 4)), ("bwd", 17.0)]
        want += [("fwd", "image", True, itm, True, True), ("bwd", 10.0), ("opt",)]
    assert log == want
    for k, v in (("loss_ritc", 1), ("loss_ritm", 2), ("loss_rmlm", 3), ("loss_rbbox", 5), ("loss_rgiou", 6)):
        assert out[k] == "%.5f" % v, (k, out)
    assert "loss_rmim" not in out and out["loss_itc"] == "1.00000"


def test_run_region_iter_honours_the_config_flags():
    log = []
    m, acc = _Model(log), _Acc(log)
    meters = PL.LossMeters()
    cfg = {"ret_bbox_loss": True, "ret_bbox_giou": False, "calc_image_bbox_loss": False}
    PL.run_region_iter(m, next(_region_batches(1)), None, acc, meters, "cpu", cfg, ret_mim_loss=False)
    assert log[0][:8] == ("fwd", "region", True, True, True, False, True, False) and log[0][8] is False
    assert log[1:] == [("bwd", 17.0)]
    assert list(meters.global_avg()) == ["loss_ritc", "loss_ritm", "loss_rmlm", "loss_rbbox", "loss_rgiou"]


@pytest.mark.parametrize("bs,max_images,max_regions", [(96, 80, 5), (6, 4, 2), (10, 2, 5)])
def test_synthetic_region_batch_layout(bs, max_images, max_regions):
    res, patch = 64, 16
    t = syn.region_batch(bs, max_images, max_regions, seed=7, image_res=res, patch_size=patch)
    image, idx, text_ids, text_atts, text_ids_masked, masked_pos, masked_ids, image_atts, target_bbox, is_image = t
    n_img, P = image.shape[0], (res // patch) ** 2
    assert image.shape == (n_img, 3, res, res) and 1 <= n_img <= max_images
    assert idx.shape == (bs,) and idx.dtype == torch.long and int(idx.min()) == 0 and int(idx.max()) == n_img - 1
    assert torch.equal(idx, idx.sort().values) and int(torch.bincount(idx).max()) <= max_regions and int(torch.bincount(idx).min()) >= 1
    for x in (text_ids, text_atts, text_ids_masked):
        assert x.shape == (bs, 30)
    assert masked_pos.shape == masked_ids.shape == (bs, 15)
    assert image_atts.shape == (bs, 1 + P) and set(image_atts.unique().tolist()) <= {0, 1}
    assert bool((image_atts[:, 0] == 1).all()) and int(image_atts[:, 1:].sum(1).min()) >= 1
    assert target_bbox.shape == (bs, 4) and target_bbox.dtype == torch.float32
    x1, y1 = target_bbox[:, 0] - target_bbox[:, 2] / 2, target_bbox[:, 1] - target_bbox[:, 3] / 2
    x2, y2 = target_bbox[:, 0] + target_bbox[:, 2] / 2, target_bbox[:, 1] + target_bbox[:, 3] / 2
    assert bool((x1 >= -1e-6).all() and (y1 >= -1e-6).all() and (x2 <= 1 + 1e-6).all() and (y2 <= 1 + 1e-6).all())
    assert bool((target_bbox[:, 2:] > 0).all())
    assert is_image.shape == (bs,) and set(is_image.unique().tolist()) <= {0, 1} and int((1 - is_image).sum()) >= 1
    whole = is_image == 1
    assert bool((image_atts[whole] == 1).all()) and bool((target_bbox[whole] == torch.tensor([0.5, 0.5, 1.0, 1.0])).all())
    # the mask is the patch rectangle the box bounds
    g = res // patch
    area = (target_bbox[:, 2] * g).round() * (target_bbox[:, 3] * g).round()
    assert torch.equal(area.long(), image_atts[:, 1:].sum(1))


def test_regions_config_has_the_sections_the_launcher_reads():
    import yaml
    with open(os.path.join(ROOT, "configs", "Pretrain_synthetic_regions.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg["regions"]) >= {"batch_size", "max_images", "max_regions"}
    assert cfg["ret_bbox_loss"] is True and cfg["ret_bbox_giou"] is True and cfg["calc_image_bbox_loss"] is False
    with open(os.path.join(ROOT, "configs", "Pretrain_synthetic.yaml")) as f:
        base = yaml.safe_load(f)
    assert "regions" not in base
    assert {k: v for k, v in cfg.items() if k in base} == base


def test_asymmetric_box_flags_raise():
    """ret_bbox_giou without ret_bbox_loss: the reference has no image_embeds_fullatts there (a NameError); text_lens with the region
    step names what is missing.  Both are decided before any tower runs."""
    from xfm_amd.model_pretrain import XFM
    m = XFM.__new__(XFM)
    img = torch.zeros(1, 3, 8, 8)
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="ret_bbox_loss"):
        XFM.forward_multimodal(m, img, ids, ids, ret_bbox_giou=True)
    with pytest.raises(ValueError, match="image_atts"):
        XFM.forward_multimodal(m, img, ids, ids, ret_bbox_loss=True)
    with pytest.raises(NotImplementedError, match="text_lens"):
        XFM.forward_multimodal(m, img, ids, ids, ret_bbox_loss=True, ret_bbox_giou=True, image_atts=torch.ones(1, 2), idx_to_group_img=ids[:, 0],
                               text_lens=[4])
