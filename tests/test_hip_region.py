"""The region pre-training step on a real MI355X: the region pooling and box-loss kernels against float64 restatements, the step
against the fixture taken from the real reference (tests/golden/pretrain_region_small.npz: 6 samples over 4 images, ret_bbox_loss and
ret_bbox_giou set), its run-to-run reproducibility, and one train() iteration with a synthetic region loader.

Tolerances.  Pooling forward: the patch rows are copies (bit-equal); the pooled row is an fp32 sum of at most 196 bf16 values divided
once, so it is within one bf16 ulp of the rounded float64 value (a tie is the only way to differ at all).  Pooling backward: one bf16
rounding of the result (2^-8 relative) plus fp32 accumulation (2^-20 of the summed magnitudes, generous for <= 2 x 3 terms).  Box loss:
the kernel and the ATen form both deliver fp32; the kernel may be 4 x as far from the float64 value as the ATen fp32 form is, plus
1e-7.  Step: the tolerances of test_hip_modules._pretrain, 2e-2 absolute on the two box losses as the grounding tests use."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from test_hip_modules import _check_grads, _load_into, _pretrain_cfg  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

BF16 = torch.bfloat16
POOL_SHAPES = [(3, 5, 7, 768), (2, 4, 196, 768)]   # (n_img, bs, P, D)


def _pool_case(n_img, bs, P, D):
    """idx: in the first shape image 1 is read by nobody and image 0 by three samples.  Sample 0's mask is a single patch, sample 1's is
    all ones, the others are random with at least one patch."""
    idx = torch.tensor([0, 0, 2, 0, 2] if n_img == 3 else [1, 0, 1, 1], dtype=torch.int32)
    assert idx.numel() == bs
    tag = f"region_pool.{n_img}.{bs}.{P}"
    full = syn.symmetric(tag + ".full", (n_img, 1 + P, D), 2.0).to(BF16)
    atts = (syn.symmetric(tag + ".atts", (bs, P), 1.0) > 0.2).to(torch.uint8)
    atts[:, P // 2] = 1
    atts[0] = 0
    atts[0, P - 1] = 1
    atts[1] = 1
    dout = syn.symmetric(tag + ".dout", (bs, 1 + P, D), 1.0).to(BF16)
    return full, idx, atts, dout


def _bf16_ulp(ref):
    """Spacing of bf16 (8 significant bits) at the magnitude of `ref` (float64)."""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_region_pool_forward_vs_float64(shape):
    from xfm_amd import functional as Fx
    full, idx, atts, _ = _pool_case(*shape)
    out, wsum = Fx.region_pool_fwd(full.cuda(), idx.cuda(), atts.cuda())
    out, wsum = out.cpu(), wsum.cpu()
    gathered = full[idx.long()]
    assert torch.equal(out[:, 1:].view(torch.int16), gathered[:, 1:].view(torch.int16)), "patch rows must be copied bit for bit"
    w = atts.double()
    assert torch.equal(wsum.double(), w.sum(1))
    ref = torch.einsum("bp,bpd->bd", w, gathered[:, 1:].double()) / w.sum(1, keepdim=True)
    ref_bf = ref.to(BF16).double()
    err = (out[:, 0].double() - ref_bf).abs()
    ulp = _bf16_ulp(ref_bf)
    print(f"pooled row: {int((err > 0).sum())} of {err.numel()} entries differ from the rounded float64 value, worst {float((err / ulp).max()):.2f} ulp")
    assert bool((err <= ulp).all())


def _pool_bwd_reference(idx, atts, dout, n_img):
    bs, N, D = dout.shape
    d, w = dout.double(), atts.double()
    coef = w / w.sum(1, keepdim=True)                                # [bs, P]
    term = d[:, 1:] + coef[:, :, None] * d[:, :1]                    # [bs, P, D]
    mag = d[:, 1:].abs() + coef[:, :, None] * d[:, :1].abs()
    ref, tot = torch.zeros(n_img, N, D, dtype=torch.float64), torch.zeros(n_img, N, D, dtype=torch.float64)
    for s in range(bs):
        ref[int(idx[s]), 1:] += term[s]
        tot[int(idx[s]), 1:] += mag[s]
    return ref, tot


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_region_pool_backward_vs_float64_and_bit_reproducible(shape, monkeypatch):
    from xfm_amd import functional as Fx
    full, idx, atts, dout = _pool_case(*shape)
    n_img = shape[0]
    g = [t.cuda() for t in (full, idx, atts, dout)]
    _, wsum = Fx.region_pool_fwd(g[0], g[1], g[2])
    monkeypatch.setenv("XFM_DETERMINISTIC", "0")
    a = Fx.region_pool_bwd(g[3], g[1], g[2], wsum, n_img).cpu()
    b = Fx.region_pool_bwd(g[3], g[1], g[2], wsum, n_img).cpu()
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    c = Fx.region_pool_bwd(g[3], g[1], g[2], wsum, n_img).cpu()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two runs differ"
    assert torch.equal(a.view(torch.int16), c.view(torch.int16)), "XFM_DETERMINISTIC changes the result"
    ref, tot = _pool_bwd_reference(idx, atts, dout, n_img)
    err = (a.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * tot
    print(f"dfull: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert float(a[:, 0].abs().max()) == 0.0, "the tower's own pooled row is not read: no gradient"
    if n_img == 3:
        assert float(a[1].abs().max()) == 0.0, "an image that no sample reads gets zeros"
    assert float(a[0, 1:].abs().max()) > 0.0


def test_region_outputs_autograd_matches_the_aten_form_and_is_reproducible(monkeypatch):
    """beit2.region_outputs on HIP tensors (the kernels behind an autograd function) against its own ATen form on the CPU, and the
    gradient w.r.t. the tower output bit-equal between two runs -- three samples share image 0."""
    from xfm_amd import beit2
    full, idx, atts, dout = _pool_case(*POOL_SHAPES[0])
    image_atts = torch.cat([torch.ones(atts.shape[0], 1, dtype=torch.long), atts.long()], dim=1)
    grads = []
    for _ in range(2):
        x = full.cuda().requires_grad_(True)
        y = beit2.region_outputs(x, idx.long().cuda(), image_atts.cuda())
        y.backward(dout.cuda())
        grads.append(x.grad.cpu())
    assert torch.equal(grads[0].view(torch.int16), grads[1].view(torch.int16))
    xc = full.float().requires_grad_(True)
    yc = beit2.region_outputs(xc, idx.long(), image_atts)
    yc.backward(dout.float())
    assert float((y.detach().cpu().float() - yc.detach()).abs().max()) <= 2.0 ** -7 * float(yc.detach().abs().max())
    assert float((grads[0].float() - xc.grad).abs().max()) <= 2.0 ** -7 * float(xc.grad.abs().max())


# ---- box loss -------------------------------------------------------------------------------------------------------------------------
def _aten_box_loss(coord, target, is_image=None):
    """XFMBase.get_bbox_loss as it stands, without its casts to fp32: the same ops in the dtype of the inputs."""
    import torch.nn.functional as F
    from xfm_amd import box_ops
    loss_bbox = F.l1_loss(coord, target, reduction='none')
    boxes1, boxes2 = box_ops.box_cxcywh_to_xyxy(coord), box_ops.box_cxcywh_to_xyxy(target)
    degenerate = (boxes1[:, 2:] < boxes1[:, :2]).any() | (boxes2[:, 2:] < boxes2[:, :2]).any()
    unit = torch.tensor([0.0, 0.0, 1.0, 1.0], device=boxes1.device, dtype=coord.dtype).expand_as(boxes1)
    giou = box_ops.paired_generalized_box_iou(torch.where(degenerate, unit, boxes1), torch.where(degenerate, unit, boxes2))
    loss_giou = torch.where(degenerate, torch.zeros_like(giou), 1 - giou)
    if is_image is None:
        num_boxes = target.size(0)
    else:
        num_boxes = torch.sum(1 - is_image)
        loss_bbox = loss_bbox * (1 - is_image.view(-1, 1))
        loss_giou = loss_giou * (1 - is_image)
    return loss_bbox.sum() / num_boxes, loss_giou.sum() / num_boxes


def _boxes(bs, tag):
    u = syn.uniform01(f"box_loss.{tag}.{bs}", bs * 8).reshape(bs, 8)
    def box(v):
        return torch.from_numpy(np.stack([0.3 + 0.4 * v[:, 0], 0.3 + 0.4 * v[:, 1], 0.1 + 0.4 * v[:, 2], 0.1 + 0.4 * v[:, 3]], 1).astype(np.float32))
    return box(u[:, :4]), box(u[:, 4:])


def _is_image(bs, kind):
    if kind == "none":
        return None
    if kind == "single":   # every row but one is a whole-image sample: a single box is left
        m = torch.ones(bs)
        m[bs // 2] = 0
        return m
    m = (torch.from_numpy(syn.uniform01(f"box_loss.is_image.{bs}", bs)) < 0.4).float()
    m[0] = 0
    return m


BOX_CASES = [(bs, kind, False) for bs in (1, 6, 300) for kind in ("none", "some", "single")] + [(6, "none", True), (6, "some", True)]


@pytest.mark.parametrize("bs,kind,degenerate", BOX_CASES)
def test_box_loss_kernels_vs_aten_float64(bs, kind, degenerate):
    from xfm_amd.xfm import XFMBase
    coord, target = _boxes(bs, kind)
    if degenerate:
        target[bs // 2, 2] = -0.2   # negative width: x2 < x1
    is_image = _is_image(bs, kind)

    def run(fn, c, t, m):
        c = c.clone().requires_grad_(True)
        l1, giou = fn(c, t, m)
        (l1 + giou).backward()
        return l1.detach().double().cpu(), giou.detach().double().cpu(), c.grad.double().cpu()

    ref = run(_aten_box_loss, coord.double(), target.double(), None if is_image is None else is_image.double())
    aten = run(_aten_box_loss, coord, target, is_image)
    own = run(lambda c, t, m: XFMBase.get_bbox_loss(None, c, t, m), coord, target, is_image)
    assert all(torch.equal(a, b) for a, b in zip(aten, own)), "the restated ATen form is not get_bbox_loss"
    got = run(lambda c, t, m: XFMBase.get_bbox_loss(None, c, t, m, fused=True), coord.cuda(), target.cuda(),
              None if is_image is None else is_image.cuda())
    report = {}
    for name, r, a, k in zip(("loss_bbox", "loss_giou", "dcoord"), ref, aten, got):
        e_aten, e_kernel = float((a - r).abs().max()), float((k - r).abs().max())
        report[name] = (e_kernel, e_aten)
    print(json.dumps(report))
    for name, (e_kernel, e_aten) in report.items():
        assert math.isfinite(e_kernel) and e_kernel <= 4.0 * e_aten + 1e-7, (name, report)
    if degenerate:
        assert float(got[1]) == 0.0 and float(ref[1]) == 0.0
        c = coord.cuda().requires_grad_(True)
        XFMBase.get_bbox_loss(None, c, target.cuda(), None if is_image is None else is_image.cuda(), fused=True)[1].backward()
        assert float(c.grad.abs().max()) == 0.0, "the degenerate rule leaves no GIoU gradient"


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
def _region_inputs(meta):
    hb = syn.pretrain_batch(meta["bs"], seed=meta["seed"])
    idx, atts = syn.region_case(meta["n_images"])
    assert idx.tolist() == meta["idx"]
    b = {k: v.cuda() for k, v in hb.items()}
    b["image"] = b["image"][:meta["n_images"]]
    kw = dict(text_ids_masked=b["text_ids_masked"], masked_pos=b["masked_pos"], masked_ids=b["masked_ids"], image_atts=atts.cuda(),
              idx_to_group_img=idx.cuda(), target_bbox=torch.tensor(meta["target"]).cuda(), is_image=torch.tensor(meta["is_image"]).cuda(),
              ret_mim_loss=True, ret_bbox_loss=True, ret_bbox_giou=True, data_source="region",
              neg_idx=(meta["image_neg_idx"], meta["text_neg_idx"]))
    return b, kw


def _region_model(meta, batch_passes):
    from xfm_amd.model_pretrain import XFM
    m = XFM(dict(_pretrain_cfg(meta), batch_passes=batch_passes))
    ours = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()}
    assert ours == meta["spec"]
    _load_into(m, meta["spec"])
    m.cuda().finalize().eval()
    return m


LOSSES = ("loss_itc", "loss_itm", "loss_mlm", "loss_bbox", "loss_giou")


@pytest.mark.parametrize("batch_passes", [True, False])
def test_pretrain_region_step_vs_golden(batch_passes):
    z, meta = load("pretrain_region_small")
    m = _region_model(meta, batch_passes)
    b, kw = _region_inputs(meta)
    losses = m(b["image"], b["text_ids"], b["text_atts"], **kw)
    report = {k: (float(losses[k]), float(z[k])) for k in LOSSES}
    print(json.dumps(report))
    ltol = {"loss_itc": 3e-3, "loss_itm": 3e-2, "loss_mlm": 3e-3}   # as test_hip_modules._pretrain
    for k in ("loss_itc", "loss_itm", "loss_mlm"):
        got, ref = report[k]
        assert abs(got - ref) <= ltol[k] * max(abs(ref), 1.0), report
    for k in ("loss_bbox", "loss_giou"):
        got, ref = report[k]
        assert abs(got - ref) <= 2e-2, report
    assert float(losses["loss_mim"]) == 0.0
    sum(losses[k] for k in LOSSES).backward()
    _check_grads(z, "grad", m, min_rms=1e-6)
    unused = set(meta["unused"])
    assert unused
    for n, p in m.named_parameters():
        if n in unused:
            assert float(p._xfm_grad.abs().max()) == 0.0, f"{n} must receive no gradient"


def test_pretrain_region_step_is_bit_reproducible_under_deterministic_mode(monkeypatch):
    """Two fresh models, the same region batch (images shared by up to two samples): bit-equal vision-tower gradients."""
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    z, meta = load("pretrain_region_small")
    runs = []
    for _ in range(2):
        m = _region_model(meta, True)
        b, kw = _region_inputs(meta)
        losses = m(b["image"], b["text_ids"], b["text_atts"], **kw)
        sum(losses[k] for k in LOSSES).backward()
        torch.cuda.synchronize()
        runs.append({n: p.grad.detach().clone() for n, p in m.vision_encoder.named_parameters() if p.grad is not None})
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) > 100
    differ = [n for n in runs[0] if not torch.equal(runs[0][n], runs[1][n])]
    assert not differ, differ[:8]
    assert any(float(g.abs().max()) > 0 for g in runs[0].values())


def test_region_step_rejects_what_it_cannot_run():
    z, meta = load("pretrain_region_small")
    m = _region_model(meta, True)
    b, kw = _region_inputs(meta)
    with pytest.raises(NotImplementedError, match="text_lens"):
        m(b["image"], b["text_ids"], b["text_atts"], text_lens=[30] * meta["bs"], **kw)
    with pytest.raises(ValueError, match="ret_bbox_loss"):
        m(b["image"], b["text_ids"], b["text_atts"], **dict(kw, ret_bbox_loss=False))


def test_train_iteration_with_a_synthetic_region_loader():
    """Pretrain.py's loaders on a small model: text-free iteration = region batch (no optimizer step) then image batch (steps)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import Pretrain
    from xfm_amd import pretrain_loop as PL
    from xfm_amd.accelerators import RCCLDDPAccelerator
    from xfm_amd.model_pretrain import XFM
    vocab = 2048
    cfg = {"use_beit_v2": True, "image_res": 224, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": 1, "text_fusion_start_at": 1, "fusion_num_hidden_layers": 1, "fusion_fusion_start_at": 0,
           "embed_dim": 256, "temp": 0.07, "vision_depth": 1, "text_config": {"vocab_size": vocab},
           "train_dataset_size": 8, "batch_size": 4, "ckpt_frequent": 10 ** 6, "ckpt_frequent_step": 10 ** 9,
           "regions": {"batch_size": 6, "max_images": 4, "max_regions": 2}, "ret_bbox_loss": True, "ret_bbox_giou": True,
           "calc_image_bbox_loss": False}
    m = XFM(cfg)
    m.load_state_dict(syn.formula_state_dict(m.state_dict()), strict=True)
    m.cuda()
    opt = PL.create_optimizer(PL.AttrDict(lr=1e-4, weight_decay=0.01, lr_mult=2), m)
    sch = PL.create_scheduler(PL.AttrDict(sched="linear", num_warmup_steps=1, epochs=1, step_per_epoch=2), opt)
    acc = RCCLDDPAccelerator({"RNG_SEED": 3, "CLIP_GRAD_NORM": 1.0, "GRAD_ACCUMULATE_STEPS": 1})
    wrapped, opt, sch = acc.set_up(m, opt, sch, 0, 1, 0)
    images = Pretrain.SyntheticLoader(1, 4, seed=5, vocab=vocab)
    regions = Pretrain.SyntheticRegionLoader(1, cfg["regions"], seed=6, vocab=vocab)
    out = PL.train(wrapped, images, (None, None, None, regions, None), opt, (0, 1), torch.device("cuda"), sch, cfg, acc, print_freq=1)
    torch.cuda.synchronize()
    for k in ("loss_ritc", "loss_ritm", "loss_rmlm", "loss_rbbox", "loss_rgiou", "loss_itc", "loss_mlm"):
        assert k in out and math.isfinite(float(out[k])), (k, out)
    assert float(out["loss_rbbox"]) > 0 and float(out["loss_rgiou"]) > 0


def test_pretrain_script_main_trains_checkpoints_and_resumes(tmp_path, capsys):
    """Pretrain.py's main() as `run.py --task pretrain` starts it, at the one-layer shape above with all three synthetic sources (text,
    region, image): one epoch of two steps, the epoch checkpoint, log.txt and config.yaml; then a second main() that resumes from that
    checkpoint with `epochs: 2` and trains exactly the remaining epoch."""
    import copy
    import os
    from types import SimpleNamespace as NS

    import yaml

    import Pretrain as script
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "Pretrain_synthetic_regions.yaml")) as f:
        shipped = yaml.safe_load(f)
    cfg = {"use_beit_v2": True, "image_res": 224, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": 1, "text_fusion_start_at": 1, "fusion_num_hidden_layers": 1, "fusion_fusion_start_at": 0,
           "embed_dim": 256, "temp": 0.07, "vision_depth": 1, "text_config": {"vocab_size": 2048},
           "images": {"batch_size": 4}, "train_dataset_size": 8, "synthetic": True, "synthetic_text_source": True,
           "regions": {"batch_size": 6, "max_images": 4, "max_regions": 2}, "ret_bbox_loss": True, "ret_bbox_giou": True,
           "calc_image_bbox_loss": False, "ckpt_frequent": 1, "ckpt_frequent_step": 10 ** 9, "print_freq": 1,
           "optimizer": dict(shipped["optimizer"]), "schedular": dict(shipped["schedular"], epochs=1),
           "accelerator": dict(shipped["accelerator"])}
    out = tmp_path / "pretrain"
    out.mkdir()
    args = NS(checkpoint="", bs=-1, epoch=-1, seed=42, output_dir=str(out))
    script.main(args, copy.deepcopy(cfg))
    steps = [json.loads(l)["step"] for l in capsys.readouterr().out.splitlines() if l.startswith('{"step"')]
    assert steps == [1, 2]
    assert (out / "model_state_epoch_0.th").exists() and (out / "training_state_latest.th").exists()
    assert yaml.safe_load((out / "config.yaml").read_text())["batch_size"] == 4
    lines = (out / "log.txt").read_text().splitlines()
    assert len(lines) == 1
    stats = json.loads(lines[0])
    for k in ("train_loss_tmlm", "train_loss_ritc", "train_loss_rbbox", "train_loss_itc", "train_loss_mlm"):
        assert math.isfinite(float(stats[k])), (k, stats)
    assert stats["epochs"] == 1
    # resume: the optimizer, the schedule and the epoch counter from the epoch checkpoint, the weights through load_pretrained
    args.checkpoint = str(out / "model_state_epoch_0.th")
    again = copy.deepcopy(cfg)
    again["resume"] = True
    again["schedular"]["epochs"] = 2
    script.main(args, again)
    steps = [json.loads(l)["step"] for l in capsys.readouterr().out.splitlines() if l.startswith('{"step"')]
    assert steps == [3, 4]   # the remaining epoch and nothing else
    assert (out / "model_state_epoch_1.th").exists()
    assert torch.load(out / "training_state_latest.th", weights_only=False)["epoch"] == 1
    lines = (out / "log.txt").read_text().splitlines()
    assert len(lines) == 2 and json.loads(lines[1])["epochs"] == 2
