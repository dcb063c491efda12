"""Host side of the ImageNet fine-tune / linear-probe loop (xfm_amd.imagenet_loop) without a GPU: the schedule, the loop on the CPU model
path (oracle forward, torch.optim.AdamW stepping) against tests/golden/imagenet_loop_small.npz -- the REFERENCE's loop, see
tools/oracle/gen_golden.py::gen_imagenet_loop -- the factories, accuracy, the launcher's command line and the best-checkpoint save.

Parameter probes after the steps are NOT compared across implementations: Adam's first updates are sign-like, a 1e-7 gradient difference
on a near-zero entry flips a full lr.  The loss trajectory carries the update instead."""
import os

import numpy as np
import pytest
import torch
import yaml

from imagenet_loop_util import OracleClassifier, eval_batch, fixture, loop_config, train_batches, used_state
from xfm_amd import imagenet_loop as IL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, ref, rms=None):
    """tests/test_oracle_golden.py's rule (golden_util.check): |err| <= 2e-5 + 2e-4 * rms of the reference."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt((ref * ref).mean())) if rms is None else rms
    err = float(np.abs(got - ref).max())
    assert err <= 2e-5 + 2e-4 * rms, (err, rms, got, ref)


class _Opt:
    def __init__(self, groups):
        self.param_groups = groups


def test_schedule_matches_the_reference_value_for_value():
    z, meta = fixture()
    cfg = loop_config(meta, False)
    opt = _Opt([{"lr": -1.0}, {"lr": -1.0, "lr_scale": 0.25}])
    got = []
    for epoch in range(2):
        for i in range(2):
            lr = IL.adjust_learning_rate(opt, i / 2 + epoch, cfg)
            assert opt.param_groups[0]["lr"] == lr and opt.param_groups[1]["lr"] == lr * 0.25
            got.append(lr)
    ref = z["ft/lr"]
    assert ref.dtype == np.float64 and len(ref) == 4
    assert np.allclose(np.asarray(got), ref, rtol=1e-12, atol=0.0)
    assert got[0] == 0.0 and got[1] == 0.5e-3 and got[2] == 1e-3 and 1e-5 < got[3] < 1e-3   # warm-up, warm-up, peak, cosine
    assert np.array_equal(z["lp/lr"], ref)
    assert IL.adjust_learning_rate(opt, 2.0, cfg) == pytest.approx(1e-5, rel=1e-12)   # the end of the half cycle: min_lr


@pytest.fixture(scope="module")
def state():
    z, meta = fixture()
    return z, meta, used_state(meta["spec"])


class _CpuAccelerator:
    """backward / step as the accelerator does them without an arena (RCCLDDPAccelerator.optimizer_step, `arena is None`)."""

    def backward_step(self, loss, optimizer):
        loss.backward()

    def optimizer_step(self, optimizer, model):
        optimizer.step()
        optimizer.zero_grad()


def _criterion(s):
    return lambda x, t: torch.nn.functional.cross_entropy(x, t, label_smoothing=s)


@pytest.mark.parametrize("is_lp", [False, True])
def test_loop_on_the_cpu_model_path_reproduces_the_reference(state, is_lp):
    z, meta, sd = state
    pre = "lp" if is_lp else "ft"
    cfg = loop_config(meta, is_lp)
    model = OracleClassifier(sd, meta["vit_depth"], is_lp)
    opt = IL.create_optimizer(cfg, model)
    assert IL.create_mixup(cfg) is None
    losses = []

    class Rec(_CpuAccelerator):
        def backward_step(self, loss, optimizer):
            losses.append(float(loss.detach()))
            super().backward_step(loss, optimizer)

    lrs = []
    orig = IL.adjust_learning_rate

    loader = train_batches(meta)
    for epoch in range(cfg["schedular"]["epochs"]):
        avg = IL.train_one_epoch(model, loader, opt, _criterion(meta["smoothing"]), epoch, None, "cpu", cfg, Rec())
        lrs.append(opt.param_groups[0]["lr"])
        assert avg["loss"] == pytest.approx(np.mean(losses[-2:]), rel=1e-6)
    assert orig is IL.adjust_learning_rate
    print(pre, "losses", losses, "reference", z[f"{pre}/loss"].tolist())
    _close(losses, z[f"{pre}/loss"])
    assert lrs == [z[f"{pre}/lr"][1], z[f"{pre}/lr"][3]]
    if is_lp:   # torch skips `grad is None`: the tower is in the optimizer and was never touched, decay included
        P = model.table()
        stepped = {k for k, p in P.items() if isinstance(p, torch.nn.Parameter) and p in opt.state}
        assert stepped == set(meta["stepped_lp"]) and all(k.startswith("cls_head.") for k in stepped)
        assert all(torch.equal(P[k].detach(), sd[k]) for k in P if k.startswith("vision_encoder."))
    images, target = eval_batch(meta)
    assert target.tolist() == meta["eval_target"]
    res = IL.evaluate(model, [(images[:4], target[:4]), (images[4:], target[4:])], "cpu", log=lambda m: None)
    with torch.no_grad():
        logits = model(images, None, None, None, False)
    _close(logits.numpy(), z[f"{pre}/eval_logits"])
    _close(res.loss_avg, float(z[f"{pre}/eval_loss"]))
    # the fixture's evaluation batch has no near-tie (margin recorded by the generator): the accuracies are exact
    assert meta["eval_margin"] > 1e-3
    ref1, ref2 = (float(v) for v in z[f"{pre}/acc"])
    assert round(res.acc1 * meta["eval_B"] / 100.0) == round(ref1 * meta["eval_B"] / 100.0)
    assert round(res.acc2 * meta["eval_B"] / 100.0) == round(ref2 * meta["eval_B"] / 100.0)
    assert float(res) == res.acc1 and res.count == meta["eval_B"]
    a1, a2 = IL.accuracy(logits, target, topk=(1, 2))
    assert float(a1) == np.float32(ref1) and float(a2) == np.float32(ref2)   # the reference's own float32 figures, bit for bit


def test_factories():
    z, meta = fixture()
    lin = torch.nn.Linear(3, 2)
    frozen = torch.nn.Linear(2, 2)
    frozen.weight.requires_grad_(False)
    model = torch.nn.Sequential(lin, frozen)
    cfg = loop_config(meta, False)
    cfg["optimizer"] = {"opt": "adamW", "lr": 4e-5, "weight_decay": 0.02, "momentum": 0.9}
    opt = IL.create_optimizer(cfg, model)
    assert type(opt) is torch.optim.AdamW and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert g["lr"] == 4e-5 and g["weight_decay"] == 0.01 and tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8 and not g["amsgrad"]
    assert len(g["params"]) == 3 and all(p.requires_grad for p in g["params"])   # Imagenet.py:566: requires_grad parameters only
    assert opt.defaults["adamw_rule"] == "torch" and g["adamw_rule"] == "torch"
    from xfm_amd.accelerators.rccl_ddp_accelerator import adamw_rule
    assert adamw_rule(opt) == "torch"
    assert adamw_rule(torch.optim.AdamW(lin.parameters(), lr=1e-3)) == "transformers"   # no marker: the rule of optim.py's optimizer
    opt.load_state_dict(opt.state_dict())   # the marker survives torch's own round trip
    assert adamw_rule(opt) == "torch"
    for name in ("lars", "sgd"):
        with pytest.raises(NotImplementedError, match="Imagenet.py:5"):
            IL.create_optimizer(dict(cfg, optimizer=dict(cfg["optimizer"], opt=name)), model)
    # criteria by the reference's conditions (Imagenet.py:605-611)
    from xfm_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    from xfm_amd.mixup import Mixup
    mix_cfg = dict(cfg, mixup=0.8, cutmix=1.0)
    mix = IL.create_mixup(mix_cfg)
    assert isinstance(mix, Mixup) and mix.mixup_alpha == 0.8 and mix.cutmix_alpha == 1.0 and mix.num_classes == meta["num_labels"]
    assert mix.label_smoothing == meta["smoothing"] and mix.mode == "batch"
    assert isinstance(IL.create_criterion(mix_cfg, mix), SoftTargetCrossEntropy)
    c = IL.create_criterion(cfg, None)
    assert isinstance(c, LabelSmoothingCrossEntropy) and c.smoothing == meta["smoothing"]
    assert type(IL.create_criterion(dict(cfg, smoothing=0.0), None)) is torch.nn.CrossEntropyLoss
    assert IL.create_mixup(dict(mix_cfg, is_lp=True)) is None                      # a linear probe disables Mixup ...
    assert isinstance(IL.create_criterion(dict(mix_cfg, is_lp=True), None), LabelSmoothingCrossEntropy)   # ... and falls to smoothing
    assert isinstance(IL.create_mixup(dict(cfg, cutmix=1.0)), Mixup)
    for name in ("Imagenet_synthetic.yaml", "Imagenet_synthetic_lp.yaml"):         # the shipped configs carry every key the loop reads
        with open(os.path.join(ROOT, "configs", name)) as f:
            y = yaml.safe_load(f)
        assert (IL.create_mixup(y) is None) == bool(y.get("is_lp", False))
        assert y["optimizer"]["opt"] == "adamW" and {"lr", "min_lr", "epochs", "warmup_epochs"} <= set(y["schedular"])


def test_accuracy_hand_worked():
    out = torch.tensor([[0.1, 0.9, 0.3, 0.2, 0.0],    # label 1: first
                        [2.0, 0.5, 1.5, 0.1, 0.3],    # label 2: second, 0.5 behind the first and 1.0 ahead of the third
                        [0.0, 0.1, 0.2, 0.3, 4.0],    # label 0: last
                        [1.0, 3.0, 2.0, 0.0, 0.5]])   # label 0: third
    target = torch.tensor([1, 2, 0, 0])
    a1, a2, a3 = IL.accuracy(out, target, topk=(1, 2, 3))
    assert a1.shape == (1,) and a1.item() == 25.0 and a2.item() == 50.0 and a3.item() == 75.0
    (only,) = IL.accuracy(out, target)
    assert only.item() == 25.0
    acc = torch.zeros(3)
    IL._topk_sums(out, target, 1, 2, acc)
    assert acc[1:].tolist() == [1.0, 2.0]
    assert acc[0].item() == pytest.approx(float(torch.nn.functional.cross_entropy(out, target, reduction="sum")), rel=1e-6)


def test_launcher_command_line():
    import run as R
    a = R.parse(["--task", "imagenet", "--dist", "gpu0", "--output_dir", "out/in", "--bs", "64", "--epoch", "3"])
    cmd, nproc, vis, sa = R.task_command(a, 8)
    assert (nproc, vis) == (1, "0")
    assert any(str(c).endswith("Imagenet.py") for c in cmd)
    assert "--bs" not in sa and "--epoch" not in sa and "--checkpoint" not in sa           # run.py:284-287 of the reference
    assert sa[sa.index("--config") + 1].endswith("configs/Imagenet_synthetic.yaml")
    assert sa[sa.index("--output_dir") + 1] == "out/in" and sa[sa.index("--seed") + 1] == 42
    a.checkpoint = "ckpt.th"
    sa = R.task_command(a, 8)[3]
    assert sa[sa.index("--checkpoint") + 1] == "ckpt.th"
    a.task = "coco_captioning"
    with pytest.raises(NotImplementedError):
        R.task_command(a, 8)
    import Imagenet as script
    with pytest.raises(NotImplementedError, match="file-backed"):
        script.synthetic_loaders({"synthetic": False}, 0)


def test_two_epoch_run_of_the_synthetic_config_writes_the_best_checkpoint(state, tmp_path):
    import Imagenet as script
    z, meta, sd = state
    with open(os.path.join(ROOT, "configs", "Imagenet_synthetic_lp.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["schedular"]["epochs"] == 2 and cfg["is_lp"]
    # the config's keys at a size the CPU model path runs in seconds: the fixture's shallow tower and label count, 2 x 4 training images
    cfg.update(num_labels=meta["num_labels"], batch_size_train=4, batch_size_test=8, train_dataset_size=8, val_dataset_size=32)
    # the reference saves when acc1 > best_acc1 with best_acc1 = 0 (Imagenet.py:614-625), and two epochs do not teach a frozen random tower
    # anything: take the first seed whose validation labels cover every class, so that even a constant prediction scores
    from xfm_amd import synthetic as syn
    seed = next(s for s in range(42, 400) if len({int(v) for k in range(4) for v in
                                                  syn.imagenet_batch(8, seed=s + 104729 + 7919 * k, image_res=16, num_labels=meta["num_labels"])[1]})
                == meta["num_labels"])
    train_loader, val_loader = script.synthetic_loaders(cfg, seed=seed)
    assert len(train_loader) == 2 and len(val_loader) == 4
    images, labels = next(iter(train_loader))
    assert images.shape == (4, 3, 224, 224) and labels.dtype == torch.int64 and 0 <= int(labels.min()) and int(labels.max()) < meta["num_labels"]
    model = OracleClassifier(sd, meta["vit_depth"], is_lp=True)
    opt = IL.create_optimizer(cfg, model)
    best, best_epoch = IL.train(model, train_loader, val_loader, opt, _criterion(cfg["smoothing"]), IL.create_mixup(cfg), "cpu", cfg,
                                _CpuAccelerator(), str(tmp_path))
    assert best > 0.0
    ckpt = torch.load(os.path.join(tmp_path, "checkpoint_best.pth"), weights_only=False)
    assert sorted(ckpt) == ["config", "epoch", "model", "optimizer"]
    assert ckpt["epoch"] == best_epoch and ckpt["config"]["is_lp"] and len(ckpt["optimizer"]["state"]) == len(meta["stepped_lp"])
    assert ckpt["optimizer"]["param_groups"][0]["adamw_rule"] == "torch"


def test_abi_and_new_symbols():
    """The two entry points of this loop exist at the ABI that introduced them (12 was taken by xfm_gemm_tn_plan; they are ABI 13)."""
    from xfm_amd import _lib
    assert _lib.ABI_VERSION >= 13
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    for name in ("xfm_adamw_torch", "xfm_ce_topk_eval"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    # argument errors come back as XFM_E_ARG before anything is launched (host-only checks: dummy non-NULL pointers are not read)
    P = 0x10000
    for bad in (dict(k1=0), dict(k2=1, k1=2), dict(k2=11), dict(ld=9), dict(R=0)):
        kw = dict(ld=10, R=2, V=10, k1=1, k2=2)
        kw.update(bad)
        rc = lib.xfm_ce_topk_eval(P, kw["ld"], kw["R"], kw["V"], P, kw["k1"], kw["k2"], None, None, P, None)
        assert rc == -1 and b"ce_topk_eval" in lib.xfm_last_error(), bad
    assert lib.xfm_ce_topk_eval(None, 10, 2, 10, P, 1, 2, None, None, P, None) == -1
    assert lib.xfm_adamw_torch(None, None) == -1
