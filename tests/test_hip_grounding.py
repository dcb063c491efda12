"""The grounding evaluation kernel, the fused loss on the task model and the loop on a real MI355X: xfm_box_eval against the fp64
restatement in tests/grounding_loop_util.py, XFMForGrounding(fused=True) against tests/golden/grounding_small.npz, and
xfm_amd.grounding_loop / Grounding_bbox.main against the reference's loop (tests/golden/grounding_loop_small.npz).
In the kernel tests every operand lies at an unaligned offset inside a larger poisoned buffer, and everything outside the documented
outputs must still hold the poison afterwards.

Tolerances:
  IoU     |IoU - IoU64| <= 2^-23.  A single rounding to fp32 of a value in [0, 1] is at most 2^-25; the rest is room for a contracted
          multiply-add in the fp64 part crossing an fp32 rounding boundary.
  pixels  the four pixel values within one fp32 rounding of the fp64 ones: |x - x64| <= 2^-24 |x64|.
  counts  EQUAL.  grounding_loop_util.box_case asserts that every sample but the constructed threshold one has |IoU64 - 0.5| > 2^-20, so
          only that one sits on the line, and there every step is exact in binary.
  model   the bounds of tests/test_hip_modules.py::test_grounding_model_vs_golden, unchanged: coords < 1e-2, both losses < 2e-2 absolute,
          _check_grads.  The fixture's flags clear a +-1e-2 move of every coordinate (the margin condition, re-asserted in
          tests/test_grounding_loop_host.py), so flags, counts and accuracies are compared for EQUALITY."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, state_from_spec  # noqa: E402
from grounding_loop_util import (BOX_EVAL_N, box_case, box_eval_digests, box_eval_restated, eval_loader, fixture, fixture_counts, fixture_rows,  # noqa: E402
                                 loop_config, run_box_eval, train_batches)
from test_hip_modules import _check_grads, _load_into, _pretrain_cfg  # noqa: E402
from xfm_amd import grounding_loop as GL  # noqa: E402
from xfm_amd import pretrain_loop as PL  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

IOU_TOL = 2.0 ** -23
U24 = 2.0 ** -24
COORD_TOL, LOSS_TOL = 1e-2, 2e-2


def _fx():
    from xfm_amd import functional as Fx
    return Fx


def _lib():
    from xfm_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------- xfm_box_eval
@pytest.mark.parametrize("out_offset", [0, 5])
@pytest.mark.parametrize("shuffled", [False, True], ids=["rows_null", "rows_shuffled"])
@pytest.mark.parametrize("n", BOX_EVAL_N)
def test_box_eval_matches_the_fp64_restatement(n, shuffled, out_offset):
    case = box_case(n, shuffled)
    want, want_counts = box_eval_restated(case.coord, case.ref_row, case.ref_box, case.ref_size, case.ref_split)
    if n >= 10:   # every kind occurs: a NaN row, an exact 0.5, an empty union, uncounted splits
        assert np.isnan(want[:, 4]).any() and (want[:, 4] == 0.5).any() and int(want_counts[:, 1].sum()) < n - int(np.isnan(want[:, 4]).sum())
    r = run_box_eval(case, out_offset=out_offset, calls=2)
    assert r.inputs_kept and r.out_kept and r.counts_kept
    nan = np.isnan(want[:, 4])
    assert np.isnan(r.out[nan]).all() and not np.isnan(r.out[~nan]).any()
    got, ref = r.out[~nan].astype(np.float64), want[~nan]
    iou_err = np.abs(got[:, 4] - ref[:, 4]).max() if len(ref) else 0.0
    pix_err = (np.abs(got[:, :4] - ref[:, :4]) - U24 * np.abs(ref[:, :4])).max() if len(ref) else 0.0
    print(f"n={n} shuffled={shuffled} off={out_offset}: IoU err {iou_err:.3e} (bound {IOU_TOL:.3e}), pixel err over its bound {pix_err:.3e}, "
          f"counts {r.counts.tolist()} want twice {want_counts.tolist()}")
    assert iou_err <= IOU_TOL
    assert pix_err <= 2.0 ** -149
    assert np.array_equal(r.counts, 2 * want_counts)   # two calls accumulate into one buffer
    for i, k in enumerate(case.kinds):
        if k == "threshold" and not nan[i]:
            assert r.out[i, 4] == 0.5
        if k == "one_pixel" and not nan[i]:
            assert r.out[i, 4] == 0.0
        if k == "union0" and not nan[i]:
            assert r.out[i, 4] == 0.0


def test_box_eval_same_bits_under_xfm_deterministic():
    """A fresh child process with XFM_DETERMINISTIC=1 against this process without it: out and counts of every case, bit for bit."""
    env = dict(os.environ, XFM_DETERMINISTIC="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "grounding_loop_util.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    child = [l for l in r.stdout.splitlines() if l.startswith("BOX_EVAL ")][-1].split()[1:]
    saved = os.environ.pop("XFM_DETERMINISTIC", None)
    try:
        own = box_eval_digests()
    finally:
        if saved is not None:
            os.environ["XFM_DETERMINISTIC"] = saved
    assert len(own) == 2 * len(BOX_EVAL_N) and child == own, (child, own)


def test_box_eval_argument_errors_launch_nothing():
    Fx, lib = _fx(), _lib().load()
    dev = "cuda"
    coord = torch.full((4, 4), 0.5, device=dev)
    box, size = torch.ones(4, 4, device=dev), torch.full((4, 2), 100.0, device=dev)
    split = torch.zeros(4, dtype=torch.int32, device=dev)
    counts = torch.full((6,), 5, dtype=torch.int64, device=dev)
    out = torch.full((8, 5), 7.0, device=dev)
    P = dict(coord=coord.data_ptr(), box=box.data_ptr(), size=size.data_ptr(), split=split.data_ptr(), counts=counts.data_ptr())
    for bad in (dict(n=0), dict(n=-3), dict(R=0), dict(off=-1), dict(coord=None), dict(box=None), dict(size=None), dict(split=None),
                dict(counts=None)):
        kw = dict(P, n=4, R=4, off=0)
        kw.update(bad)
        rc = lib.xfm_box_eval(kw["coord"], None, kw["box"], kw["size"], kw["split"], kw["n"], kw["R"], out.data_ptr(), kw["off"],
                              kw["counts"], None)
        assert rc == -1 and b"box_eval" in lib.xfm_last_error(), bad
    with pytest.raises(_lib().XfmHipError, match="box_eval"):
        Fx.box_eval(coord, None, box, size, split, counts, out, -1)
    torch.cuda.synchronize()
    assert counts.tolist() == [5] * 6 and float(out.min()) == 7.0 == float(out.max())


# ---------------------------------------------------------------------------------------------------------------- the task model
def test_grounding_model_fused_vs_golden(monkeypatch):
    """XFMForGrounding(..., fused=True) on grounding_small.npz under the bounds of test_grounding_model_vs_golden: the two losses come out
    of xfm_box_loss_fwd and their gradient out of xfm_box_loss_bwd."""
    import xfm_amd.xfm as X
    from xfm_amd.model_grounding import XFMForGrounding
    z, meta = load("grounding_small")
    m = XFMForGrounding(_pretrain_cfg(meta))
    _load_into(m, meta["spec"])
    m.cuda().finalize().eval()
    b = {k: v.cuda() for k, v in syn.pretrain_batch(meta["B"], seed=99).items()}
    target = torch.tensor(meta["target"]).cuda()
    calls = []
    real_fwd, real_bwd = X.Fx.box_loss_fwd, X.Fx.box_loss_bwd
    monkeypatch.setattr(X.Fx, "box_loss_fwd", lambda *a, **kw: (calls.append("fwd"), real_fwd(*a, **kw))[1])
    monkeypatch.setattr(X.Fx, "box_loss_bwd", lambda *a, **kw: (calls.append("bwd"), real_bwd(*a, **kw))[1])
    coord, l1, giou = m(b["image"], b["text_ids"], b["text_atts"], target_bbox=target, fused=True)
    print("coord err", np.abs(coord.detach().float().cpu().numpy() - z["coord"]).max(), "losses", float(l1), float(giou), "reference",
          float(z["loss_bbox"]), float(z["loss_giou"]))
    assert np.abs(coord.detach().float().cpu().numpy() - z["coord"]).max() < COORD_TOL
    assert abs(float(l1) - float(z["loss_bbox"])) < LOSS_TOL and abs(float(giou) - float(z["loss_giou"])) < LOSS_TOL
    (l1 + giou).backward()
    assert calls == ["fwd", "bwd"]
    _check_grads(z, "grad", m, min_rms=1e-6)


# ---------------------------------------------------------------------------------------------------------------- the loop
@pytest.fixture(scope="module")
def gold():
    z, meta = fixture()
    return z, meta, state_from_spec(meta["spec"])


def _build(gold, train):
    """The fixture model on the GPU; for training behind RCCLDDPAccelerator with the four-group optimizer and the linear schedule.  Dropout
    and drop-path are off, as in the fixture (the reference model stayed in eval mode)."""
    from xfm_amd.accelerators import RCCLDDPAccelerator
    from xfm_amd.model_grounding import XFMForGrounding
    z, meta, sd = gold
    cfg = loop_config(meta, text_config={"hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0})
    m = XFMForGrounding(cfg)
    m.load_state_dict(sd, strict=True)
    m.cuda()
    for blk in m.vision_encoder.blocks:
        blk.drop_path_prob = 0.0
    if not train:
        return cfg, m.finalize().eval(), None, None, None
    opt = PL.create_optimizer(PL.AttrDict(cfg["optimizer"]), m)
    sch = PL.AttrDict(cfg["schedular"])
    sch["step_per_epoch"] = len(meta["train_seeds"])
    scheduler = PL.create_scheduler(sch, opt)
    rec = {"loss": [], "steps": 0, "fused_adamw": 0}

    class Recording(RCCLDDPAccelerator):
        def backward_step(self, loss, optimizer, sync=None):
            rec["loss"].append(loss.detach())
            return super().backward_step(loss, optimizer, sync=sync)

        def optimizer_step(self, optimizer, model, grad_norm=0.0):
            rec["steps"] += 1
            return super().optimizer_step(optimizer, model, grad_norm)

        def _fused_adamw(self, optimizer, clip_coef):
            rec["fused_adamw"] += 1
            return super()._fused_adamw(optimizer, clip_coef)

    acc = Recording({"RNG_SEED": 3, "CLIP_GRAD_NORM": 0.0, "GRAD_ACCUMULATE_STEPS": 1})
    wrapped, opt, scheduler = acc.set_up(m, opt, scheduler, 0, 1, 0)
    return cfg, wrapped, opt, scheduler, (acc, rec)


def test_evaluation_against_the_reference_with_one_device_read(gold, monkeypatch, tmp_path):
    z, meta, _ = gold
    cfg, m, _, _, _ = _build(gold, train=False)
    loader = eval_loader(z, meta)
    reads, kernel_calls, coords = [], [], []
    real = GL._read

    def counted_read(t):
        value = real(t)
        reads.append((tuple(t.shape), value))
        return value

    monkeypatch.setattr(GL, "_read", counted_read)
    Fx = _fx()
    real_eval = Fx.box_eval
    monkeypatch.setattr(Fx, "box_eval", lambda *a, **kw: (kernel_calls.append(a[0].shape[0]), real_eval(*a, **kw))[1])
    hook = m.register_forward_hook(lambda mod, args, out: coords.append(out.detach().float().cpu()))
    dev = torch.device("cuda")
    acc = GL.evaluation(m, loader, dev, cfg, result_dir=str(tmp_path), filename="epoch0")
    hook.remove()
    print("accuracy", acc, "reference", meta["acc"], "counts", reads)
    assert [shape for shape, _ in reads] == [(3, 2)] and kernel_calls == meta["eval_batches"]   # ONE device read per pass
    assert np.array_equal(np.asarray(reads[0][1]), fixture_counts(z, meta))
    assert acc == meta["acc"] and set(acc) == {"val_d", "testA_d", "testB_d"}
    coord = torch.cat(coords).numpy()
    print("coords", coord.tolist(), "reference", z["eval/coord"].tolist())
    assert coord.shape == (meta["eval_B"], 4) and np.abs(coord - z["eval/coord"]).max() < COORD_TOL
    saved = torch.load(tmp_path / "epoch0.pth", weights_only=False)
    assert saved["ref_id"] == meta["ref_ids"] and tuple(saved["pred"].shape) == (meta["eval_B"], 5) and saved["pred"].dtype == torch.float32
    assert ((saved["pred"][:, 4].numpy() >= 0.5) == z["eval/correct"]).all()
    own, _ = box_eval_restated(coord, fixture_rows(meta), z["eval/ref_box"], z["eval/ref_size"], z["eval/ref_split"])
    assert np.abs(saved["pred"].double().numpy()[:, 4] - own[:, 4]).max() <= IOU_TOL   # the kernel on the GPU's own predictions
    # the VLUE form: every sample counts as one split
    reads.clear()
    score = GL.evaluation(m, loader, dev, dict(cfg, vlue_test=True))
    assert [shape for shape, _ in reads] == [(3, 2)] and score == {"score": int(z["eval/correct"].sum()) / meta["eval_B"]}


def test_two_training_iterations_against_the_reference(gold, monkeypatch):
    z, meta, _ = gold
    cfg, wrapped, opt, scheduler, (acc, rec) = _build(gold, train=True)
    fused = []
    inner = wrapped.module if hasattr(wrapped, "module") else wrapped
    orig = inner.get_bbox_loss
    monkeypatch.setattr(inner, "get_bbox_loss", lambda *a, **kw: (fused.append(kw.get("fused")), orig(*a, **kw))[1])
    meters = []
    stats = GL.train_one_epoch(wrapped, train_batches(meta), opt, 0, torch.device("cuda"), scheduler, cfg, acc, print_freq=1,
                               log=lambda epoch, i, avg: meters.append(dict(avg)))
    ref = z["train/loss"]
    # the meters hold running means: undo them to get the two iterations' own values
    l_bbox = [meters[0]["loss_bbox"], 2 * meters[1]["loss_bbox"] - meters[0]["loss_bbox"]]
    l_giou = [meters[0]["loss_giou"], 2 * meters[1]["loss_giou"] - meters[0]["loss_giou"]]
    print("loss_bbox", l_bbox, "loss_giou", l_giou, "reference", ref.tolist(), "total", [float(l) for l in rec["loss"]])
    assert rec["steps"] == 2 == rec["fused_adamw"] and len(rec["loss"]) == 2 and fused == [True, True]   # two steps on xfm_adamw
    assert [g["lr"] for g in opt.param_groups] == z["train/lr"][1].tolist()   # after two scheduler steps
    for i in range(2):
        assert abs(l_bbox[i] - ref[i, 0]) <= LOSS_TOL and abs(l_giou[i] - ref[i, 1]) <= LOSS_TOL, (i, l_bbox, l_giou, ref.tolist())
        assert abs(float(rec["loss"][i]) - (l_bbox[i] + l_giou[i])) <= 1e-5
    assert set(stats) == {"loss_bbox", "loss_giou", "lr"}


# ---------------------------------------------------------------------------------------------------------------- the script
def test_grounding_script_main_trains_evaluates_and_keeps_the_best_checkpoint(gold, tmp_path, capsys):
    """Grounding_bbox.py's main() as `run.py --task refcoco_bbox` starts it, at the fixture's shallow shape with synthetic loaders: one
    epoch, the log line, the best checkpoint and the result file; then the `--evaluate` form on a fresh model.
    So that val_d is known to beat 0, both runs start from a checkpoint whose box head has a zero output weight and the bias that makes
    every prediction the box of the synthetic test set's first val ref; the `--evaluate` form (no training step in between) must then
    give exactly the accuracies the fp64 restatement gives for that constant prediction."""
    from types import SimpleNamespace as NS

    import Grounding_bbox as script
    from xfm_amd.model_grounding import XFMForGrounding
    _, meta, _ = gold
    n_test, seed = 12, 42
    cfg = loop_config(meta, synthetic=True, train_dataset_size=2 * meta["B"], test_dataset_size=n_test, print_freq=1)
    cfg["schedular"]["epochs"] = 1
    refs = script.SyntheticTestSet(n_test, seed + 15485863)   # the test set synthetic_loaders builds for rank 0
    assert sorted(set(refs.ref_split.tolist())) == [0, 1, 2] and int(refs.ref_split[0]) == 0
    (x, y, w, h), (W, H) = refs.ref_box[0].tolist(), refs.ref_size[0].tolist()
    const = torch.tensor([(x + w / 2) / W, (y + h / 2) / H, w / W, h / H], dtype=torch.float64)
    torch.manual_seed(0)
    sd = XFMForGrounding(cfg).state_dict()
    sd["bbox_head.3.weight"] = torch.zeros_like(sd["bbox_head.3.weight"])
    sd["bbox_head.3.bias"] = torch.log(const / (1 - const)).float()
    ckpt = tmp_path / "start.th"
    torch.save({"model": sd}, ckpt)
    coord = torch.sigmoid(sd["bbox_head.3.bias"]).expand(n_test, 4).numpy()
    want_out, want_counts = box_eval_restated(coord, None, refs.ref_box.numpy(), refs.ref_size.numpy(), refs.ref_split.numpy())
    assert want_out[0, 4] > 0.9 and np.abs(want_out[:, 4] - 0.5).min() > 1e-3   # (no flag hangs on the last bits of the sigmoid)
    want = {f"{name}_d": want_counts[s, 0] / want_counts[s, 1] for s, name in enumerate(GL.SPLITS)}
    assert want["val_d"] > 0

    out = tmp_path / "grd"
    (out / "result").mkdir(parents=True)
    args = NS(checkpoint=str(ckpt), bs=-1, seed=seed, evaluate=False, load_bbox_pretrain=True, output_hdfs="", output_dir=str(out),
              result_dir=str(out / "result"))
    script.main(args, dict(cfg, schedular=dict(cfg["schedular"]), optimizer=dict(cfg["optimizer"])))
    capsys.readouterr()
    text = (out / "log.txt").read_text().splitlines()
    line = json.loads(text[0])
    assert set(line) >= {"val_d", "testA_d", "testB_d", "train_loss_bbox", "train_loss_giou", "epoch"} and line["epoch"] == 0
    assert line["val_d"] > 0 and text[-1] == "best epoch: 0"
    best = torch.load(out / "model_state_epoch_best.th", weights_only=False)
    assert sorted(best) == ["config", "model"] and isinstance(best["model"], dict)
    assert (out / "training_state_latest.th").exists()
    saved = torch.load(out / "result" / "epoch0.pth", weights_only=False)
    assert saved["ref_id"] == list(range(n_test)) and tuple(saved["pred"].shape) == (n_test, 5)
    args.evaluate = True
    script.main(args, dict(cfg, schedular=dict(cfg["schedular"]), optimizer=dict(cfg["optimizer"])))
    import ast
    records = [ast.literal_eval(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{'val_d'")]
    assert records == [want], (records, want)
    saved = torch.load(out / "result" / "grounding_bbox_eval.pth", weights_only=False)
    assert saved["ref_id"] == list(range(n_test))
    err = np.abs(saved["pred"].double().numpy() - want_out)
    assert (err[:, 4] <= 1e-5).all() and (err[:, :4] <= 1e-4 * np.abs(want_out[:, :4]) + 1e-3).all(), err.max(0)
