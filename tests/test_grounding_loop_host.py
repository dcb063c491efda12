"""Host side of the grounding fine-tune / evaluation loop (xfm_amd.grounding_loop) without a GPU: box_eval_host against the fixture taken
from the REFERENCE's own computeIoU / grounding_eval_bbox (tests/golden/grounding_loop_small.npz, see tools/oracle/gen_grounding_loop.py),
the margin condition that lets the GPU tests compare flags for equality, the loop on the CPU model path (oracle forward, HF-rule AdamW
stepping), the best-checkpoint rule, the launcher's command line, the config, and the ABI of the box-evaluation kernel."""
import inspect
import itertools
import json
import os

import numpy as np
import pytest
import torch
import yaml

from grounding_loop_util import (box_eval_restated, eval_loader, fixture, fixture_counts, fixture_rows, loop_config, oracle_model,
                                 train_batches)
from test_vqa_loop_host import _close, _HFStep
from xfm_amd import grounding_loop as GL
from xfm_amd import pretrain_loop as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    z, meta = fixture()
    return z, meta


def _tables(z):
    return z["eval/ref_box"], z["eval/ref_size"], z["eval/ref_split"]


def test_box_eval_host_reproduces_the_reference_evaluation(gold):
    z, meta = gold
    rows = fixture_rows(meta)
    out, counts = GL.box_eval_host(z["eval/coord"], rows, *_tables(z))
    print("IoU", out[:, 4].tolist(), "reference", z["eval/iou"].tolist(), "source", meta["eval_source"])
    assert np.abs(out[:, 4] - z["eval/iou"]).max() <= 1e-6          # the reference forms the pixel box in fp32, this in fp64
    assert np.abs(out[:, :4] - z["eval/pixel_box"]).max() <= 1e-3   # pixels of up to 640: a few fp32 roundings of 3.8e-5 each
    assert ((out[:, 4] >= 0.5) == z["eval/correct"]).all()
    assert np.array_equal(counts, fixture_counts(z, meta))
    assert GL.grounding_acc(counts.tolist(), {}) == meta["acc"]
    assert GL.grounding_acc(counts.tolist(), {"vlue_test": True}) == {"score": int(z["eval/correct"].sum()) / meta["eval_B"]}
    # the independent restatement of the tests agrees with the module's host form, special rows included
    coord = np.concatenate([z["eval/coord"], [[0.5, 0.5, 0.0, 0.0], [0.3, 0.3, 0.2, 0.2], [0.3, 0.3, 0.2, 0.2]]]).astype(np.float32)
    box = np.concatenate([z["eval/ref_box"], [[5.0, 5.0, 0.0, 0.0]]]).astype(np.float32)
    size = np.concatenate([z["eval/ref_size"], [[100.0, 100.0]]]).astype(np.float32)
    split = np.concatenate([z["eval/ref_split"], [1]]).astype(np.int32)
    rows2 = np.concatenate([rows, [8, -1, 9]])
    a, ca = GL.box_eval_host(coord, rows2, box, size, split)
    b, cb = box_eval_restated(coord, rows2, box, size, split)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b)) and np.array_equal(ca, cb)
    assert a[6, 4] == 0.0 and np.isnan(a[7:]).all() and ca[1, 1] == counts[1, 1] + 1   # union 0: IoU 0, counted, not correct
    with pytest.raises(ZeroDivisionError):   # an empty split divides by zero, as the reference does
        GL.grounding_acc([[1, 2], [0, 0], [1, 1]], {})


def test_margin_condition_holds_on_the_fixture(gold):
    """Every sample's flag stays the same when each of its 4 coordinates moves by -1e-2, 0 or +1e-2 (all 81 combinations): 1e-2 is the
    coordinate bound of test_grounding_model_vs_golden, so no allowed error of the GPU path flips a flag.  All three splits and both
    outcomes occur."""
    z, meta = gold
    rows = fixture_rows(meta)
    assert meta["coord_tol"] == 1e-2
    for d in itertools.product((-1.0, 0.0, 1.0), repeat=4):
        moved = (z["eval/coord"].astype(np.float64) + np.asarray(d) * meta["coord_tol"]).astype(np.float32)
        out, _ = box_eval_restated(moved, rows, *_tables(z))
        assert ((out[:, 4] >= 0.5) == z["eval/correct"]).all(), (d, out[:, 4])
    assert sorted(set(z["eval/ref_split"][rows].tolist())) == [0, 1, 2] and set(z["eval/correct"].tolist()) == {True, False}
    box, size = z["eval/ref_box"], z["eval/ref_size"]   # valid ground truth: inside its image
    assert (box[:, :2] >= 0).all() and (box[:, 2:] > 0).all() and (box[:, 0] + box[:, 2] <= size[:, 0]).all() \
        and (box[:, 1] + box[:, 3] <= size[:, 1]).all()


def _optimizer(meta, model):
    opt = PL.create_optimizer(PL.AttrDict(meta["optimizer"]), model)
    sch = PL.AttrDict(meta["schedular"])
    sch["step_per_epoch"] = len(meta["train_seeds"])
    return opt, PL.create_scheduler(sch, opt), sch


def test_loop_on_the_cpu_model_path_reproduces_the_reference(gold, monkeypatch, tmp_path):
    z, meta = gold
    model = oracle_model(meta)
    cfg = loop_config(meta)
    # the evaluation pass at the formula weights: one read, the fixture's counts, accuracies and result rows
    reads = []
    real = GL._read
    monkeypatch.setattr(GL, "_read", lambda t: (reads.append(tuple(t.shape)), real(t))[1])
    loader = eval_loader(z, meta)
    acc = GL.evaluation(model, loader, "cpu", cfg, result_dir=str(tmp_path), filename="epoch0")
    assert reads == [(3, 2)] and acc == meta["acc"]
    saved = torch.load(tmp_path / "epoch0.pth", weights_only=False)
    assert saved["ref_id"] == meta["ref_ids"] and tuple(saved["pred"].shape) == (meta["eval_B"], 5)
    assert np.abs(saved["pred"][:, 4].numpy() - z["eval/iou"]).max() <= 1e-4   # (oracle coords within 2e-5 of the reference's)
    with torch.no_grad():
        image, (ids, atts), _ = eval_loader(z, meta, splits=(meta["eval_B"],))[0]
        coord = model(image, ids, atts)
    assert np.abs(coord.numpy() - z["eval/coord"]).max() <= 2e-5
    # two training iterations: both losses, the learning rates after each scheduler step
    opt, scheduler, sch = _optimizer(meta, model)
    assert (sch["num_warmup_steps"], sch["num_training_steps"]) == (meta["num_warmup_steps"], meta["num_training_steps"])
    assert [len(g["params"]) for g in opt.param_groups] == meta["groups"]
    step = _HFStep()
    lrs, logs = [], []
    real_step = scheduler.step
    monkeypatch.setattr(scheduler, "step", lambda *a, **kw: (real_step(*a, **kw), lrs.append([g["lr"] for g in opt.param_groups]))[0])
    stats = GL.train_one_epoch(model, train_batches(meta), opt, 0, "cpu", scheduler, cfg, step, print_freq=1,
                               log=lambda e, i, avg: logs.append(dict(avg)))
    ref = z["train/loss"]
    l_bbox = [logs[0]["loss_bbox"], 2 * logs[1]["loss_bbox"] - logs[0]["loss_bbox"]]
    l_giou = [logs[0]["loss_giou"], 2 * logs[1]["loss_giou"] - logs[0]["loss_giou"]]
    print("loss_bbox", l_bbox, "loss_giou", l_giou, "total", step.losses, "reference", ref.tolist())
    _close(l_bbox, ref[:, 0])
    _close(l_giou, ref[:, 1])
    _close(step.losses, ref.sum(1))          # loss = loss_bbox + loss_giou
    assert np.array_equal(np.asarray(lrs), z["train/lr"])
    assert set(stats) == {"loss_bbox", "loss_giou", "lr"} and stats["loss_bbox"] == "{:.5f}".format(np.mean(l_bbox))


def test_train_keeps_the_best_checkpoint_and_names_the_best_epoch(gold, tmp_path):
    _, meta = gold
    vals = iter([0.2, 0.5, 0.4])
    seen, saved = [], []

    def stub(model, data_loader, device, config, result_dir=None, filename=None):
        seen.append((result_dir, filename))
        return {"val_d": next(vals), "testA_d": 0.1, "testB_d": 0.3}

    class Ckpt:
        def save_checkpoint(self, model_state, epoch, training_states, step=-1):
            saved.append((epoch, sorted(model_state), "state" in training_states))

    class NoStep:
        def backward_step(self, loss, optimizer):
            pass

        def optimizer_step(self, optimizer, model):
            pass

    model = torch.nn.Linear(2, 2)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    cfg = loop_config(meta)
    cfg["schedular"]["epochs"] = 3
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    best = GL.train(model, [], [], opt, "cpu", sched, cfg, NoStep(), Ckpt(), str(tmp_path), str(tmp_path / "r"), evaluate=stub)
    assert best == (0.5, 1)
    assert saved == [("best", ["config", "model"], True)] * 2               # epochs 0 and 1 beat the best so far, epoch 2 does not
    assert seen == [(str(tmp_path / "r"), "epoch%d" % e) for e in range(3)]
    text = (tmp_path / "log.txt").read_text().splitlines()
    assert [json.loads(l)["epoch"] for l in text[:3]] == [0, 1, 2] and text[3] == "best epoch: 1"
    assert [json.loads(l)["val_d"] for l in text[:3]] == [0.2, 0.5, 0.4] and set(json.loads(text[0])) == {"val_d", "testA_d", "testB_d", "epoch"}


def test_launcher_command_line_config_and_synthetic_loaders():
    import run as R
    a = R.parse(["--task", "refcoco_bbox", "--dist", "gpu0", "--output_dir", "out/grd", "--bs", "40"])
    cmd, nproc, vis, sa = R.task_command(a, 8)
    assert (nproc, vis) == (1, "0") and any(str(c).endswith("Grounding_bbox.py") for c in cmd)
    assert sa[sa.index("--config") + 1].endswith("configs/Grounding_bbox_synthetic.yaml")
    assert sa[sa.index("--bs") + 1] == 40 and sa[sa.index("--seed") + 1] == 42 and sa[sa.index("--output_dir") + 1] == "out/grd"   # --bs whole
    assert "--load_bbox_pretrain" in sa and "--evaluate" not in sa and "--checkpoint" not in sa and "--epoch" not in sa
    a.evaluate, a.checkpoint = True, "ckpt.th"
    sa = R.task_command(a, 8)[3]
    assert "--evaluate" in sa and sa[sa.index("--checkpoint") + 1] == "ckpt.th"
    assert "Grounding_bbox_pretrain.py" in R.__doc__   # the first stage is named as not built
    with pytest.raises(NotImplementedError):
        R.task_command(R.parse(["--task", "coco_captioning", "--dist", "gpu0", "--output_dir", "o"]), 8)

    import Grounding_bbox as script
    from types import SimpleNamespace as NS
    with pytest.raises(NotImplementedError, match="file-backed"):
        script.synthetic_loaders({"synthetic": False}, 0)
    with pytest.raises(NotImplementedError, match="output_hdfs"):
        script.main(NS(output_hdfs="hdfs://somewhere", bs=-1, seed=42, evaluate=False, checkpoint="", load_bbox_pretrain=False,
                       output_dir=".", result_dir="."), {})
    src = inspect.getsource(script)
    for flag in ("--checkpoint", "--config", "--output_dir", "--output_hdfs", "--device", "--seed", "--evaluate", "--load_bbox_pretrain", "--bs"):
        assert f'"{flag}"' in src, flag
    with open(os.path.join(ROOT, "configs", "Grounding_bbox_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    reference_keys = ["train_file", "test_file", "refcoco_data", "det_file", "coco_file", "image_root", "careful_hflip", "use_beit_v2",
                      "vision_config", "image_res", "patch_size", "local_attn_depth", "text_encoder", "text_num_hidden_layers",
                      "text_fusion_start_at", "fusion_num_hidden_layers", "fusion_fusion_start_at", "batch_size", "max_tokens", "optimizer",
                      "schedular"]   # the keys of the reference's configs/xfm-ft/Grounding_bbox.yaml
    assert [k for k in reference_keys if k not in cfg] == []
    assert cfg["image_res"] == 384 and cfg["batch_size"] == 20 and cfg["max_tokens"] == 40 and cfg["schedular"]["sched"] == "linear"
    assert cfg["optimizer"] == {"opt": "adamW", "lr": 2e-5, "weight_decay": 0.01, "lr_mult": 2}
    assert {"synthetic", "train_dataset_size", "test_dataset_size", "accelerator", "print_freq"} <= set(cfg)
    cfg.update(image_res=32, batch_size=3, train_dataset_size=7, test_dataset_size=9, max_tokens=12)
    train_loader, test_loader = script.synthetic_loaders(cfg, seed=42)
    assert len(train_loader) == 3 and len(test_loader) == 3   # ceil(7 / 3) as Grounding_bbox.py:192; 9 // 3
    image, (ids, atts), target = next(iter(train_loader))
    assert image.shape == (3, 3, 32, 32) and ids.shape == atts.shape and ids.shape[0] == 3 and ids.shape[1] <= 12
    assert int(atts.sum(1).max()) == ids.shape[1]             # padded to the longest expression of the batch
    assert target.shape == (3, 4) and target.dtype == torch.float32
    assert bool((target[:, :2] - target[:, 2:] / 2 >= 0).all()) and bool((target[:, :2] + target[:, 2:] / 2 <= 1).all())
    ref_ids = [int(r) for _, _, rid in test_loader for r in rid]
    ds = test_loader.dataset
    assert ref_ids == list(range(9)) and all(ds.ref_index[r] == r for r in ref_ids)
    box, size = ds.ref_box, ds.ref_size
    assert box.shape == (9, 4) and size.shape == (9, 2) and ds.ref_split.dtype == torch.int32
    assert sorted(set(ds.ref_split.tolist())) == [0, 1, 2]
    assert bool((box[:, :2] >= 0).all()) and bool((box[:, 2:] > 0).all())
    assert bool((box[:, 0] + box[:, 2] <= size[:, 0]).all()) and bool((box[:, 1] + box[:, 3] <= size[:, 1]).all())


def test_fused_keyword_and_cpu_tensors():
    from xfm_amd import _lib
    from xfm_amd import functional as Fx
    from xfm_amd.model_grounding import XFMForGrounding
    assert inspect.signature(XFMForGrounding.forward).parameters["fused"].default is False
    coord = torch.full((2, 4), 0.5)
    with pytest.raises(_lib.XfmHipError):
        Fx.box_eval(coord, None, torch.ones(2, 4), torch.ones(2, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int64))


def test_abi_and_new_symbol():
    """xfm_box_eval exists at ABI 16 and refuses bad arguments before anything is launched (host-only checks: the dummy non-NULL pointers
    are not read)."""
    from xfm_amd import _lib
    assert _lib.ABI_VERSION >= 16
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    assert "xfm_box_eval" in _lib.SIGNATURES and lib.xfm_box_eval is not None
    with open(os.path.join(ROOT, "include", "xfm_hip.h")) as f:
        hdr = f.read()
    assert "int xfm_box_eval(" in hdr and "utils.py:349-361" in hdr
    rc = lib.xfm_box_eval(None, None, None, None, None, 4, 4, None, 0, None, None)
    assert rc == -1 and b"box_eval" in lib.xfm_last_error()
    P = 0x10000
    for bad in (dict(n=0), dict(R=0), dict(off=-1)):
        kw = dict(n=4, R=4, off=0)
        kw.update(bad)
        rc = lib.xfm_box_eval(P, None, P, P, P, kw["n"], kw["R"], None, kw["off"], P, None)
        assert rc == -1 and b"box_eval" in lib.xfm_last_error(), bad
    with open(os.path.join(ROOT, "xfm_amd", "csrc", "capi.hip")) as f:
        assert f.read().count('#include "grounding.hip"') == 1
