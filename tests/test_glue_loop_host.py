"""Host side of the GLUE fine-tune / evaluation loop (xfm_amd.glue_loop) without a GPU: the schedules and the optimizer groups value for value
and name for name, the three runs on the CPU model path (oracle forward, HF-rule AdamW stepping) against tests/golden/glue_loop_small.npz
-- the REFERENCE's loop, see tools/oracle/gen_glue_loop.py --, the metrics on hand-worked cases, the launcher's command line, a run of the
shipped config, and the ABI of the four metric / loss kernels."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from glue_loop_util import (correlations_restated, eval_batches, fixture, loop_config, oracle_model, ranks_restated, train_batches)
from golden_util import check
from xfm_amd import glue_loop as GL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ("mrpc", "mnli", "stsb")


def _close(got, ref):
    """tests/test_imagenet_loop_host.py's rule for its CPU loop (golden_util.check): |err| <= 2e-5 + 2e-4 * rms of the reference."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt((ref * ref).mean()))
    err = float(np.abs(got - ref).max())
    assert err <= 2e-5 + 2e-4 * rms, (err, rms, got, ref)


class _HFStep:
    """backward / step without an arena, stepping with the transformers AdamW rule that glue_loop.create_optimizer's object stands for (eps
    before the bias correction, decay after the update): what xfm_adamw runs on the GPU.  Takes the loop's `sync` hint and records it."""
    takes_sync_hint = True

    def __init__(self):
        self.losses, self.syncs, self.lr_at = [], [], []

    def backward_step(self, loss, optimizer, sync=None):
        self.losses.append(float(loss.detach()))
        self.syncs.append(sync)
        loss.backward()

    @torch.no_grad()
    def optimizer_step(self, optimizer, model):
        self.lr_at.append([g["lr"] for g in optimizer.param_groups])
        for g in optimizer.param_groups:
            b1, b2 = g["betas"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = optimizer.state[p]
                if not st:
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                st["exp_avg"].mul_(b1).add_(p.grad, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                step_size = g["lr"] * math.sqrt(1 - b2 ** st["step"]) / (1 - b1 ** st["step"])
                p.addcdiv_(st["exp_avg"], st["exp_avg_sq"].sqrt().add_(g["eps"]), value=-step_size)
                if g["weight_decay"] > 0:
                    p.add_(p, alpha=-g["lr"] * g["weight_decay"])
        optimizer.zero_grad()


def test_schedules_match_transformers_value_for_value():
    z, meta = fixture()
    P = meta["sched_probe"]
    for name in ("linear", "constant", "constant_with_warmup", "cosine"):
        w = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([w], lr=P["lr"])
        cfg = {"gradient_accumulation_steps": 1, "max_train_steps": P["num_training_steps"], "num_train_epochs": None,
               "lr_scheduler_type": name, "num_warmup_steps": P["num_warmup_steps"]}
        sch = GL.create_scheduler(cfg, opt, 4)
        assert cfg["num_train_epochs"] == math.ceil(P["num_training_steps"] / 4)   # run_glue.py:318
        got = []
        for _ in range(P["steps"]):
            got.append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
        ref = z[f"sched/{name}"]
        assert ref.dtype == np.float64 and np.array_equal(np.asarray(got), ref), (name, got, ref.tolist())
    assert z["sched/linear"][0] == 0.0 and z["sched/linear"][2] == P["lr"] and z["sched/linear"][-1] == 0.0
    assert set(z["sched/constant"].tolist()) == {P["lr"]} and 0 < z["sched/cosine"][4] < P["lr"]
    for name in ("cosine_with_restarts", "polynomial"):
        with pytest.raises(NotImplementedError, match="run_glue.py:320-325"):
            GL.create_scheduler({"gradient_accumulation_steps": 1, "max_train_steps": 5, "lr_scheduler_type": name, "num_warmup_steps": 0},
                                torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0), 4)
    # the step arithmetic of :314-318 for the accumulating run: 5 batches, gas 2 -> 3 updates per epoch
    cfg = loop_config(meta, "mnli")
    GL.create_scheduler(cfg, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0), 5)
    assert cfg["max_train_steps"] == 3 == meta["runs"]["mnli"]["max_train_steps"] and cfg["num_train_epochs"] == 1
    cfg = dict(cfg, max_train_steps=None, num_batches_per_epoch=5, num_train_epochs=4)
    GL.create_scheduler(cfg, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0))
    assert cfg["max_train_steps"] == 12


def test_optimizer_groups_match_the_reference_name_for_name():
    z, meta = fixture()
    model = oracle_model(meta, "mrpc")
    opt = GL.create_optimizer(loop_config(meta, "mrpc"), model)
    assert type(opt) is torch.optim.AdamW and len(opt.param_groups) == 2
    names = {id(p): n for n, p in model.named_parameters()}
    have = set(names.values())
    got = [[names[id(p)] for p in g["params"]] for g in opt.param_groups]
    want = [[n for n in g if n in have] for g in meta["groups"]]   # (the CPU model path carries the text tower and the head only)
    assert got == want and len(got[0]) > 10 and len(got[1]) > 10
    assert all(("bias" in n or "LayerNorm.weight" in n) for n in got[1]) and not any("bias" in n or "LayerNorm.weight" in n for n in got[0])
    assert [g["weight_decay"] for g in opt.param_groups] == [meta["weight_decay"], 0.0]
    for g in opt.param_groups:
        assert tuple(g["betas"]) == tuple(meta["betas"]) == (0.9, 0.999) and g["eps"] == meta["eps"] == 1e-6
        assert g["lr"] == meta["learning_rate"] and "adamw_rule" not in g
    from xfm_amd.accelerators.rccl_ddp_accelerator import adamw_rule
    assert adamw_rule(opt) == "transformers"


@pytest.mark.parametrize("task", TASKS)
def test_loop_on_the_cpu_model_path_reproduces_the_reference(task, tmp_path):
    z, meta = fixture()
    R = meta["runs"][task]
    model = oracle_model(meta, task)
    cfg = loop_config(meta, task)
    opt = GL.create_optimizer(cfg, model)
    loader = train_batches(meta, task)
    assert all(ids.shape[1] == int(atts.sum(1).max()) <= meta["max_length"] for ids, atts, _ in loader)   # padded to the batch's longest
    sch = GL.create_scheduler(cfg, opt, len(loader))
    acc = _HFStep()
    saved = []

    class Ckpt:
        def save_checkpoint(self, model_state, epoch, training_states, step=-1):
            saved.append((epoch, sorted(model_state), isinstance(model_state["model"], dict), len(training_states["state"])))

    mm = eval_batches(meta, task, "eval_mm") if task == "mnli" else None
    history = GL.train(model, loader, eval_batches(meta, task), opt, sch, "cpu", cfg, acc, Ckpt(), str(tmp_path), mismatched_loader=mm)
    gas = R["gradient_accumulation_steps"]
    losses = [l * gas for l in acc.losses]   # loss / gradient_accumulation_steps goes into the backward (:358)
    print(task, "losses", losses, "reference", z[f"{task}/loss"].tolist())
    _close(losses, z[f"{task}/loss"])
    assert np.array_equal(np.asarray(acc.lr_at), z[f"{task}/lr_at"])
    assert [g["lr"] for g in opt.param_groups] == z[f"{task}/lr_after"][-1].tolist() == [0.0, 0.0]
    assert len(acc.lr_at) == R["updates"] == 3
    assert [i for i, s in enumerate(acc.syncs) if s] == R["update_steps"]          # (0, 2, 4 for the gas = 2 run of 5 batches)
    P = model.table()
    for n in meta["state_of"]:
        check(z, f"{task}/param/{n}", P[n], atol=2e-5, rtol=2e-4)
    assert saved == [(0, ["config", "model"], True, R["stepped"])]   # a state_dict, where :391 pickles the module
    lines = [json.loads(l) for l in open(tmp_path / "log.txt")]
    assert lines[0]["epoch"] == 0 and lines[0]["completed_steps"] == 3 and lines[0]["train_loss"] == "{:.5f}".format(np.mean(losses))
    passes = [("eval", history[0])] + ([("eval_mm", history[1])] if task == "mnli" else [])
    assert len(history) == len(passes) and (task != "mnli" or (history[1]["epoch"] == "mnli-mm" and lines[1]["epoch"] == "mnli-mm"))
    for tag, h in passes:
        res = GL.evaluate(model, eval_batches(meta, task, tag), "cpu", cfg)
        assert {k: h[k] for k in GL.TASK_METRICS[task]} == dict(res)
        with torch.no_grad():
            logits = torch.cat([model(None, ids, atts, lab, train=False) for ids, atts, lab in eval_batches(meta, task, tag)])
        _close(logits.numpy().reshape(-1), z[f"{task}/{tag}_logits/probe"])
        ref_metric = R[tag]["metric"]
        assert res.count == meta["eval_rows"] == 12 and set(res) == set(ref_metric) == set(GL.TASK_METRICS[task])
        if task == "stsb":
            _close(res.predictions, z[f"{task}/{tag}_preds"])
            labels = torch.cat([lab for _, _, lab in eval_batches(meta, task, tag)]).numpy()
            assert np.array_equal(labels, z[f"{task}/{tag}_labels"]) and len(set(labels.tolist())) < 12   # the 0.2 grid: tied labels
            # the host form against scipy's figures ON THE REFERENCE'S OWN predictions, and against the restatement on the loop's
            ref = GL.correlations_host(z[f"{task}/{tag}_preds"], z[f"{task}/{tag}_labels"])
            own = correlations_restated(res.predictions, labels)
            print(task, "correlations", dict(res), "reference", ref_metric)
            for got, want in ((ref[0], ref_metric["pearson"]), (ref[1], ref_metric["spearmanr"]), (res["pearson"], own[0]),
                              (res["spearmanr"], own[1])):
                assert abs(got - want) <= 1e-10, (got, want)
            assert abs(res["spearmanr"] - ref_metric["spearmanr"]) <= 1e-10   # the ranks of 12 separated predictions do not move
            _close([res["pearson"]], [ref_metric["pearson"]])                 # (the loop's OWN predictions: the CPU loop's rule)
        else:
            assert R[tag]["margin"] > R[tag]["bound"] > 0   # the generator's condition: no allowed error flips an argmax
            assert list(res.predictions) == z[f"{task}/{tag}_preds"].tolist()
            assert dict(res) == ref_metric, (dict(res), ref_metric)
            L = R["num_labels"]
            want = np.bincount(z[f"{task}/{tag}_labels"] * L + z[f"{task}/{tag}_preds"], minlength=L * L).reshape(L, L)
            assert res.confusion == want.tolist()


def test_metrics_hand_worked():
    # every prediction is class 0: no positive prediction -> F1 = 0 (zero denominator rule: TP = FP = 0, FN = 3 gives 0 / 3 = 0 as well),
    # one predicted class -> MCC = 0 by the zero-denominator rule
    conf = [[5, 0], [3, 0]]
    assert GL.metrics_from_confusion("mrpc", conf) == {"accuracy": 5 / 8, "f1": 0.0}
    assert GL.metrics_from_confusion("cola", conf) == {"matthews_correlation": 0.0}
    assert GL.metrics_from_confusion("qqp", [[4, 0], [0, 0]]) == {"accuracy": 1.0, "f1": 0.0}   # 2 TP + FP + FN = 0
    # binary: TP = 3, FP = 1, FN = 2, TN = 4 -> F1 = 6 / 9; MCC = (3 * 4 - 1 * 2) / sqrt(4 * 5 * 5 * 6)
    conf = [[4, 1], [2, 3]]
    m = GL.metrics_from_confusion("mrpc", conf)
    assert m["accuracy"] == 0.7 and m["f1"] == pytest.approx(6 / 9, abs=1e-15)
    assert GL.metrics_from_confusion("cola", conf)["matthews_correlation"] == pytest.approx(10 / math.sqrt(600), abs=1e-15)
    # three classes, rows = labels: c = 2 + 1 + 3 = 6, s = 10, t = (3, 3, 4), p = (3, 2, 5)
    conf = [[2, 0, 1], [1, 1, 1], [0, 1, 3]]
    num = 6 * 10 - (3 * 3 + 3 * 2 + 4 * 5)
    den = math.sqrt((100 - (9 + 4 + 25)) * (100 - (9 + 9 + 16)))
    assert GL.metrics_from_confusion("mnli", conf) == {"accuracy": 0.6}
    assert GL.metrics_from_confusion("mnli", np.asarray(conf).reshape(-1)) == {"accuracy": 0.6}
    # (cola is binary in GLUE; the formula is the multiclass one and is checked on three classes through its own name)
    GL.TASK_METRICS["_mcc3"] = ("matthews_correlation",)
    try:
        assert GL.metrics_from_confusion("_mcc3", conf)["matthews_correlation"] == pytest.approx(num / den, abs=1e-15)
    finally:
        del GL.TASK_METRICS["_mcc3"]
    assert set(GL.TASK_METRICS) == {"cola", "stsb", "mrpc", "qqp", "sst2", "mnli", "mnli_matched", "mnli_mismatched", "qnli", "rte", "wnli"}
    assert [GL.task_num_labels(t) for t in ("stsb", "mnli", "mrpc", "cola")] == [1, 3, 2, 2]


def test_correlations_host_hand_worked():
    x = [1.0, 2.0, 3.0, 4.0]
    assert GL.correlations_host(x, [2.0, 4.0, 6.0, 8.0]) == (pytest.approx(1.0, abs=1e-15), pytest.approx(1.0, abs=1e-15))
    p, s = GL.correlations_host(x, [5.0, 5.0, 5.0, 5.0])   # a constant vector: zero denominator -> NaN, as scipy returns
    assert math.isnan(p) and math.isnan(s)
    p, s = GL.correlations_host(x, [1.0, float("nan"), 2.0, 3.0])
    assert math.isnan(p) and math.isnan(s)
    # ties share the mean of their 1-based positions; -0.0 == +0.0
    assert GL.average_ranks([0.4, -0.0, 0.4, 0.0, -3.0, 0.4]).tolist() == [5.0, 2.5, 5.0, 2.5, 1.0, 5.0]
    assert ranks_restated([0.4, -0.0, 0.4, 0.0, -3.0, 0.4]).tolist() == [5.0, 2.5, 5.0, 2.5, 1.0, 5.0]
    # x ranks (1, 2, 3, 4), y ranks (1.5, 1.5, 3, 4): Sxy = 4.5, Sxx = 5, Syy = 4.5
    p, s = GL.correlations_host(x, [0.2, 0.2, 0.6, 1.0])
    assert s == pytest.approx(4.5 / math.sqrt(5 * 4.5), abs=1e-15)
    g = np.random.default_rng(5)
    a, b = g.standard_normal(300), np.round(g.uniform(0, 5, 300) * 5) / 5
    got, want = GL.correlations_host(a, b), correlations_restated(a, b)
    assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12


def test_launcher_command_line_and_synthetic_loaders():
    import run as R
    a = R.parse(["--task", "glue", "--dist", "gpu0", "--output_dir", "out/glue", "--bs", "64", "--epoch", "3"])
    cmd, nproc, vis, sa = R.task_command(a, 8)
    assert (nproc, vis) == (1, "0") and any(str(c).endswith("run_glue.py") for c in cmd)
    assert "--bs" not in sa and "--epoch" not in sa and "--checkpoint" not in sa           # run.py:263-272 of the reference
    assert sa[sa.index("--config") + 1].endswith("configs/glue_synthetic.yaml")
    assert sa[sa.index("--output_dir") + 1] == "out/glue" and sa[sa.index("--seed") + 1] == 42
    a.checkpoint = "ckpt.th"
    sa = R.task_command(a, 8)[3]
    assert sa[sa.index("--checkpoint") + 1] == "ckpt.th"
    a.task = "coco_captioning"
    with pytest.raises(NotImplementedError):
        R.task_command(a, 8)
    import run_glue as script
    with pytest.raises(NotImplementedError, match="file-backed"):
        script.synthetic_loaders({"synthetic": False}, 0)
    ref_keys = ["train_file", "validation_file", "test_file", "glue_datasets", "task_name", "num_labels", "max_length",
                "per_device_train_batch_size", "per_device_eval_batch_size", "learning_rate", "weight_decay", "num_train_epochs",
                "max_train_steps", "pad_to_max_length", "use_slow_tokenizer", "gradient_accumulation_steps", "num_warmup_steps", "seed",
                "lr_scheduler_type", "output_dir", "checkpoint", "ckpt_frequent", "use_beit_v2", "vision_config", "image_res", "patch_size",
                "local_attn_depth", "text_encoder", "text_num_hidden_layers", "text_fusion_start_at", "fusion_num_hidden_layers",
                "fusion_fusion_start_at", "use_huggingface_models", "model_name_or_path"]   # configs/xfm-ft/glue_mrpc.yaml
    for name, task in (("glue_synthetic.yaml", "mrpc"), ("glue_synthetic_stsb.yaml", "stsb")):
        with open(os.path.join(ROOT, "configs", name)) as f:
            cfg = yaml.safe_load(f)
        assert set(ref_keys) <= set(cfg) and cfg["synthetic"] is True and cfg["task_name"] == task
        assert cfg["num_labels"] == GL.task_num_labels(task) and cfg["max_train_steps"] is None and not cfg["use_huggingface_models"]
    ids, atts, labels = __import__("xfm_amd.synthetic", fromlist=["x"]).glue_batch(6, seed=3, max_length=20, min_len=4, num_labels=1)
    assert labels.dtype == torch.float32 and ids.shape == atts.shape and ids.shape[1] == int(atts.sum(1).max()) <= 20
    assert all(abs(v * 5 - round(v * 5)) < 1e-5 and 0.0 <= v <= 5.0 for v in labels.tolist())
    assert bool((ids[atts == 0] == 1).all()) and bool((ids[:, 0] == 0).all())


def test_one_epoch_run_of_the_synthetic_config_writes_log_and_checkpoint(tmp_path):
    import run_glue as script
    from xfm_amd import task as T
    z, meta = fixture()
    with open(os.path.join(ROOT, "configs", "glue_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    # the config's keys at a size the CPU model path runs in seconds: the fixture's depth, 3 x 4 training pairs of at most 16 tokens
    cfg.update(text_num_hidden_layers=meta["text_layers"], text_fusion_start_at=meta["text_layers"], max_length=16, num_train_epochs=1,
               per_device_train_batch_size=4, per_device_eval_batch_size=4, train_dataset_size=12, val_dataset_size=8)
    train_loader, val_loader, mm = script.synthetic_loaders(cfg, seed=42)
    assert len(train_loader) == 3 and len(val_loader) == 2 and mm is None
    ids, atts, labels = next(iter(train_loader))
    assert ids.shape[0] == 4 and ids.shape[1] <= 16 and labels.dtype == torch.int64 and 0 <= int(labels.min()) and int(labels.max()) < 2
    model = oracle_model(meta, "mrpc")
    opt = GL.create_optimizer(cfg, model)
    sch = GL.create_scheduler(cfg, opt, len(train_loader))
    history = GL.train(model, train_loader, val_loader, opt, sch, "cpu", cfg, _HFStep(), T.Checkpointer(str(tmp_path)), str(tmp_path))
    assert len(history) == 1 and set(history[0]) == {"epoch", "accuracy", "f1"} and 0.0 <= history[0]["accuracy"] <= 1.0
    line = json.loads(open(tmp_path / "log.txt").read())
    assert line["epoch"] == 0 and line["completed_steps"] == 3 and line["eval_accuracy"] == history[0]["accuracy"]
    ckpt = torch.load(tmp_path / "model_state_epoch_0.th", weights_only=False)
    assert sorted(ckpt) == ["config", "model"] and isinstance(ckpt["model"], dict) and ckpt["config"]["task_name"] == "mrpc"
    assert torch.load(tmp_path / "training_state_latest.th", weights_only=False)["epoch"] == 0


def test_abi_and_new_symbols():
    """The four entry points exist at ABI 15, and refuse bad arguments before anything is launched (host-only checks: the dummy non-NULL
    pointers are not read)."""
    from xfm_amd import _lib
    from xfm_amd import functional as Fx
    assert _lib.ABI_VERSION >= 15
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    for name in ("xfm_cls_eval", "xfm_corr_rank", "xfm_mse_fwd", "xfm_mse_bwd"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "xfm_hip.h")).read()
    assert f"#define XFM_METRIC_MAX_L {Fx.METRIC_MAX_L}" in hdr and f"#define XFM_CORR_MAX_N {Fx.CORR_MAX_N}" in hdr
    assert Fx.METRIC_MAX_L >= 32 and Fx.CORR_MAX_N == 8192
    P = 0x10000
    for bad in (dict(B=0), dict(L=1), dict(L=Fx.METRIC_MAX_L + 1, ld=64), dict(ld=2), dict(off=-1), dict(logits=None), dict(labels=None),
                dict(conf=None)):
        kw = dict(logits=P, ld=3, B=4, L=3, labels=P, conf=P, pred=P, off=0)
        kw.update(bad)
        rc = lib.xfm_cls_eval(kw["logits"], kw["ld"], kw["B"], kw["L"], kw["labels"], kw["conf"], kw["pred"], kw["off"], None)
        assert rc == -1 and b"cls_eval" in lib.xfm_last_error(), bad
    for bad in (dict(N=1), dict(N=Fx.CORR_MAX_N + 1), dict(x=None), dict(y=None), dict(out=None)):
        kw = dict(x=P, y=P, N=5, out=P)
        kw.update(bad)
        rc = lib.xfm_corr_rank(kw["x"], kw["y"], kw["N"], kw["out"], None, None, None)
        assert rc == -1 and b"corr_rank" in lib.xfm_last_error(), bad
    for bad in (dict(B=0), dict(stride=0), dict(pred=None), dict(target=None), dict(out=None)):
        kw = dict(pred=P, stride=1, target=P, B=4, out=P)
        kw.update(bad)
        rc = lib.xfm_mse_fwd(kw["pred"], kw["stride"], 0, kw["target"], kw["B"], kw["out"], None)
        assert rc == -1 and b"mse_fwd" in lib.xfm_last_error(), bad
        rc = lib.xfm_mse_bwd(kw["pred"], kw["stride"], 1, kw["target"], P, kw["B"], kw["out"], None)
        assert rc == -1 and b"mse_bwd" in lib.xfm_last_error(), bad
    assert lib.xfm_mse_bwd(P, 1, 0, P, None, 4, P, None) == -1
    # like every product op, the wrappers refuse CPU tensors
    with pytest.raises(_lib.XfmHipError):
        Fx.cls_eval(torch.zeros(2, 3), 3, torch.zeros(2, dtype=torch.int64), torch.zeros(9, dtype=torch.int64))
    with pytest.raises(_lib.XfmHipError):
        Fx.corr_rank(torch.zeros(4), torch.zeros(4))
    with pytest.raises(_lib.XfmHipError):
        Fx.mse_fwd(torch.zeros(4), torch.zeros(4))
    with pytest.raises(_lib.XfmHipError):
        Fx.mse_bwd(torch.zeros(4), torch.zeros(4), torch.ones(1))
