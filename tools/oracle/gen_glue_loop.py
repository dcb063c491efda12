"""Generate tests/golden/glue_loop_small.npz from the REAL reference (behind ref_shim, as gen_golden.py does).

Run in the build container only:   python tools/oracle/gen_glue_loop.py

run_glue.py itself cannot be imported here (`datasets`, `accelerate`, ruamel, a tokenizer), so, as for vqa_loop_small: the MODEL is the
reference's XFMForClassification on its text-only branch (shallow towers, formula weights), the schedule values are those of the installed
`transformers.get_scheduler`, the optimizer is the HF AdamW rule (gen_vqa_loop.HFAdamW: this transformers no longer ships the class) over
the two groups of run_glue.py:292-303, and the loop of run_glue.py:347-421 is restated call for call around them on token-id batches.  The
model stays in eval mode (dropout off), which is how the other task fixtures make the run reproducible.

Three runs of one epoch each, B = 4, T <= 16:
  mrpc  2 labels, gradient_accumulation_steps 1, 3 batches
  mnli  3 labels, gradient_accumulation_steps 2, 5 batches -- updates fall at steps 0, 2, 4 (the rule AS WRITTEN, :360), and the final
        mismatched pass (:396-421)
  stsb  1 label (regression: MSE, Pearson / Spearman), 3 batches
Stored (data only): per-micro-batch losses, the learning rate at and after every update, the number of updates, parameter probes after the
run (the CPU loop test compares them; the GPU tests do not: Adam's first updates are sign-like), the evaluation logits / predictions / labels of 12 rows after the epoch, and the metric
values computed HERE with sklearn / scipy (what load_metric("glue", task) wraps).

The margin condition: every evaluation row of the classification runs has a top-1 minus top-2 logit margin above what the GPU tests' rule
on those logits (tests/test_hip_modules.py::_check_out: rel-L2 <= 2e-2 over the whole logits tensor) can move a difference of two entries
by, sqrt(2) * 2e-2 * ||logits||_2 -- so no allowed error flips an argmax, and predictions and confusion-derived metrics are compared for
EQUALITY.  The evaluation seeds are searched until the reference's own logits satisfy it; the margin and the bound go into `meta`."""
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
from gen_vqa_loop import HFAdamW  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

OUT_TOL = 2e-2   # tests/test_hip_modules.py OUT_TOL
GLUE_LOOP = {"B": 4, "max_length": 16, "min_len": 5, "eval_rows": 12, "text_layers": 2, "fusion_layers": 0,
             "learning_rate": 5e-5, "weight_decay": 0.01, "num_warmup_steps": 0, "lr_scheduler_type": "linear", "num_train_epochs": 1,
             "runs": {"mrpc": {"num_labels": 2, "gradient_accumulation_steps": 1, "train_seeds": [811, 812, 813]},
                      "mnli": {"num_labels": 3, "gradient_accumulation_steps": 2, "train_seeds": [821, 822, 823, 824, 825]},
                      "stsb": {"num_labels": 1, "gradient_accumulation_steps": 1, "train_seeds": [831, 832, 833]}},
             "sched_probe": {"num_warmup_steps": 2, "num_training_steps": 7, "steps": 9, "lr": 5e-5},
             "state_of": ["cls_head.0.weight", "cls_head.3.weight", "cls_head.3.bias", "text_encoder.encoder.layer.1.output.dense.weight",
                          "text_encoder.embeddings.LayerNorm.weight"]}
NO_DECAY = ["bias", "LayerNorm.weight"]   # run_glue.py:292


def batches(seeds, num_labels):
    L = GLUE_LOOP
    return [syn.glue_batch(L["B"], seed=s, max_length=L["max_length"], min_len=L["min_len"], num_labels=num_labels) for s in seeds]


def glue_metric(task, predictions, references):
    """datasets' glue metric (metrics/glue/glue.py): simple_accuracy, acc_and_f1, pearson_and_spearman, matthews_corrcoef."""
    from scipy.stats import pearsonr, spearmanr
    from sklearn.metrics import f1_score, matthews_corrcoef
    p, r = np.asarray(predictions), np.asarray(references)
    if task == "cola":
        return {"matthews_correlation": float(matthews_corrcoef(r, p))}
    if task == "stsb":   # (the metric hands scipy Python floats: fp64 arithmetic on the fp32 values)
        p, r = p.astype(np.float64), r.astype(np.float64)
        return {"pearson": float(pearsonr(p, r)[0]), "spearmanr": float(spearmanr(p, r)[0])}
    if task in ("mrpc", "qqp"):
        return {"accuracy": float((p == r).mean()), "f1": float(f1_score(y_true=r, y_pred=p))}
    return {"accuracy": float((p == r).mean())}


def evaluate(m, task, num_labels, seeds):
    """run_glue.py:370-386 on fixed batches -> logits, predictions, labels, metrics, margin."""
    logits, labels = [], []
    with torch.no_grad():
        for ids, atts, lab in batches(seeds, num_labels):
            logits.append(m(image=None, text_ids=ids, text_atts=atts, targets=lab, train=False))
            labels.append(lab)
    logits, labels = torch.cat(logits), torch.cat(labels)
    if num_labels == 1:
        preds = logits.squeeze()
        return dict(logits=logits, preds=preds, labels=labels, metric=glue_metric(task, preds.numpy(), labels.numpy()), margin=None,
                    bound=None)
    preds = logits.argmax(dim=-1)
    top = logits.sort(dim=1, descending=True).values
    margin = float((top[:, 0] - top[:, 1]).min())
    bound = math.sqrt(2.0) * OUT_TOL * float(logits.double().norm())
    return dict(logits=logits, preds=preds, labels=labels, metric=glue_metric(task, preds.numpy(), labels.numpy()), margin=margin, bound=bound)


def search_eval(m, task, num_labels, first_seed, tries=400):
    """The first evaluation seeds (3 batches of 4 rows) whose rows ALL clear the bound, preferring passes whose metric says something
    (more than one class predicted, accuracy strictly between 0 and 1, a non-zero F1 where the task has one)."""
    best = None
    for base in range(first_seed, first_seed + 3 * tries, 3):
        seeds = [base, base + 1, base + 2]
        ev = evaluate(m, task, num_labels, seeds)
        if num_labels == 1:
            return seeds, ev
        if ev["margin"] <= 1.05 * ev["bound"]:
            continue
        acc = ev["metric"]["accuracy"]
        telling = 0.0 < acc < 1.0 and len(set(ev["preds"].tolist())) > 1 and ev["metric"].get("f1", 1.0) > 0.0
        if best is None or (telling, ev["margin"] / ev["bound"]) > best[0]:
            best = ((telling, ev["margin"] / ev["bound"]), seeds, ev)
        if telling and best[0][1] > 1.5:
            break
    assert best is not None, f"{task}: no evaluation seeds whose margins clear the bound; scale the cls_head output weights"
    return best[1], best[2]


def schedule_probe():
    """Learning rates of transformers.get_scheduler for every type glue_loop builds, value for value."""
    from transformers import get_scheduler
    P = GLUE_LOOP["sched_probe"]
    out = {}
    for name in ("linear", "constant", "constant_with_warmup", "cosine"):
        w = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([w], lr=P["lr"])
        sch = get_scheduler(name=name, optimizer=opt, num_warmup_steps=P["num_warmup_steps"], num_training_steps=P["num_training_steps"])
        lrs = []
        for _ in range(P["steps"]):
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
        out[name] = lrs
    return out


def main():
    import models.beit2 as rb
    from models.model_classification import XFMForClassification
    from transformers import get_scheduler
    ref_shim.init_single_process_group()
    L = GLUE_LOOP
    out, meta_runs, spec_by_run, groups_by_run = {}, {}, {}, {}
    for task, R in L["runs"].items():
        torch.manual_seed(0)
        with G.shallow_vit():
            probe = rb.beit_base_patch16(img_size=224, drop_rate=0.0, drop_path_rate=0.1, attn_drop_rate=0.0, use_mean_pooling=True,
                                         init_scale=0.001, use_rel_pos_bias=True, use_abs_pos_emb=False, init_values=0.1, qkv_bias=True,
                                         local_attn_depth=-1)   # (the re-bound factory)
            config = ref_shim.pretrain_config(text_layers=L["text_layers"], fusion_layers=L["fusion_layers"], overrides={
                "vision_config": G._beit_ckpt_config(probe), "task_name": task, "num_labels": R["num_labels"]})
            m = XFMForClassification(config)
        G.load_formula(m)
        m.eval()
        # run_glue.py:292-303
        optimizer_grouped_parameters = [
            {"params": [p for n, p in m.named_parameters() if not any(nd in n for nd in NO_DECAY)], "weight_decay": L["weight_decay"]},
            {"params": [p for n, p in m.named_parameters() if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]
        optimizer = HFAdamW(optimizer_grouped_parameters, lr=L["learning_rate"])
        names = {id(p): n for n, p in m.named_parameters()}
        groups = [[names[id(p)] for p in g["params"]] for g in optimizer.param_groups]
        loader = batches(R["train_seeds"], R["num_labels"])
        gas = R["gradient_accumulation_steps"]
        # run_glue.py:314-325
        num_update_steps_per_epoch = math.ceil(len(loader) / gas)
        max_train_steps = L["num_train_epochs"] * num_update_steps_per_epoch
        lr_scheduler = get_scheduler(name=L["lr_scheduler_type"], optimizer=optimizer, num_warmup_steps=L["num_warmup_steps"],
                                     num_training_steps=max_train_steps)
        losses, lr_at, lr_after, update_steps = [], [], [], []
        completed_steps = 0
        for epoch in range(L["num_train_epochs"]):   # run_glue.py:347-368
            for step, (input_ids, attention_mask, labels) in enumerate(loader):
                loss = m(image=None, text_ids=input_ids, text_atts=attention_mask, targets=labels)
                losses.append(float(loss.detach()))
                loss = loss / gas
                loss.backward()
                if step % gas == 0 or step == len(loader) - 1:
                    lr_at.append([g["lr"] for g in optimizer.param_groups])
                    optimizer.step()
                    lr_scheduler.step()
                    optimizer.zero_grad()
                    completed_steps += 1
                    update_steps.append(step)
                    lr_after.append([g["lr"] for g in optimizer.param_groups])
                if completed_steps >= max_train_steps:
                    break
        print(task, "losses", losses, "lr", lr_at, "updates at", update_steps, flush=True)
        out[f"{task}/loss"] = np.asarray(losses, dtype=np.float64)
        out[f"{task}/lr_at"] = np.asarray(lr_at, dtype=np.float64)
        out[f"{task}/lr_after"] = np.asarray(lr_after, dtype=np.float64)
        for n, p in m.named_parameters():
            if n in L["state_of"]:
                G.pack(f"{task}/param/{n}", p, out, 256)
        passes = [("eval", 900 if task != "stsb" else 960)] + ([("eval_mm", 2100)] if task == "mnli" else [])
        rec = {"num_labels": R["num_labels"], "gradient_accumulation_steps": gas, "train_seeds": R["train_seeds"], "updates": completed_steps,
               "update_steps": update_steps, "max_train_steps": max_train_steps,
               "stepped": sum(1 for p in m.parameters() if p in optimizer.state)}
        for tag, first_seed in passes:
            seeds, ev = search_eval(m, task, R["num_labels"], first_seed)
            print(task, tag, "seeds", seeds, "metric", ev["metric"], "margin", ev["margin"], "bound", ev["bound"], "preds", ev["preds"].tolist(),
                  "labels", ev["labels"].tolist(), flush=True)
            G.pack(f"{task}/{tag}_logits", ev["logits"], out)   # (12 x L entries: the probe IS the tensor)
            out[f"{task}/{tag}_preds"] = ev["preds"].numpy()
            out[f"{task}/{tag}_labels"] = ev["labels"].numpy()
            rec[tag] = {"seeds": seeds, "metric": ev["metric"], "margin": ev["margin"], "bound": ev["bound"]}
        meta_runs[task] = rec
        spec_by_run[task] = G.spec_of(m)
        groups_by_run[task] = groups
    sched = schedule_probe()
    for name, lrs in sched.items():
        out[f"sched/{name}"] = np.asarray(lrs, dtype=np.float64)
    # one spec serves the three runs up to the head's output width
    spec = spec_by_run["mrpc"]
    for task, s in spec_by_run.items():
        assert {k: v for k, v in s.items() if not k.startswith("cls_head.3.")} == {k: v for k, v in spec.items() if not k.startswith("cls_head.3.")}
        assert groups_by_run[task] == groups_by_run["mrpc"]
    meta = {"spec": spec, "groups": groups_by_run["mrpc"], "vit_depth": G.SHALLOW, "betas": [0.9, 0.999], "eps": 1e-6, "out_tol": OUT_TOL,
            **{k: v for k, v in GLUE_LOOP.items() if k != "runs"}, "runs": meta_runs}
    G.save("glue_loop_small", out, meta)
    print(json.dumps({k: v for k, v in meta.items() if k not in ("spec", "groups")})[:3000])


if __name__ == "__main__":
    ref_shim.install()
    main()
