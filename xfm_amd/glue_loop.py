"""The GLUE fine-tune / evaluation task loop around the HIP step: optimizer, scheduler, the training epoch with the reference's gradient
accumulation rule, the evaluation pass with GLUE's metrics, and the per-epoch evaluation / checkpoint loop of run_glue.py.

Mirrors (names, argument meaning, ordering):
  * task_num_labels          run_glue.py:157-163   1 for stsb (regression), else the size of the task's label list
  * create_optimizer         run_glue.py:292-303   two AdamW groups (decay / no decay), transformers' AdamW defaults
  * create_scheduler         run_glue.py:314-325   the step arithmetic and get_scheduler
  * train_one_epoch          run_glue.py:347-368
  * evaluate                 run_glue.py:370-386   (and :404-421, the mismatched pass of mnli)
  * train                    run_glue.py:347-421
  * TASK_METRICS / metrics_from_confusion / correlations_host   what load_metric("glue", task).compute() returns
What differs, on purpose:
  * the batches carry TOKEN IDS: (input_ids, attention_mask, labels) tuples where the reference's collate emits a dict (:354-356); there is
    no tokenizer and no dataset code on this path;
  * the reference hands every batch's predictions and labels to `metric.add_batch` on the host (:381-384).  Here a classification batch
    adds its confusion counts into ONE int64 device buffer and writes its predictions behind the previous batch's (xfm_cls_eval); a
    regression batch copies its predictions and labels behind the previous batch's in two fp32 device buffers and xfm_corr_rank runs once
    at the end; the device is read ONCE per pass (`_read`) and the metrics follow from the counts on the host;
  * the training losses are parked (task.LossMeters) and read when a log line is due;
  * the checkpoint holds `model.state_dict()` where :391 pickles the module object;
  * under data parallelism EVERY rank evaluates the WHOLE validation set (no `accelerator.gather`, :382-383, no collective), as the VQA
    loop does: the metrics are identical on every rank."""
import json
import math
import os

import numpy as np
import torch

from . import functional as Fx
from .pretrain_loop import linear_schedule
from .task import LossMeters, is_distributed, is_main_process, to_device, unwrap
from .task import read as _read  # the loop's single device-to-host read (evaluate calls it once per pass; the tests count its calls)

F32 = torch.float32

# load_metric("glue", task): the names of the values compute() returns
TASK_METRICS = {"cola": ("matthews_correlation",), "stsb": ("pearson", "spearmanr"), "mrpc": ("accuracy", "f1"), "qqp": ("accuracy", "f1"),
                "sst2": ("accuracy",), "mnli": ("accuracy",), "mnli_matched": ("accuracy",), "mnli_mismatched": ("accuracy",),
                "qnli": ("accuracy",), "rte": ("accuracy",), "wnli": ("accuracy",)}
NO_DECAY = ("bias", "LayerNorm.weight")   # run_glue.py:292 (substring match)


def task_num_labels(task):
    """run_glue.py:157-163: regression (stsb) has one output; else the length of the GLUE task's label list."""
    if task not in TASK_METRICS:
        raise KeyError(f"task_name == {task!r} is not a GLUE task")
    return 1 if task == "stsb" else (3 if task.startswith("mnli") else 2)


# ------------------------------------------------------------------------------------------------------------------------ metrics
def metrics_from_confusion(task, conf):
    """The glue metric of a classification task from the confusion counts conf[label][prediction] (an [L, L] or flat [L * L] sequence of
    ints), in Python floats.  accuracy = trace / sum; binary f1 with positive label 1 = 2 TP / (2 TP + FP + FN), 0.0 when the
    denominator is 0; matthews_correlation = the multiclass formula (c s - sum_k t_k p_k) / sqrt((s^2 - sum_k p_k^2)(s^2 - sum_k t_k^2))
    with c the trace, s the sum, t_k the row sums and p_k the column sums, 0.0 when the denominator is 0."""
    flat = [int(v) for v in np.asarray(conf).reshape(-1).tolist()]
    L = int(round(math.sqrt(len(flat))))
    assert L * L == len(flat) and L >= 2, len(flat)
    m = [flat[r * L:(r + 1) * L] for r in range(L)]
    s = sum(flat)
    c = sum(m[k][k] for k in range(L))
    out = {}
    for name in TASK_METRICS[task]:
        if name == "accuracy":
            out[name] = c / s if s else float("nan")
        elif name == "f1":
            assert L == 2, "binary f1 (positive label 1)"
            tp, fp, fn = m[1][1], m[0][1], m[1][0]
            den = 2 * tp + fp + fn
            out[name] = 2.0 * tp / den if den else 0.0
        elif name == "matthews_correlation":
            t = [sum(m[k]) for k in range(L)]
            p = [sum(m[r][k] for r in range(L)) for k in range(L)]
            den = (s * s - sum(v * v for v in p)) * (s * s - sum(v * v for v in t))
            out[name] = (c * s - sum(a * b for a, b in zip(t, p))) / math.sqrt(den) if den else 0.0
        else:
            raise KeyError(f"{task}: {name} is not a confusion-matrix metric")
    return out


def average_ranks(v):
    """scipy.stats.rankdata(v, method='average') in numpy: a stable sort, then equal values share the mean of their 1-based positions."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    order = np.argsort(v, kind="stable")
    sv = v[order]
    starts = np.flatnonzero(np.r_[True, sv[1:] != sv[:-1]])
    ends = np.r_[starts[1:], v.size]
    ranks = np.empty(v.size, dtype=np.float64)
    ranks[order] = np.repeat((starts + 1 + ends) / 2.0, ends - starts)
    return ranks


def _pearson(a, b):
    da, db = a - a.sum() / a.size, b - b.sum() / b.size
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64((da * db).sum()) / np.sqrt(np.float64((da * da).sum()) * np.float64((db * db).sum())))


def correlations_host(x, y):
    """(pearson, spearmanr) of two vectors in fp64 on the host -- the definitions xfm_corr_rank computes: two-pass Pearson, the same formula
    on average ranks; a constant vector gives NaN (a zero denominator), and so does any NaN in x or y."""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    if np.isnan(x).any() or np.isnan(y).any():
        return float("nan"), float("nan")
    return _pearson(x, y), _pearson(average_ranks(x), average_ranks(y))


# ------------------------------------------------------------------------------------------------------------------------ factories
def create_optimizer(config, model):
    """run_glue.py:292-303: names containing `bias` or `LayerNorm.weight` get weight decay 0, the rest config['weight_decay'];
    transformers' AdamW defaults (betas (0.9, 0.999), eps 1e-6, bias correction on).  As in pretrain_loop.create_optimizer the
    torch.optim.AdamW object carries the groups / hyper-parameters / state_dict; it has NO `adamw_rule` marker, so RCCLDDPAccelerator
    steps it with the transformers rule (xfm_adamw)."""
    named = list(model.named_parameters())
    pg = [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": config['weight_decay']},
          {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]
    return torch.optim.AdamW(pg, lr=config['learning_rate'], betas=(0.9, 0.999), eps=1e-6)


def _schedule(name, num_warmup_steps, num_training_steps):
    """transformers.get_scheduler's multipliers (optimization.py) for the types built here."""
    if name == "linear":
        return lambda step: linear_schedule(step, num_warmup_steps, num_training_steps)
    if name == "constant":
        return lambda step: 1
    if name == "constant_with_warmup":
        return lambda step: float(step) / float(max(1.0, num_warmup_steps)) if step < num_warmup_steps else 1.0
    if name == "cosine":
        def cosine(step, num_cycles=0.5):
            if step < num_warmup_steps:
                return float(step) / float(max(1, num_warmup_steps))
            progress = float(step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))
        return cosine
    if name in ("cosine_with_restarts", "polynomial"):
        raise NotImplementedError(f"lr_scheduler_type == {name!r} (run_glue.py:320-325 get_scheduler) is not built: no shipped config sets it")
    raise ValueError(f"lr_scheduler_type == {name!r}")


def create_scheduler(config, optimizer, num_batches=None):
    """run_glue.py:314-325.  num_batches = len(train_dataloader) (default: config['num_batches_per_epoch']).  Fills config['max_train_steps']
    or config['num_train_epochs'] as the reference does and returns the LambdaLR of get_scheduler(config['lr_scheduler_type'])."""
    if num_batches is None:
        num_batches = config['num_batches_per_epoch']
    num_update_steps_per_epoch = math.ceil(num_batches / config['gradient_accumulation_steps'])
    if config.get('max_train_steps') is None:
        config['max_train_steps'] = config['num_train_epochs'] * num_update_steps_per_epoch
    else:
        config['num_train_epochs'] = math.ceil(config['max_train_steps'] / num_update_steps_per_epoch)
    fn = _schedule(config['lr_scheduler_type'], config['num_warmup_steps'], config['max_train_steps'])
    return torch.optim.lr_scheduler.LambdaLR(optimizer, fn, last_epoch=-1)


# ------------------------------------------------------------------------------------------------------------------------ loop
def _backward(accelerator, loss, optimizer, is_update):
    if getattr(accelerator, "takes_sync_hint", False):   # gradients are exchanged on the backward an update follows
        accelerator.backward_step(loss, optimizer, sync=is_update)
    else:
        accelerator.backward_step(loss, optimizer)


def train_one_epoch(model, loader, optimizer, lr_scheduler, epoch, device, config, accelerator, completed_steps=0, print_freq=50, log=None):
    """run_glue.py:347-368, the accumulation rule AS WRITTEN: loss / gradient_accumulation_steps goes into the backward, and an update
    happens when `step % gradient_accumulation_steps == 0 or step == len(loader) - 1` -- the first micro-batch of an epoch is an update
    of its own.  Gradients accumulate in the arena between updates (the accelerator zeroes them in optimizer_step).  The epoch ends
    early once completed_steps >= max_train_steps.  Returns (the epoch's meters, completed_steps)."""
    model.train()
    meters = LossMeters()
    gas = config['gradient_accumulation_steps']
    n = len(loader)
    for step, (input_ids, attention_mask, labels) in enumerate(loader):
        input_ids, attention_mask, labels = to_device(device, (input_ids, attention_mask, labels))
        loss = model(None, input_ids, attention_mask, labels)
        meters.update(loss=loss, lr=optimizer.param_groups[0]["lr"])
        loss = loss / gas
        is_update = step % gas == 0 or step == n - 1
        _backward(accelerator, loss, optimizer, is_update)
        if is_update:
            accelerator.optimizer_step(optimizer, model)   # (step, then zero_grad)
            lr_scheduler.step()
            completed_steps += 1
        if step % print_freq == 0:
            meters.flush()
            if log is not None:
                log(epoch, step, meters.global_avg())
        if completed_steps >= config['max_train_steps']:
            break
    return meters.global_avg(), completed_steps


class EvalResult(dict):
    """evaluate()'s return value: the metric dict of the task (what metric.compute() returns), with the pass's collected predictions
    (.predictions, a list), the confusion counts of a classification pass (.confusion, [L][L]) and the sample count attached."""
    predictions = ()
    confusion = None
    count = 0


@torch.no_grad()
def evaluate(model, loader, device, config):
    """run_glue.py:370-386: model.eval(), `outputs.argmax(dim=-1)` (classification) or `outputs.squeeze()` (regression) per batch, the glue
    metric over the pass.  A batch is (input_ids, attention_mask, labels).  One device read per pass (see the module docstring).  Above
    XFM_METRIC_MAX_L classes or XFM_CORR_MAX_N regression rows, and on CPU tensors, the plain torch / numpy form of the same definitions
    runs on the collected outputs."""
    model.eval()
    task = config['task_name']
    L = int(config['num_labels'])
    regression = L == 1
    cap = len(loader) * int(config['per_device_eval_batch_size'])
    conf = preds = refs = None
    done = 0
    for input_ids, attention_mask, labels in loader:
        input_ids, attention_mask, labels = to_device(device, (input_ids, attention_mask, labels))
        outputs = model(None, input_ids, attention_mask, labels, train=False)
        n = outputs.shape[0]
        if preds is None:
            dev = outputs.device
            preds = torch.zeros(cap, dtype=F32 if regression else torch.int64, device=dev)
            refs = torch.zeros(cap, dtype=F32 if regression else torch.int64, device=dev)
            conf = None if regression else torch.zeros(L * L, dtype=torch.int64, device=dev)
        assert done + n <= cap, "a batch larger than per_device_eval_batch_size"
        if regression:
            preds[done:done + n] = outputs.reshape(-1)
            refs[done:done + n] = labels.reshape(-1)
        else:
            labels = labels.reshape(-1).to(torch.int64)
            refs[done:done + n] = labels
            logits = outputs if outputs.dtype == F32 else outputs.float()
            if logits.is_cuda and L <= Fx.METRIC_MAX_L:
                Fx.cls_eval(logits, L, labels.contiguous(), conf, preds, done)
            else:
                p = logits.argmax(dim=-1)
                preds[done:done + n] = p
                ok = (labels >= 0) & (labels < L)
                conf += torch.bincount(labels[ok] * L + p[ok], minlength=L * L)
        done += n
    if preds is None:
        raise ValueError("evaluate: empty loader")
    if regression:
        if preds.is_cuda and 2 <= done <= Fx.CORR_MAX_N:
            corr = Fx.corr_rank(preds[:done], refs[:done])
            values = _read(torch.cat([corr, preds[:done].double()]))
            res = EvalResult(zip(TASK_METRICS[task], values[:2]))
            res.predictions = values[2:]
        else:
            values = _read(torch.cat([preds[:done].double(), refs[:done].double()]))
            res = EvalResult(zip(TASK_METRICS[task], correlations_host(values[:done], values[done:])))
            res.predictions = values[:done]
    else:
        values = _read(torch.cat([conf, preds[:done]]))
        res = EvalResult(metrics_from_confusion(task, values[:L * L]))
        res.confusion = [values[r * L:(r + 1) * L] for r in range(L)]
        res.predictions = values[L * L:]
    res.count = done
    return res


def train(model, train_loader, eval_loader, optimizer, lr_scheduler, device, config, accelerator, checkpointer, output_dir,
          mismatched_loader=None, train_sampler=None, print_freq=50, log=None):
    """run_glue.py:347-421: per epoch -- train, evaluate, on the main process a log.txt JSON line, and every `ckpt_frequent` epochs a
    checkpoint through `checkpointer.save_checkpoint(model_state={'model': state_dict, 'config': config}, epoch=..., training_states=
    optimizer.state_dict())`; for mnli the final pass over the mismatched validation set (:396-421).  Every rank evaluates the whole
    validation set (no collective).  Returns the list of per-epoch metric dicts (the mismatched pass last, under 'mnli-mm')."""
    history = []
    completed_steps = 0
    for epoch in range(config['num_train_epochs']):
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        stats, completed_steps = train_one_epoch(model, train_loader, optimizer, lr_scheduler, epoch, device, config, accelerator,
                                                 completed_steps=completed_steps, print_freq=print_freq, log=log)
        eval_metric = evaluate(model, eval_loader, device, config)
        print(f"epoch {epoch}: {dict(eval_metric)}", flush=True)
        history.append({"epoch": epoch, **eval_metric})
        if is_main_process():
            with open(os.path.join(output_dir, "log.txt"), "a") as f:
                f.write(json.dumps({**{f'train_{k}': "{:.5f}".format(v) for k, v in stats.items()},
                                    **{f'eval_{k}': v for k, v in eval_metric.items()}, 'epoch': epoch,
                                    'completed_steps': completed_steps}) + "\n")
            if (epoch + 1) % config['ckpt_frequent'] == 0 and checkpointer is not None:
                save_obj = {'model': unwrap(model).state_dict(), 'config': config}
                checkpointer.save_checkpoint(model_state=save_obj, epoch=epoch, training_states=optimizer.state_dict())
        if is_distributed():
            torch.distributed.barrier()
    if config['task_name'] == "mnli" and mismatched_loader is not None:
        eval_metric = evaluate(model, mismatched_loader, device, config)
        print(f"mnli-mm: {dict(eval_metric)}", flush=True)
        history.append({"epoch": "mnli-mm", **eval_metric})
        if is_main_process():
            with open(os.path.join(output_dir, "log.txt"), "a") as f:
                f.write(json.dumps({**{f'eval_{k}': v for k, v in eval_metric.items()}, 'epoch': "mnli-mm"}) + "\n")
    return history
