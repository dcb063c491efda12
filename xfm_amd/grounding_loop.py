"""The referring-expression grounding fine-tune / evaluation task loop around the HIP step: the training epoch, the box-accuracy
evaluation pass and the per-epoch evaluate / best-checkpoint loop of Grounding_bbox.py.

Mirrors (names, argument meaning, ordering):
  * train_one_epoch   Grounding_bbox.py:39-70    (`train` there; `train` here is the epoch loop of main())
  * evaluation        Grounding_bbox.py:73-93 (`val`) + dataset/utils.py:155-175 collect_tensor_result + :271-345 grounding_eval_bbox /
                      grounding_eval_bbox_vlue + :349-361 computeIoU
  * train             Grounding_bbox.py:200-242
The optimizer (four AdamW groups, `lr_mult` on model.init_params) and the linear warm-up / decay schedule are the pre-training loop's
(pretrain_loop.create_optimizer / create_scheduler = optim.py / scheduler.py, which Grounding_bbox.py:189-193 calls); the step runs
through RCCLDDPAccelerator on the transformers-rule xfm_adamw.
What differs, on purpose:
  * the batches carry TOKEN IDS -- an expression is an (input_ids, attention_mask) pair where the reference tokenizes strings (:52, :83);
    there is no tokenizer and no dataset code on this path;
  * the reference reads both losses with `.item()` after every step (:63-64); here the loss tensors are parked (task.LossMeters) and read
    when a log line is due.  On HIP tensors the model runs with `fused=True`: the two losses are one kernel each way (xfm_box_loss_fwd /
    xfm_box_loss_bwd) in place of about 30 ATen launches;
  * the reference keeps every prediction as a Python record (:90-91), saves and reloads them, then moves each one to the device and back
    and computes its IoU in Python (utils.py:281-288).  Here the ground truth -- the loader's `dataset` carries `ref_box` [R, 4],
    `ref_size` [R, 2], `ref_split` [R] and `ref_index` (ref_id -> row) in place of the REFER object -- is uploaded once, every batch runs
    xfm_box_eval behind the previous batch's rows, and the [3, 2] counts buffer is read ONCE per pass;
  * on one node every rank evaluates the whole synthetic test set: the per-rank result files of collect_tensor_result and their merge are
    not built (nor its HDFS copy).
`box_eval_host` is this module's host form of the kernel's arithmetic (numpy fp64): evaluation() uses it only where the tensors are on the
CPU, where there is no device to run the kernel on."""
import json
import os

import numpy as np
import torch

from .task import LossMeters, is_distributed, is_main_process, to_device, unwrap
from .task import read as _read  # the loop's single device-to-host read (evaluation calls it once per pass; the tests count its calls)

SPLITS = ('val', 'testA', 'testB')   # the rows of the counts buffer (ref['split'], utils.py:290-301)


def train_one_epoch(model, data_loader, optimizer, epoch, device, scheduler, config, accelerator, print_freq=50, log=None):
    """Grounding_bbox.py:39-70 (`train`): per iteration -- upload, (_, loss_bbox, loss_giou) = model(image, ids, atts, target_bbox=...),
    loss = loss_bbox + loss_giou, backward and step through the accelerator, scheduler.step().  A batch is (image, (text_ids, text_atts),
    target_bbox).  Returns the epoch's meters formatted as the reference does (:70)."""
    model.train()
    meters = LossMeters()
    for i, (image, text, target_bbox) in enumerate(data_loader):
        image, (text_ids, text_atts), target_bbox = to_device(device, (image, text, target_bbox))
        if image.is_cuda:
            _, loss_bbox, loss_giou = model(image, text_ids, text_atts, target_bbox=target_bbox, fused=True)
        else:   # (a CPU model path has no kernels to fuse onto)
            _, loss_bbox, loss_giou = model(image, text_ids, text_atts, target_bbox=target_bbox)
        loss = loss_bbox + loss_giou
        meters.update(loss_bbox=loss_bbox, loss_giou=loss_giou, lr=optimizer.param_groups[0]["lr"])
        accelerator.backward_step(loss, optimizer)
        accelerator.optimizer_step(optimizer, model)
        scheduler.step()
        optimizer.zero_grad()
        if i % print_freq == 0:
            meters.flush()
            if log is not None:
                log(epoch, i, meters.global_avg())
    avg = meters.global_avg()
    print("Averaged stats:", {k: round(v, 6) for k, v in avg.items()}, flush=True)
    return {k: "{:.5f}".format(v) for k, v in avg.items()}


def box_eval_host(coord, ref_row, ref_box, ref_size, ref_split):
    """xfm_box_eval's arithmetic on the host, numpy fp64 from the fp32 inputs: coord [n, 4] (cx, cy, w, h) in [0, 1], ref_row [n] (or
    None = rows 0 .. n - 1) into ref_box [R, 4] (x, y, w, h in pixels), ref_size [R, 2] (width, height), ref_split [R].
    -> (out fp64 [n, 5] = (x, y, w, h in pixels, IoU), counts int64 [3, 2] = (#IoU >= 0.5, #samples) per split).  A row outside the tables
    gives a NaN out row and is counted nowhere; union <= 0 gives IoU 0."""
    coord = np.asarray(coord, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    ref_box = np.asarray(ref_box, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    ref_size = np.asarray(ref_size, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    ref_split = np.asarray(ref_split).reshape(-1)
    n, R = coord.shape[0], ref_box.shape[0]
    rows = np.arange(n) if ref_row is None else np.asarray(ref_row).reshape(-1)
    out = np.full((n, 5), np.nan)
    counts = np.zeros((3, 2), dtype=np.int64)
    for i in range(n):
        r = int(rows[i])
        if r < 0 or r >= R:
            continue
        W, H = ref_size[r]
        rx, ry, rw, rh = ref_box[r]
        pw, ph = coord[i, 2] * W, coord[i, 3] * H
        px, py = coord[i, 0] * W - pw / 2, coord[i, 1] * H - ph / 2
        x1, y1 = max(rx, px), max(ry, py)
        x2, y2 = min(rx + rw - 1, px + pw - 1), min(ry + rh - 1, py + ph - 1)
        inter = (x2 - x1 + 1) * (y2 - y1 + 1) if x1 < x2 and y1 < y2 else 0.0
        union = rw * rh + pw * ph - inter
        iou = 0.0 if union <= 0 else inter / union
        out[i] = (px, py, pw, ph, iou)
        s = int(ref_split[r])
        if 0 <= s < 3:
            counts[s, 1] += 1
            counts[s, 0] += int(iou >= 0.5)
    return out, counts


def grounding_acc(counts, config):
    """The accuracy dict of grounding_eval_bbox (utils.py:303) -- or of grounding_eval_bbox_vlue (:340) when config['vlue_test'], where
    every sample counts as one split -- from the [3, 2] counts.  An empty split divides by zero, as the reference does."""
    if config.get('vlue_test'):
        eval_result = {'score': sum(c for c, _ in counts) / sum(n for _, n in counts)}
    else:
        eval_result = {f'{name}_d': counts[s][0] / counts[s][1] for s, name in enumerate(SPLITS)}
    for metric, acc in eval_result.items():
        print(f'{metric}: {acc:.3f}', flush=True)
    return eval_result


@torch.no_grad()
def evaluation(model, data_loader, device, config, result_dir=None, filename=None):
    """Grounding_bbox.py:73-93 + grounding_eval_bbox: predict a box for every test expression and count the IoU >= 0.5 hits per split.
    The three ref tables are uploaded once; every batch writes its (x, y, w, h, IoU) rows behind the previous batch's in one fp32 device
    buffer and adds into one int64 [3, 2] counts buffer, read ONCE at the end.  A batch is (image, (text_ids, text_atts), ref_ids).
    With `result_dir` the [N, 5] buffer is copied out once more and saved with the ref ids as <result_dir>/<filename>.pth.  Returns
    {'val_d', 'testA_d', 'testB_d'}, or {'score'} when config['vlue_test']."""
    from . import functional as Fx
    model.eval()
    dataset = data_loader.dataset
    ref_box, ref_size, ref_split = to_device(device, (dataset.ref_box.float().contiguous(), dataset.ref_size.float().contiguous(),
                                                      dataset.ref_split.to(torch.int32).contiguous()))
    ref_index = dataset.ref_index
    n_max = len(data_loader) * config['batch_size']   # one row per expression: len(loader) batches of at most batch_size
    out = torch.full((n_max, 5), float('nan'), dtype=torch.float32, device=device)
    counts = torch.zeros(3, 2, dtype=torch.int64, device=device)
    ref_ids, done = [], 0
    for image, text, ref_id in data_loader:
        image, (text_ids, text_atts) = to_device(device, (image, text))
        outputs_coord = model(image, text_ids, text_atts, target_bbox=None)
        n = outputs_coord.shape[0]
        ids = [int(r) for r in (ref_id.tolist() if torch.is_tensor(ref_id) else ref_id)]   # (host tensors)
        assert len(ids) == n and done + n <= n_max   # :88
        rows = torch.tensor([ref_index.get(r, -1) for r in ids], dtype=torch.int32)
        if outputs_coord.is_cuda:
            Fx.box_eval(outputs_coord.float().contiguous(), rows.to(device, non_blocking=True), ref_box, ref_size, ref_split, counts, out, done)
        else:   # no device: the documented host form
            o, c = box_eval_host(outputs_coord.float().numpy(), rows.numpy(), ref_box.numpy(), ref_size.numpy(), ref_split.numpy())
            out[done:done + n] = torch.from_numpy(o).float()
            counts += torch.from_numpy(c)
        ref_ids.extend(ids)
        done += n
    acc = grounding_acc(_read(counts), config)
    if result_dir is not None and is_main_process():
        os.makedirs(result_dir, exist_ok=True)
        torch.save({'ref_id': ref_ids, 'pred': out[:done].cpu()}, os.path.join(result_dir, '%s.pth' % filename))
    return acc


def train(model, train_loader, test_loader, optimizer, device, scheduler, config, accelerator, checkpointer, output_dir, result_dir,
          train_sampler=None, print_freq=50, log=None, evaluate=None):
    """Grounding_bbox.py:200-242: per epoch -- train, evaluate (the rows go to <result_dir>/epoch<N>.pth), on the main process a log.txt
    line and, whenever val_d beats the best so far, `checkpointer.save_checkpoint(model_state=..., epoch='best', training_states=...)`
    (optimizer.state_dict() carries the fused AdamW moments in torch's format); then the closing `best epoch: %d`.  `evaluate` stands in
    for evaluation() (same arguments).  Returns (best, best_epoch)."""
    evaluate = evaluate or evaluation
    max_epoch = config['schedular']['epochs']
    best = 0
    best_epoch = 0
    for epoch in range(0, max_epoch):
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        train_stats = train_one_epoch(model, train_loader, optimizer, epoch, device, scheduler, config, accelerator, print_freq=print_freq,
                                      log=log)
        # (one node: every rank evaluates the whole synthetic test set; collect_tensor_result's merge is not needed)
        acc = evaluate(unwrap(model), test_loader, device, config, result_dir=result_dir, filename='epoch%d' % epoch)
        if is_main_process():
            log_stats = {**{f'train_{k}': v for k, v in train_stats.items()}, **{f'{k}': v for k, v in acc.items()}, 'epoch': epoch}
            if acc['val_d'] > best:
                save_obj = {'model': unwrap(model).state_dict(), 'config': config}
                if checkpointer is not None:
                    checkpointer.save_checkpoint(model_state=save_obj, epoch='best', training_states=optimizer.state_dict())
                best = acc['val_d']
                best_epoch = epoch
            with open(os.path.join(output_dir, "log.txt"), "a") as f:
                f.write(json.dumps(log_stats) + "\n")
        if is_distributed():
            torch.distributed.barrier()
    if is_main_process():
        with open(os.path.join(output_dir, "log.txt"), "a") as f:
            f.write("best epoch: %d" % best_epoch)
    return best, best_epoch
