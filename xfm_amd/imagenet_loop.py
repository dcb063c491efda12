"""The ImageNet fine-tune / linear-probe task loop around the HIP step: the per-iteration cosine schedule, the training epoch, the
evaluation pass and the best-checkpoint loop of Imagenet.py.

Mirrors (names, argument meaning, ordering):
  * accuracy                 Imagenet.py:221-235   top-k accuracy in percent
  * adjust_learning_rate     Imagenet.py:241-257   linear warm-up, then half-cycle cosine, per iteration
  * train_one_epoch          Imagenet.py:437-492   (`train` there; `train` here is the epoch loop of main())
  * evaluate                 Imagenet.py:495-536
  * create_optimizer         Imagenet.py:565-574
  * create_mixup / create_criterion   Imagenet.py:592-611
  * train                    Imagenet.py:614-637
What differs, on purpose: the reference reads the loss with `.item()` after every training step (:477) and the loss and two accuracies
after every validation batch (:521-523).  Here the training losses are parked (task.LossMeters) and read when a log line is
due, and the evaluation adds its three sums on the device (xfm_ce_topk_eval) into one buffer that is read ONCE at the end."""
import math
import os

import torch

from . import functional as Fx
from .task import LossMeters, is_distributed, is_main_process, to_device, unwrap
from .task import read as _read  # the loop's single device-to-host read (evaluate calls it once per pass; the tests count its calls)

F32 = torch.float32


def adjust_learning_rate(optimizer, epoch, config):
    """Imagenet.py:241-257: decay the learning rate with half-cycle cosine after warm-up; a group's `lr_scale` multiplies it."""
    warmup_epochs = config['schedular']['warmup_epochs']
    epochs = config['schedular']['epochs']
    peak_lr = config['schedular']['lr']
    min_lr = config['schedular']['min_lr']
    if epoch < warmup_epochs:
        lr = peak_lr * epoch / warmup_epochs
    else:
        lr = min_lr + (peak_lr - min_lr) * 0.5 * (1. + math.cos(math.pi * (epoch - warmup_epochs) / (epochs - warmup_epochs)))
    for param_group in optimizer.param_groups:
        if "lr_scale" in param_group:
            param_group["lr"] = lr * param_group["lr_scale"]
        else:
            param_group["lr"] = lr
    return lr


def _topk_sums(output, target, k1, k2, acc):
    """acc [3] += (sum of CE rows, #{label in top k1}, #{label in top k2}) of one batch: the kernel on a GPU fp32 batch, the plain torch
    form elsewhere (stable sort: the kernel's tie rule)."""
    if output.is_cuda and output.dtype == F32 and output.dim() == 2 and output.stride(1) == 1:
        Fx.ce_topk_eval(output, output.shape[1], target.reshape(-1).to(torch.int64).contiguous(), k1, k2, acc)
        return
    out = output.float()
    rows = torch.nn.functional.cross_entropy(out, target, reduction='none')
    order = torch.sort(out, dim=1, descending=True, stable=True).indices
    rank = (order == target.view(-1, 1)).float().argmax(dim=1)
    acc += torch.stack([rows.sum(), (rank < k1).sum().float(), (rank < k2).sum().float()]).to(acc.dtype)


def accuracy(output, target, topk=(1,)):
    """Imagenet.py:221-235: the accuracy over the k top predictions for the given k -> a list of one-element tensors, in percent.
    A GPU fp32 `output` with one or two k goes through xfm_ce_topk_eval (no topk / eq / sum launches); anything else takes the
    reference's torch form."""
    with torch.no_grad():
        batch_size = target.size(0)
        if output.is_cuda and output.dtype == F32 and 1 <= len(topk) <= 2 and output.dim() == 2 and output.stride(1) == 1 \
                and list(topk) == sorted(topk) and max(topk) <= output.shape[1]:
            acc = torch.zeros(3, dtype=F32, device=output.device)
            _topk_sums(output, target, topk[0], topk[-1], acc)
            return [acc[1 + i:2 + i].mul(100.0 / batch_size) for i in range(len(topk))]
        maxk = max(topk)
        _, pred = output.topk(maxk, 1, True, True)
        pred = pred.t()
        correct = pred.eq(target.view(1, -1).expand_as(pred))
        res = []
        for k in topk:
            correct_k = correct[:k].reshape(-1).float().sum(0, keepdim=True)
            res.append(correct_k.mul_(100.0 / batch_size))
        return res


def create_optimizer(config, model):
    """Imagenet.py:565-574.  `adamW` is torch.optim.AdamW(parameters, lr=...) with torch's defaults -- ONE group, betas (0.9, 0.999),
    eps 1e-8, weight decay 0.01 on every tensor; the config's `weight_decay` is not passed (:570).  The `adamw_rule="torch"` marker
    (defaults and the group) tells RCCLDDPAccelerator to step with torch's rule (xfm_adamw_torch), not the transformers rule that
    optim.py's optimizer stands for."""
    parameters = list(filter(lambda p: p.requires_grad, model.parameters()))
    opt = config['optimizer']['opt']
    if opt == 'lars':
        raise NotImplementedError("optimizer.opt == 'lars' (Imagenet.py:567-568) is not built: no shipped config sets it")
    if opt != 'adamW':
        raise NotImplementedError(f"optimizer.opt == {opt!r}: SGD (Imagenet.py:571-574) is not built: no shipped config sets it")
    optimizer = torch.optim.AdamW(parameters, lr=config['optimizer']['lr'])
    optimizer.defaults["adamw_rule"] = "torch"
    for g in optimizer.param_groups:
        g["adamw_rule"] = "torch"
    return optimizer


def create_mixup(config):
    """Imagenet.py:592-600: Mixup / CutMix when the config asks for it and the run is not a linear probe; else None."""
    is_lp = config.get('is_lp', False)
    mixup_active = (config['mixup'] > 0 or config['cutmix'] > 0. or config['cutmix_minmax'] is not None) and not is_lp
    if not mixup_active:
        return None
    from .mixup import Mixup
    return Mixup(mixup_alpha=config['mixup'], cutmix_alpha=config['cutmix'], cutmix_minmax=config['cutmix_minmax'],
                 prob=config['mixup_prob'], switch_prob=config['mixup_switch_prob'], mode=config['mixup_mode'],
                 label_smoothing=config['smoothing'], num_classes=config['num_labels'])


def create_criterion(config, mixup_fn):
    """Imagenet.py:605-611: soft targets behind Mixup (the smoothing is in its label transform), else label smoothing, else plain CE."""
    if mixup_fn is not None:
        from .losses import SoftTargetCrossEntropy
        return SoftTargetCrossEntropy()
    if config['smoothing'] > 0.:
        from .losses import LabelSmoothingCrossEntropy
        return LabelSmoothingCrossEntropy(smoothing=config['smoothing'])
    return torch.nn.CrossEntropyLoss()


def train_one_epoch(model, loader, optimizer, criterion, epoch, mixup_fn, device, config, accelerator, print_freq=50, log=None):
    """Imagenet.py:437-492 (`train`): per iteration -- lr from i / len(loader) + epoch, upload, Mixup, model(images, None, None, None,
    False), criterion on the logits, zero_grad / backward / step through the accelerator.  The loss tensors are parked and read when a
    log line is due (every `print_freq` iterations, :491-492).  Returns the epoch's meters."""
    model.train()
    meters = LossMeters()
    n = len(loader)
    for i, (images, target) in enumerate(loader):
        adjust_learning_rate(optimizer, i / n + epoch, config)   # FROM MAE: a per-iteration (not per-epoch) schedule (:457-458)
        images = to_device(device, images)
        if config.get('task_name') == 'kitti':
            target = target['type']
        target = to_device(device, target)
        if mixup_fn is not None:
            images, target = mixup_fn(images, target)
        output = model(images, None, None, None, False)
        loss = criterion(output, target)
        meters.update(loss=loss, lr=optimizer.param_groups[0]["lr"])
        optimizer.zero_grad()
        accelerator.backward_step(loss, optimizer)
        accelerator.optimizer_step(optimizer, model)
        if i % print_freq == 0:
            meters.flush()
            if log is not None:
                log(epoch, i, meters.global_avg())
    return meters.global_avg()


class EvalResult(float):
    """evaluate()'s return value: top1.avg as the reference returns it (a float), with the pass's other figures attached."""
    loss_avg = acc1 = acc2 = 0.0
    count = 0


@torch.no_grad()
def evaluate(model, loader, device, log=None):
    """Imagenet.py:495-536: model.eval(), CrossEntropyLoss and accuracy(topk=(1, 2)) -- as the reference actually calls it -- over the
    validation loader.  AverageMeter's sample-weighted means (batch mean x batch size, summed, over the sample count) are sums over
    samples: every batch adds its three sums into ONE device buffer, read once at the end.  Returns top1.avg; the result also
    carries (.loss_avg, .acc1, .acc2) and .count."""
    model.eval()
    acc = None
    count = 0
    for images, target in loader:
        images, target = to_device(device, (images, target))
        output = model(images, None, None, None, False)
        if acc is None:
            acc = torch.zeros(3, dtype=F32, device=output.device)
        _topk_sums(output.float() if output.dtype != F32 else output, target, 1, 2, acc)
        count += images.size(0)
    if acc is None:
        raise ValueError("evaluate: empty loader")
    loss_sum, n1, n2 = _read(acc)
    res = EvalResult(100.0 * n1 / count)
    res.loss_avg, res.acc1, res.acc2, res.count = loss_sum / count, 100.0 * n1 / count, 100.0 * n2 / count, count
    msg = ' * Acc@1 {:.3f} Acc@5 {:.3f}'.format(res.acc1, res.acc2)   # (the reference's line, :533-534: its "Acc@5" meter holds top-2)
    (log or print)(msg)
    return res


def train(model, train_loader, val_loader, optimizer, criterion, mixup_fn, device, config, accelerator, output_dir, train_sampler=None,
          print_freq=50, log=None):
    """Imagenet.py:614-637: per epoch -- train, evaluate, and on rank 0 save checkpoint_best.pth (model / optimizer / config / epoch) when
    the accuracy improved.  optimizer.state_dict() carries the fused AdamW moments in torch's own format
    (RCCLDDPAccelerator._publish_optimizer_state).  Returns (best_acc1, best_epoch)."""
    base = unwrap(model)
    best_acc1, best_epoch = 0, 0
    for epoch in range(0, config['schedular']['epochs']):
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        train_one_epoch(model, train_loader, optimizer, criterion, epoch, mixup_fn, device, config, accelerator, print_freq=print_freq,
                        log=log)
        acc1 = evaluate(model, val_loader, device)
        if is_main_process():
            is_best = acc1 > best_acc1
            best_acc1 = max(float(acc1), best_acc1)
            if is_best:
                best_epoch = epoch
                save_obj = {'model': base.state_dict(), 'optimizer': optimizer.state_dict(), 'config': config, 'epoch': epoch}
                torch.save(save_obj, os.path.join(output_dir, 'checkpoint_best.pth'))
                print("best_acc1 = ", best_acc1, flush=True)
        if is_distributed():
            torch.distributed.barrier()
    return best_acc1, best_epoch
