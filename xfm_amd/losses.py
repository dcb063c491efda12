"""The two criteria of the ImageNet fine-tune step (Imagenet.py:605-609) under timm's names and call forms, each one autograd
function over the soft cross-entropy kernels (xfm_ce_soft_* / xfm_ce_smooth_*): no ATen log_softmax, no dense smoothed target, no
host sync."""
import torch
from torch import nn

from . import functional as Fx

F32 = torch.float32


def _rows4(t, C):
    """fp32 [R, ld] copy / view of t [..., C] for the row kernels: they read 16-byte granules, so a width that is not a multiple of 4
    goes into a padded buffer (the way ops._SmallCEFn does; the padding is never read into a result)."""
    t = t.reshape(-1, C).float().contiguous()
    if C >= 4 and C % 4:
        padded = torch.zeros((t.shape[0], (C + 3) // 4 * 4), dtype=F32, device=t.device)
        padded[:, :C] = t
        t = padded
    return t


class _SoftTargetCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        C = logits.shape[-1]
        assert target.shape == logits.shape, (target.shape, logits.shape)
        lg, tg = _rows4(logits, C), _rows4(target, C)
        lse, tsum, rows = Fx.ce_soft_fwd(lg, C, tg)
        ctx.save_for_backward(lg, tg, lse, tsum)
        ctx.C, ctx.shape, ctx.dtype = C, logits.shape, logits.dtype
        return rows.sum() / rows.numel()

    @staticmethod
    def backward(ctx, g):
        lg, tg, lse, tsum = ctx.saved_tensors
        C = ctx.C
        d = Fx.ce_soft_bwd(lg, C, tg, lse, tsum, (g.float() / lg.shape[0]).reshape(1), (C + 7) // 8 * 8)
        return d[:, :C].to(ctx.dtype).reshape(ctx.shape), None


class _LabelSmoothCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, smoothing):
        C = logits.shape[-1]
        lg = _rows4(logits, C)
        labels = labels.reshape(-1).contiguous()
        off = smoothing / C
        on = 1.0 - smoothing + off
        lse, rows = Fx.ce_smooth_fwd(lg, C, labels, on, off)
        ctx.save_for_backward(lg, labels, lse)
        ctx.C, ctx.shape, ctx.dtype, ctx.on_off = C, logits.shape, logits.dtype, (on, off)
        return rows.sum() / rows.numel()

    @staticmethod
    def backward(ctx, g):
        lg, labels, lse = ctx.saved_tensors
        C = ctx.C
        d = Fx.ce_smooth_bwd(lg, C, labels, *ctx.on_off, lse, (g.float() / lg.shape[0]).reshape(1), (C + 7) // 8 * 8)
        return d[:, :C].to(ctx.dtype).reshape(ctx.shape), None, None


class SoftTargetCrossEntropy(nn.Module):
    """timm.loss.SoftTargetCrossEntropy (Imagenet.py:605-607, the criterion behind Mixup): mean over rows of
    sum(-target * log_softmax(x, -1), -1).  Logits of any float dtype and class count; target of the same shape (Mixup's output),
    non-negative, any row sum, no gradient.  The gradient comes back in the logits' dtype."""

    def forward(self, x, target):
        return _SoftTargetCEFn.apply(x, target)


class LabelSmoothingCrossEntropy(nn.Module):
    """timm.loss.LabelSmoothingCrossEntropy (Imagenet.py:608-609, mixing off): mean over rows of
    (1 - smoothing) * nll + smoothing * mean(-log_softmax) = F.cross_entropy(x, labels, label_smoothing=smoothing).  The smoothed
    row is never built (label-form kernel: on = 1 - s + s / C, off = s / C).  Like timm's, the mean is over ALL rows; a label of -100
    contributes 0 to it."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing

    def forward(self, x, target):
        return _LabelSmoothCEFn.apply(x, target, self.smoothing)
