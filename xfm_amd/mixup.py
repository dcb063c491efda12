"""timm.data.Mixup for device batches (Imagenet.py:597-600 builds it, :468-469 calls it): the mixing parameters are drawn on the host
from numpy.random as timm draws them, one small pinned upload carries them, and the batch and its soft target are produced by two
kernels (xfm_mixup: one in-place pass over the images; xfm_mixup_target) instead of flip / mul_ / mul_ / add_ and two one_hot
scatters.  No device sync."""
import numpy as np
import torch

from . import functional as Fx


class Mixup:
    """Mixup / CutMix with timm's constructor keywords.  `mode` 'batch' (one draw for the whole batch) and 'elem' (the same draw per
    row; timm vectorises its per-row draws, so the numpy stream is consumed in another order) are built; 'pair' and `cutmix_minmax`
    raise NotImplementedError -- no shipped config sets them.  A CutMix draw whose box comes out empty changes no pixel, and its lam is
    1 here whether or not `correct_lam` is set."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        if cutmix_minmax is not None:
            raise NotImplementedError("Mixup: cutmix_minmax (the min/max box ratio form of CutMix) is not built")
        if mode == 'pair':
            raise NotImplementedError("Mixup: mode='pair' is not built (modes: 'batch', 'elem')")
        if mode not in ('batch', 'elem'):
            raise ValueError(f"Mixup: unknown mode {mode!r}")
        self.mixup_alpha, self.cutmix_alpha = mixup_alpha, cutmix_alpha
        self.mix_prob, self.switch_prob = prob, switch_prob
        self.label_smoothing, self.num_classes = label_smoothing, num_classes
        self.mode, self.correct_lam = mode, correct_lam
        self.mixup_enabled = True   # timm's switch: set False to pass batches through

    def _draw_one(self, H, W):
        """-> (lam, (yl, yh, xl, xh)): timm's _params_per_batch followed by its rand_bbox / cutmix_bbox_and_lam."""
        lam, box = 1., (0, 0, 0, 0)
        if not self.mixup_enabled or not np.random.rand() < self.mix_prob:
            return lam, box
        if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
            use_cutmix = bool(np.random.rand() < self.switch_prob)
            alpha = self.cutmix_alpha if use_cutmix else self.mixup_alpha
        elif self.mixup_alpha > 0.:
            use_cutmix, alpha = False, self.mixup_alpha
        elif self.cutmix_alpha > 0.:
            use_cutmix, alpha = True, self.cutmix_alpha
        else:
            raise ValueError("One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true.")
        lam = float(np.random.beta(alpha, alpha))
        if use_cutmix and lam != 1.:   # (timm draws no box at lam == 1 either)
            ratio = np.sqrt(1 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy, cx = np.random.randint(0, H), np.random.randint(0, W)
            yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
            xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
            area = (yh - yl) * (xh - xl)
            if area == 0:
                return 1., (0, 0, 0, 0)
            box = (yl, yh, xl, xh)
            if self.correct_lam:
                lam = 1. - area / float(H * W)
        return lam, box

    def draw(self, B, H, W):
        """The host side of one call -> (lam float32 [B], box int32 [B, 4] = yl, yh, xl, xh; an empty box = mixup).  Separate from
        __call__ so that parameters can be injected (override or replace this method)."""
        lam, box = np.ones(B, dtype=np.float32), np.zeros((B, 4), dtype=np.int32)
        if self.mode == 'batch':
            lam[:], box[:] = self._draw_one(H, W)
        else:
            for i in range(B):
                lam[i], box[i] = self._draw_one(H, W)
        return lam, box

    def __call__(self, x, target):
        B, _, H, W = x.shape
        if B % 2:
            raise AssertionError("Batch size should be even when using this")
        lam, box = self.draw(B, H, W)
        words = torch.empty(5 * B, dtype=torch.int32, pin_memory=True)   # lam | box in one upload
        host = words.numpy()
        host[:B] = np.ascontiguousarray(lam, dtype=np.float32).view(np.int32)
        host[B:] = np.ascontiguousarray(box, dtype=np.int32).reshape(-1)
        dev = words.to(x.device, non_blocking=True)
        lam_d, box_d = dev[:B].view(torch.float32), dev[B:].view(B, 4)
        Fx.mixup_(x, lam_d, box_d)
        soft = Fx.mixup_target(target.reshape(-1).to(torch.int64).contiguous(), lam_d, self.num_classes, self.label_smoothing)
        return x, soft
