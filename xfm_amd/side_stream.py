"""The second HIP stream of a launch stream: weight-gradient GEMMs, K/V pre-projections and parameter-gradient folds that nothing on
the activation chain waits for (every tower, the stand-alone ops, the ViT trunk and the data-parallel accelerator use it)."""
import contextlib
import os

import torch

from . import functional as Fx
from . import marks as _marks


class _DeferredCall:
    """One-shot work of a _WgradStream flush."""
    persistent = False

    def __init__(self, fn, keep=()):
        self.fn, self.keep = fn, tuple(keep)

    def run(self):
        self.fn()


class _WgradStream:
    """Weight-gradient GEMMs of a tower's backward on a second HIP stream.  dW only feeds the optimizer / all-reduce, so the
    dY^T X products need not sit on the activation-gradient critical path: at the fusion / text towers' sizes (M = 7680 / 1920 rows)
    neither the dgrad nor the wgrad kernels fill the 256 CUs on their own, and the two chains overlap.  Every launch waits for an
    event recorded on the main stream after its dY was produced; the tensors it reads are kept alive until the main stream has
    re-joined (the caching allocator reuses freed blocks in main-stream order only)."""
    _streams = {}
    enabled = os.environ.get("XFM_WGRAD_STREAM", "1") != "0"
    priority = int(os.environ.get("XFM_WGRAD_PRIO", "0"))  # HIP stream priority of the second stream (lower number = served first)

    @classmethod
    def side_of(cls, device, launch):
        """The side stream of (device, launch stream), created on first use.  One per LAUNCH stream: the text tower's backward runs on
        its own stream next to the ViT's, and its small weight gradients must not queue (FIFO) behind the ViT's grouped launch on a
        shared side stream."""
        key = (device.index if device.index is not None else torch.cuda.current_device(), launch.cuda_stream)
        if key not in cls._streams:
            cls._streams[key] = torch.cuda.Stream(device=device, priority=cls.priority)
        return cls._streams[key]

    @classmethod
    def sides(cls, device_index):
        """{launch stream handle: side stream} of the side streams that exist on a device (creates none)."""
        return {launch: side for (d, launch), side in list(cls._streams.items()) if d == device_index}

    def __init__(self, device, label=None):
        self.label = label
        if label is not None:
            _marks.mark(label + " begin")
        self.main = torch.cuda.current_stream(device)
        if label is not None:   # a tower's backward starts: its gradient writes must follow a pending asynchronous zero_grad (arena.grads_ready)
            from .arena import grads_ready
            grads_ready(device)
        self.on = _WgradStream.enabled
        if self.on:
            self.side = _WgradStream.side_of(device, self.main)
            self.side.wait_stream(self.main)  # arena state (zeroed grads, earlier kernels) is visible to the side stream
        self.keep = []
        self.queue = []
        self.reduces = []

    def _hand_over(self, keep):
        """The side stream waits for everything enqueued on the main stream so far and `keep` (what the work touches) is held until the
        re-join -> the context under which the work is launched on the side stream.  Single-stream mode: launched in place."""
        if not self.on:
            return contextlib.nullcontext()
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.side.wait_event(ev)
        self.keep.append(keep)
        return torch.cuda.stream(self.side)

    def defer_tn(self, dy, x, dw, dbias=None):
        """Queue dw += dy^T @ x (dbias += column sums of dy) for the next flush(): everything queued -- all over the same M rows --
        runs as ONE grouped launch (Fx.gemm_tn_group: whole 256 x 256 tiles with one owner each instead of 7 M-split planes and a
        reduce per projection; the 48 weight gradients of the ViT trunk: 5.2 -> 3.9 ms).  The queue holds dy / x alive."""
        self.queue.append((dy, x, dw, dbias))

    def defer_call(self, fn, keep=()):
        """fn() runs with the next flush() (second stream, after everything the launch stream holds then): parameter-gradient kernels
        that nothing on the activation-gradient chain waits for (the relative-position table gradients of the ViT blocks, the batched
        LayerNorm folds of the layer executor).  `keep`: the tensors it touches."""
        self.reduces.append(_DeferredCall(fn, keep))

    def defer_reduces(self, rq):
        """A Fx.ReduceQueue: whatever LayerNorm backward kernels have queued on it is folded by every flush() until the join."""
        self.reduces.append(rq)

    def flush(self):
        reduces = self.reduces
        self.reduces = [r for r in reduces if getattr(r, "persistent", False)]   # a ReduceQueue stays registered (more kernels will append to it)
        items, self.queue = self.queue, []
        if not (reduces or items):
            return
        by_m = {}
        for it in items:   # one grouped launch per distinct row count (a tower's projections share M; the K/V projections of the image states
            by_m.setdefault(it[0].shape[0], []).append(it)   # and the pruned last layer have their own)
        with self._hand_over((items, reduces)):
            for r in reduces:
                r.run()
            for group in by_m.values():
                Fx.gemm_tn_group(group)

    def gemm_tn(self, dy, x, dw, **kw):
        with self._hand_over((dy, x)):
            Fx.gemm_tn(dy, x, dw, **kw)

    def project(self, x, slot):
        """x @ slot.W^T + b on the side stream; returns (tensor, event) for take()."""
        if not self.on:
            return Fx.gemm_nt(x, slot.wb, slot.b), None
        with torch.cuda.stream(self.side):
            y = Fx.gemm_nt(x, slot.wb, slot.b)
            ev = torch.cuda.Event()
            ev.record(self.side)
        y.record_stream(self.main)  # allocated on the side stream, consumed on the main one
        return y, ev

    def take(self, pair):
        y, ev = pair
        if ev is not None:
            self.main.wait_event(ev)
        return y

    def run(self, fn, keep=()):
        """fn() on the side stream, after everything enqueued on the main stream so far; `keep` = the tensors it touches."""
        with self._hand_over(tuple(keep)):
            return fn()

    def sync_side(self):
        """The launch stream waits for what the second stream has been given so far (queued weight gradients are not launched)."""
        if self.on:
            self.main.wait_stream(self.side)

    def join_at_end(self):
        """Like join(), but the launch stream re-joins when the whole backward pass is over (an engine callback, as
        model_pretrain._JoinAfterBackward): the weight gradients given to the second stream here need not finish before the NEXT node's
        activation gradients start -- only before anyone reads the parameter gradients.  Only inside a backward pass."""
        self.flush()
        if self.on:
            main, side, keep = self.main, self.side, self.keep

            def rejoin():
                main.wait_stream(side)
                # the callback runs on the thread (and current stream) that called backward(): if this node ran on another stream (the
                # text tower's, replayed by autograd), that caller -- the optimizer, the gradient norm, the final all-reduce -- must wait
                # for these weight gradients too, whatever order the end-of-backward callbacks run in
                cur = torch.cuda.current_stream(main.device)
                if cur != main:
                    cur.wait_stream(side)
                keep.clear()
            torch.autograd.Variable._execution_engine.queue_callback(rejoin)
            self.keep = []
        else:
            self.keep.clear()

    def join(self):
        if self.label is not None:
            _marks.mark(self.label + " chain end")
        self.flush()
        if self.on:
            self.main.wait_stream(self.side)
        self.keep.clear()
        if self.label is not None:
            _marks.mark(self.label + " end")
