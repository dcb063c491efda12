"""What the three vision towers share: `beit2.VisionTransformer` (BEiT v2), `vit.VisionTransformer` (plain ViT) and
`model_vqkd.TokenizerEncoder` (the VQ-KD tokenizer's encoder).

`_TrunkFn` runs a tower's blocks and its final LayerNorm as ONE autograd node whose forward / backward are explicit sequences of C-ABI
kernel launches (xfm_amd.functional).  `_FusedViT` is the towers' base: it declares, as class attributes, everything the node asks a
tower, and owns the arena plumbing, the patch-token step and the drop-path draw.  `_Affine`, `_Dense` and `PatchEmbed` are the
parameter containers (the arithmetic runs in the fused kernels).
"""
import math
import os

import torch
import torch.nn as nn

from . import _lib
from . import functional as Fx
from .arena import LinearSlot, OwnsArena, ParamArena, arena_note_grad, arena_note_use, grad_of
from .ops import linear_slot
from .side_stream import _WgradStream

# XFM_ATTN_FAST_DELTA=1: the attention backward takes delta = dO . O from the forward's output (kept as bf16 hi + lo halves) instead of a
# first pass over the keys: dQ kernel 198 -> 165 us, forward 69 -> 80 us at B = 128 (tools/bench_attn.py), the step unchanged within
# noise (41.6 vs 41.5 ms, tools/ab.sh) -- off by default, the exact two-pass form costs nothing
_FAST_DELTA = os.environ.get("XFM_ATTN_FAST_DELTA", "0") != "0"
_VIT_FUSED_BWD = os.environ.get("XFM_ATTN_VIT_BWD", "0") != "0"   # opt-in single-pass attention backward (measured slower than the split pair: csrc/attention_vit.hip)
# the trunk's gradients leave for the all-reduce in chunks of this many blocks, from inside its backward; what is still there when the
# backward ends (blocks 0 .. chunk, the embeddings) is the exposed tail of the exchange: 2 -> 3 blocks = 85 MB of fp32 gradients behind
# five overlapped 57-MB collectives (round 2: 4 -> 5 blocks = 142 MB behind two of 114 MB)
# XFM_VIT_DEFER_WGRAD=0: one xfm_gemm_tn per projection as the backward reaches it (rounds 1-3) instead of the grouped launch
_DEFER_WGRAD = os.environ.get("XFM_VIT_DEFER_WGRAD", "1") != "0"
_RELPOS_AHEAD = os.environ.get("XFM_VIT_RELPOS_AHEAD", "1") != "0"   # A/B knob: the blocks' dense biases built up front on the second stream
_DEFER_LN = os.environ.get("XFM_VIT_DEFER_LN", "1") != "0"   # A/B knob: one batched LayerNorm column-sum reduce for the trunk
_WGRAD_GROUP_BLOCKS = int(os.environ.get("XFM_VIT_WGRAD_GROUP", "0"))   # blocks per grouped launch (0: the whole trunk at its end)
# (round 4: every hand-over also launches the chunk's queued weight gradients as one grouped call -- 0.43 ms per block in chunks of two,
# 0.37 in chunks of four, 0.33 for the whole trunk at once -- so chunks of four again: 0.6 ms less weight-gradient time than chunks of
# two for ~0.25 ms more exposed exchange (blocks 0-4 instead of 0-2 after the backward))
_GRAD_CHUNK_BLOCKS = max(1, int(os.environ.get("XFM_VIT_GRAD_CHUNK", "4")))


class _Affine(nn.Module):
    """weight/bias container for a LayerNorm (arithmetic runs in the fused HIP kernels)."""

    def __init__(self, dim, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))
        self.eps = eps


class _Dense(nn.Module):
    """weight/bias container for a Linear."""

    def __init__(self, fin, fout, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(fout, fin))
        self.bias = nn.Parameter(torch.zeros(fout)) if bias else None
        nn.init.trunc_normal_(self.weight, std=0.02, a=-2.0, b=2.0)


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.patch_shape = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.patch_shape[0] * self.patch_shape[1]
        self.proj = nn.Module()
        self.proj.weight = nn.Parameter(torch.empty(embed_dim, in_chans, patch_size, patch_size))
        self.proj.bias = nn.Parameter(torch.zeros(embed_dim))
        nn.init.kaiming_uniform_(self.proj.weight, a=math.sqrt(5))


class _FusedViT(OwnsArena, nn.Module):
    """Base of the towers whose blocks run through `_TrunkFn`.  A subclass has `patch_embed`, `cls_token`, `blocks` (each with norm1,
    attn.{qkv, proj, scale}, norm2, mlp.{fc1, fc2}, gamma_1 / gamma_2 -- None without layer scale -- and drop_path_prob), `embed_dim`
    and `num_heads`, and defines `_final_norm` (the LayerNorm behind the last block, fused into that block's second residual kernel)
    and `_qkv_bias_parts(blk)` (the bias operands of a block's qkv GEMM: Parameters, or an int = that many structural zeros)."""
    _rel_pos = False           # a relative-position bias per block (BEiT); the tower's attach() then provides _index32 and the sorted index
    _pool_tail = False         # the node replaces the cls row by the mean of the normalised patch rows (BEiT's forward_avgpool)
    _draw_at_rate_zero = False  # BEiT draws drop-path scales whenever it trains, even when no block drops; the plain ViT only if one does
    _trunk_bwd_done = None     # event behind the last trunk backward: two passes of one step accumulate into the same arena ranges
    _block_grad_hook = None    # data parallel: the accelerator's hand-over of finished block ranges (hook(vit, lo, hi, wg) -> bool)
    _arena = None
    _dp_keep = None

    def _layer_scale(self, gamma, grad=False):
        """(scale vector, where its gradient accumulates or None) of one residual branch.  A tower without layer scale multiplies by
        a constant vector of ones that has no gradient."""
        if gamma is None:
            return self._ones, None
        return gamma, (grad_of(gamma) if grad else None)

    # ---- arena plumbing -----------------------------------------------------------------------
    def linear_slots(self):
        self._slot_patch = LinearSlot("patch_embed", [self.patch_embed.proj.weight], [self.patch_embed.proj.bias])
        self._slot_patch.need_t = False
        self._slots = []
        out = [self._slot_patch]
        for i, blk in enumerate(self.blocks):
            s = {"qkv": LinearSlot(f"blocks.{i}.qkv", [blk.attn.qkv.weight], self._qkv_bias_parts(blk)),
                 "proj": LinearSlot(f"blocks.{i}.proj", [blk.attn.proj.weight], [blk.attn.proj.bias]),
                 "fc1": LinearSlot(f"blocks.{i}.fc1", [blk.mlp.fc1.weight], [blk.mlp.fc1.bias]),
                 "fc2": LinearSlot(f"blocks.{i}.fc2", [blk.mlp.fc2.weight], [blk.mlp.fc2.bias])}
            self._slots.append(s)
            out.extend(s.values())
        return out

    def attach(self, arena):
        self._arena = arena
        N = self.patch_embed.num_patches + 1
        self._bias_ld = (N + 15) // 16 * 16
        if self.blocks[0].gamma_1 is None:
            self._ones = torch.ones(self.embed_dim, dtype=torch.float32, device=arena.device)

    def finalize(self, device=None):
        """Stand-alone use (the XFM wrapper builds one arena for all towers instead)."""
        device = device or self.cls_token.device
        self.attach(ParamArena(self, self.linear_slots(), device))
        self._own_arena = True
        return self

    def _ready(self):
        if self._arena is None or not self._arena.attached():
            if self._arena is not None and not self._own_arena:
                raise RuntimeError("parameters were moved after the arena was built; call finalize() again")
            self.finalize()

    # ---- the parts of forward() the towers share ------------------------------------------------
    def _patch_tokens(self, x):
        """Images [B, C, H, W] -> fp32 patch tokens [B, P, D]: the patch gather and the patch-embed GEMM."""
        patches = Fx.patchify(x.float().contiguous(), self.patch_embed.patch_size[0])
        return linear_slot(patches, self._slot_patch, x_requires_grad=False, out_fp32=True).view(x.shape[0], -1, self.embed_dim)

    def _drop_path_scales(self, B, device):
        """fp32 [depth, 2, B] of 0 or 1 / keep for the two residual branches of every block, or None when nothing is drawn."""
        if not self.training or not (self._draw_at_rate_zero or any(b.drop_path_prob > 0 for b in self.blocks)):
            return None
        keep = self._dp_keep
        if keep is None or keep.device != device:  # built once: a per-forward torch.tensor(..., device=cuda) would sync
            keep = 1.0 - torch.tensor([[b.drop_path_prob] * 2 for b in self.blocks], device=device).view(-1, 2, 1)
            self._dp_keep = keep
        return (torch.rand(len(self.blocks), 2, B, device=device) < keep).float() / keep


def _bias_plan(N, need_grad, fused_bwd):
    """(transposed dense copy, forward tiles, backward tiles): which forms of a block's relative-position bias the attention
    kernels of a pass over N tokens read."""
    if 64 < N <= 224:   # the batch-walking ViT-shape kernels (csrc/attention_vit.hip) read accumulator-layout copies
        return True, True, bool(fused_bwd and need_grad)
    if N > 256 and need_grad:   # 384 / 480 px: the long-sequence backward kernels (csrc/attention_long.hip) read both tile copies;
        return False, True, True   # their dK/dV kernel reads the tiled transposed copy, no dense one
    return True, False, False


def _block_bias(vit, blk, H, N, ld, need_grad):
    """(dense, dense_t, tiles) of one block's relative-position bias, as _TrunkFn.forward builds them."""
    transposed, tiles_fwd, tiles_bwd = _bias_plan(N, need_grad, _VIT_FUSED_BWD)
    dense = Fx.relpos_gather(blk.attn.relative_position_bias_table, vit._index32, H, N, ld, transposed=transposed)
    dense, dense_t = dense if transposed else (dense, None)
    tiles = Fx.bias_tiles(dense, N, blk.attn.scale, fwd=True, bwd=tiles_bwd) if tiles_fwd else None
    return dense, dense_t, tiles


def _biases_ahead(vit, H, N, ld, need_grad, device):
    """The blocks' dense relative-position biases (table gather + accumulator-layout copies: two 5-us kernels per block) depend on the
    weights alone: all 24 launches go to the second stream up front and run under the first block's GEMMs.  None in single-stream mode."""
    pre = _WgradStream(device)
    if not pre.on:
        return None
    with torch.cuda.stream(pre.side):
        ahead = [_block_bias(vit, blk, H, N, ld, need_grad) for blk in vit.blocks]
        ev_bias = torch.cuda.Event()
        ev_bias.record(pre.side)
    for triple in ahead:
        for t in triple[:2] + tuple(triple[2] or ()):
            if t is not None:
                t.record_stream(pre.main)
    pre.main.wait_event(ev_bias)
    return ahead


def _reduce_queue(wg, n_blocks, M, D, device):
    """One batched column-sum reduce for the two LayerNorm backward kernels of every block (dgamma / dbeta / bias / layer-scale
    gradients), run with the queued weight gradients."""
    rq = Fx.ReduceQueue(device, 2 * n_blocks * ((_lib.load().xfm_layernorm_bwd_workspace(M, D, 2) + 255) // 256 * 256))   # LN_LS
    wg.defer_reduces(rq)
    return rq


def _relpos_table_grad(vit, blk, ddense, H, N, ld):
    """The launch that adds a block's relative-position TABLE gradient from its dense bias gradient."""
    G = blk.attn.window_size[0]
    dtab = grad_of(blk.attn.relative_position_bias_table)
    if N > 256 and blk.attn.window_size[0] == blk.attn.window_size[1] and N == G * G + 1:
        return lambda: Fx.relpos_grid_grad(ddense, G, H, ld, dtab)   # (144 -> ~20 us at 901 tokens)
    return lambda: Fx.relpos_scatter_sorted(ddense, vit._relpos_order, vit._relpos_start, H, N, ld, dtab)


def _nt320_hint(M, D, device):
    """tile_hint of the trunk's five N = D projections (forward proj and fc2, the dgrads of fc1, proj and qkv) for M rows, decided
    once per trunk pass: 6, the one-round 320 x 256 tile (csrc/nt320_gemm.hip), where 256 x 256 tiles need more than one round of the
    CUs and 320 x 256 tiles fit in one (M = 25216: 297 against 237 tiles on 256 CUs) -- the library's plan then splits a small-tile tail
    off every such call; 0 = the automatic plan.  XFM_GEMM_NT320=0 makes the library plan hint 6 as hint 0."""
    if device.type != "cuda" or D % 256 != 0:
        return 0
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return 6 if -(-M // 320) * (D // 256) <= cus < -(-M // 256) * (D // 256) else 0


class _TrunkFn(torch.autograd.Function):
    """All transformer blocks + the final LayerNorm as one node.  x0: fp32 [B, N, D] -> bf16 [B, N, D]."""

    @staticmethod
    def forward(ctx, x0, vit, dp):
        B, N, D = x0.shape
        M, H = B * N, vit.num_heads
        x = x0.reshape(M, D).contiguous()
        ld = vit._bias_ld
        blocks = vit.blocks
        need_grad = bool(ctx.needs_input_grad[0])
        saved = []
        n0 = blocks[0].norm1
        y, mean, rstd = Fx.ln_fwd(x, n0.weight, n0.bias, n0.eps)
        ctx.first = (x, mean, rstd)
        ctx.nxt = nxts = [blk.norm1 for blk in blocks[1:]] + [vit._final_norm]   # the LayerNorm fused behind each block
        rel_pos = vit._rel_pos
        ctx.nt_hint = hint = _nt320_hint(M, D, x.device)
        ahead = _biases_ahead(vit, H, N, ld, need_grad, x.device) if rel_pos and x.is_cuda and _RELPOS_AHEAD else None
        for i, blk in enumerate(blocks):
            s = vit._slots[i]
            g1, _ = vit._layer_scale(blk.gamma_1)
            g2, _ = vit._layer_scale(blk.gamma_2)
            dense = dense_t = tiles = None
            if ahead is not None:
                dense, dense_t, tiles = ahead[i]
            elif rel_pos:
                dense, dense_t, tiles = _block_bias(vit, blk, H, N, ld, need_grad)
            qkv = Fx.gemm_nt(y, s["qkv"].wb, s["qkv"].b)
            # long sequences keep the low half of O: the backward then takes delta from dO . (O + O_lo) instead of a first pass over
            # the keys (two of the dQ kernel's five matrix products: 355 -> 224 us per layer at 901 tokens for 24 us of forward)
            if need_grad and (_FAST_DELTA or N > 256):
                ctxv, lse, ctxv_lo = Fx.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, N, N, blk.attn.scale, bias=dense, lo=True,
                                                 bias_tiles=tiles)
            else:
                (ctxv, lse), ctxv_lo = Fx.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, N, N, blk.attn.scale, bias=dense,
                                                   bias_tiles=tiles), None
            h1 = Fx.gemm_nt(ctxv, s["proj"].wb, s["proj"].b, tile_hint=hint)
            dp1 = None if dp is None else dp[i, 0]
            dp2 = None if dp is None else dp[i, 1]
            x1, y2, mean2, rstd2 = Fx.ln_ls_fwd(x, h1, g1, dp1, N, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
            hact, u = Fx.gemm_nt(y2, s["fc1"].wb, s["fc1"].b, epi=Fx.EPI_GELU)
            h2 = Fx.gemm_nt(hact, s["fc2"].wb, s["fc2"].b, tile_hint=hint)
            nxt = nxts[i]
            x2, yn, meann, rstdn = Fx.ln_ls_fwd(x1, h2, g2, dp2, N, nxt.weight, nxt.bias, nxt.eps)
            saved.append((y, dense, qkv, ctxv, lse, h1, x1, mean2, rstd2, y2, u, hact, h2, x2, meann, rstdn, dp1, dp2, dense_t, ctxv_lo, tiles))
            x, y = x2, yn
        ctx.saved, ctx.vit, ctx.shape = saved, vit, (B, N, D)
        ctx.noted = need_grad
        if ctx.noted:
            arena_note_use(vit)
        ctx.pooled = bool(vit._pool_tail)
        if ctx.pooled:  # beit2.py:455-466: the cls row leaves as the mean of the normalised patch rows (in place: y is not saved)
            Fx.pool_rows_fwd_(y, B, N)
        return y.view(B, N, D)

    @staticmethod
    def backward(ctx, dy_out):
        vit, (B, N, D) = ctx.vit, ctx.shape
        M, H = B * N, vit.num_heads
        blocks = vit.blocks
        ld = vit._bias_ld
        hint = ctx.nt_hint
        # two passes of one step (clean / MIM-masked view) may run on different streams; their weight gradients accumulate (+=) into the
        # same arena ranges, so a pass starts only once the previous one -- wherever it ran -- has finished
        prev = vit._trunk_bwd_done
        if prev is not None and dy_out.is_cuda:
            torch.cuda.current_stream(dy_out.device).wait_event(prev)
        dy = dy_out.reshape(M, D).contiguous()
        if ctx.pooled:
            dy = Fx.pool_rows_bwd(dy if dy.dtype == torch.bfloat16 else dy.to(torch.bfloat16), B, N)
        dstream = torch.zeros((M, D), dtype=torch.float32, device=dy.device)
        wg = _WgradStream(dy.device, "vit bwd")
        done = len(blocks)
        ddense_all = None
        # the blocks' weight gradients are QUEUED and run as one grouped launch at the end of the trunk (or before each hand-over of a
        # gradient range to the data-parallel accelerator below): 48 projections x 9-36 output tiles walk whole tiles over all of M
        queued = _DEFER_WGRAD and dy.is_cuda
        tn = wg.defer_tn if queued else wg.gemm_tn
        # ... and so are the column-sum folds of the two LayerNorm backward kernels of a block
        rq = _reduce_queue(wg, len(blocks), M, D, dy.device) if _DEFER_LN and dy.is_cuda else None
        g = grad_of
        for i in reversed(range(len(blocks))):
            blk, s, nxt = blocks[i], vit._slots[i], ctx.nxt[i]
            (y, dense, qkv, ctxv, lse, h1, x1, mean2, rstd2, y2, u, hact, h2, x2, meann, rstdn, dp1, dp2, dense_t, ctxv_lo, tiles) = ctx.saved[i]
            g1, dg1 = vit._layer_scale(blk.gamma_1, grad=True)
            g2, dg2 = vit._layer_scale(blk.gamma_2, grad=True)
            dh2 = Fx.ln_ls_bwd(dy, dstream, x2, meann, rstdn, nxt.weight, h2, g2, dp2, N, g(nxt.weight), g(nxt.bias),
                               s["fc2"].db, dg2, defer=rq)
            tn(dh2, hact, s["fc2"].dw)
            du = Fx.gemm_nt(dh2, s["fc2"].wt, epi=Fx.EPI_DGELU, aux=u, n=s["fc2"].K)
            tn(du, y2, s["fc1"].dw, dbias=s["fc1"].db)
            dy2 = Fx.gemm_nt(du, s["fc1"].wt, n=s["fc1"].K, tile_hint=hint)
            dh1 = Fx.ln_ls_bwd(dy2, dstream, x1, mean2, rstd2, blk.norm2.weight, h1, g1, dp1, N, g(blk.norm2.weight),
                               g(blk.norm2.bias), s["proj"].db, dg1, defer=rq)
            tn(dh1, ctxv, s["proj"].dw)
            dctx = Fx.gemm_nt(dh1, s["proj"].wt, n=s["proj"].K, tile_hint=hint)
            dqkv = torch.empty_like(qkv)
            ddense = None
            if dense is not None:  # one zero fill for the whole trunk's bias-gradient scratch instead of one per block
                if ddense_all is None:
                    ddense_all = torch.zeros((len(blocks),) + tuple(dense.shape), dtype=dense.dtype, device=dense.device)
                ddense = ddense_all[i]
            Fx.attn_bwd(dctx, qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ctxv, lse, dqkv[:, :D], dqkv[:, D:2 * D],
                        dqkv[:, 2 * D:], B, H, N, N, blk.attn.scale, bias=dense, dbias=ddense, bias_t=dense_t, o_lo=ctxv_lo,
                        bias_tiles=tiles if (_VIT_FUSED_BWD or N > 256) else None)
            if dense is not None:   # the table gradient is a parameter gradient -- it runs with the queued weight gradients
                fn = _relpos_table_grad(vit, blk, ddense, H, N, ld)
                if queued:
                    wg.defer_call(fn, keep=(ddense_all,))
                else:
                    fn()
            tn(dqkv, y, s["qkv"].dw, dbias=s["qkv"].db)
            dy = Fx.gemm_nt(dqkv, s["qkv"].wt, n=s["qkv"].K, tile_hint=hint)
            ctx.saved[i] = None
            if _WGRAD_GROUP_BLOCKS > 0 and i % _WGRAD_GROUP_BLOCKS == 0:
                wg.flush()
            # data parallel: the gradients of blocks [i + 1, done) are final now (block i's own norm1 gradient is only written while
            # block i - 1 is processed) once this pass is the tower's last pending use -- hand that arena range to the accelerator,
            # so its all-reduce runs under the remaining blocks' backward
            if ctx.noted and i > 0 and i % _GRAD_CHUNK_BLOCKS == 0 and i + 1 < done:
                hook = vit._block_grad_hook
                # (the hook flushes the queued weight gradients itself once it knows the range really leaves now)
                if hook is not None and hook(vit, i + 1, done, wg):
                    done = i + 1
        x0, mean0, rstd0 = ctx.first
        n0 = blocks[0].norm1
        Fx.ln_bwd(dy, x0, mean0, rstd0, n0.weight, grad_of(n0.weight), grad_of(n0.bias), dx32=dstream, dx_accum=True)
        wg.join()
        if dstream.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dstream.device))
            vit._trunk_bwd_done = ev
        if ctx.noted:
            arena_note_grad(vit)
        return dstream.view(B, N, D), None, None
