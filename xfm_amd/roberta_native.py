"""The native executor of a RobertaEncoder's layers: ONE C-ABI call per layer and direction (csrc/encoder.hip), the default route of
every pre-training and fine-tuning step.  What it shares with the kernel-by-kernel pass lives in roberta_encoder."""
import ctypes
import math
import os

import torch

from . import _lib
from . import functional as Fx
from ._lib import ReduceItem, RLayerBwd, RLayerIO, RLayerLayout, RLayerParams, check
from .arena import arena_note_grad, arena_note_use
from .roberta_encoder import EncGrad, _grad_pair, _input_grads, check_pass_args, head_rows, pass_needs
from .roberta_layer import _seed_counter
from .side_stream import _WgradStream

BF16, F32 = torch.bfloat16, torch.float32


def _rlayer_params(layer, cfg):
    """The layer's static pointers for xfm_rlayer_fwd / _bwd (cached: operand copies and arena views are allocated once)."""
    P = getattr(layer, "_rlp", None)
    if P is not None:
        return P
    s = layer._s
    for slot in s.values():
        slot._alloc()
    P = RLayerParams()

    def put(name, slot, fwd=True):
        if fwd:
            setattr(P, "w" + name, slot._wb.data_ptr())
            setattr(P, "b" + name, slot.b.data_ptr())
        setattr(P, "w" + name + "_t", slot._wt.data_ptr())
        setattr(P, "ld_w" + name + "_t", slot._wt.stride(0))
        setattr(P, "dw" + name, slot._dw.data_ptr())
        setattr(P, "db" + name, slot._db.data_ptr())

    put("qkv", s["qkv"]); put("o", s["o"]); put("i", s["i"]); put("out", s["out"])
    lns = [layer.attention.output.LayerNorm, None, layer.output.LayerNorm]
    if layer.has_cross_attention:
        put("q2", s["q2"]); put("kv2", s["kv2"], fwd=False); put("o2", s["o2"])
        lns[1] = layer.crossattention.output.LayerNorm
    for k, ln in enumerate(lns):
        if ln is not None:
            setattr(P, f"ln{k + 1}_w", ln.weight.data_ptr()); setattr(P, f"ln{k + 1}_b", ln.bias.data_ptr())
            setattr(P, f"dln{k + 1}_w", ln.weight._xfm_grad.data_ptr()); setattr(P, f"dln{k + 1}_b", ln.bias._xfm_grad.data_ptr())
    P.D, P.H, P.FF, P.has_cross, P.eps = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, int(layer.has_cross_attention), \
        layer.output.LayerNorm.eps
    layer._rlp = P
    arena = s["qkv"]._arena
    own = [p for k in ("qkv", "o", "i", "out") for plist in (s[k].weights, s[k].biases) for p in plist if not isinstance(p, int)]
    own += [lns[0].weight, lns[0].bias, lns[2].weight, lns[2].bias]
    cross = []
    if layer.has_cross_attention:
        cross = [p for k in ("q2", "kv2", "o2") for plist in (s[k].weights, s[k].biases) for p in plist if not isinstance(p, int)]
        cross += [lns[1].weight, lns[1].bias]
    layer._rl_params = (own, cross)
    layer._rl_units = (sorted({arena._unit_of[id(p)] for p in own}), sorted({arena._unit_of[id(p)] for p in cross}))
    return P


def _rl_touch(layer, arena, cross):
    """Mark the layer's parameters live (their gradients are written by the native backward) -- a unit-flag check per layer once
    they all are."""
    live = arena.live
    for units, params in zip(layer._rl_units[:2 if cross else 1], layer._rl_params):
        for u in units:
            if not live[u]:
                arena.touch_all(params)
                break


def _view(slab, off, rows, cols, dtype=BF16):
    n = rows * cols * (2 if dtype == BF16 else 4)
    return slab[off:off + n].view(dtype).view(rows, cols)


_KV_AHEAD = os.environ.get("XFM_KV_AHEAD", "1") != "0"   # A/B knob of RobertaModel.prefetch_cross_kv
_RL_DEFER_LN = os.environ.get("XFM_RL_DEFER_LN", "1") != "0"   # A/B knob: one batched LayerNorm column-sum reduce per tower
_RL_DEFER_WGRAD = os.environ.get("XFM_RL_DEFER_WGRAD", "1") != "0"
_TOWER_JOIN_END = os.environ.get("XFM_TOWER_JOIN_END", "0") != "0"


def _bwd_workspaces(layouts, wg, device):
    """-> (bw with the launch stream's workspace, the side stream and its workspace filled in, [the two buffers]: the caller keeps them)."""
    Lmax = max(layouts.values(), key=lambda L: L.ws_side_bytes)
    bw = RLayerBwd()
    ws_main = Fx.workspace(max(L.ws_main_bytes for L in layouts.values()), device)
    bw.ws_main, bw.ws_main_bytes = ws_main.data_ptr(), ws_main.numel() * 4
    if wg.on:
        with torch.cuda.stream(wg.side):
            ws_side = Fx.workspace(Lmax.ws_side_bytes, device)
        bw.side_stream = wg.side.cuda_stream
    else:
        # (single stream: the per-stream workspace is already ws_main -- take a buffer of its own)
        ws_side = torch.empty(max(Lmax.ws_side_bytes // 4 + 1, 1), dtype=F32, device=device)
    bw.ws_side, bw.ws_side_bytes = ws_side.data_ptr(), ws_side.numel() * 4
    return bw, [ws_main, ws_side]


def _ln_reduce_table(lib, bw, rows, D, n_layers, device):
    """The LayerNorm backward kernels' column-sum folds (dgamma / dbeta / output-projection bias gradients): partials stay in per-call
    slices of one buffer and ONE batched reduce runs with the weight gradients, instead of a 7-us kernel behind each of the 3 per layer.
    -> (items the native backward fills, their count, the buffer, floats per call); Nones with the knob off."""
    if not _RL_DEFER_LN:
        return None, None, None, 0
    ln_stride = (lib.xfm_layernorm_bwd_workspace(rows, D, 1) // 4 + 63) // 64 * 64   # LN_POST
    ln_ws = torch.empty(max(3 * n_layers * ln_stride, 1), dtype=F32, device=device)
    ln_items, ln_count = (ReduceItem * (3 * n_layers))(), ctypes.c_int(0)
    bw.ln_items, bw.ln_count, bw.ln_ws_stride = ctypes.addressof(ln_items), ctypes.addressof(ln_count), ln_stride
    return ln_items, ln_count, ln_ws, ln_stride


def _defer_layer_wgrads(wg, layer, L, slab, bslab, x_in, R, FF, cross, dkv, enc):
    """A layer's weight gradients join the tower's queue: operands at the layout's offsets of the two slabs (kept alive by the caller)."""
    sl, D = layer._s, x_in.shape[1]
    Sv = lambda off, cols: _view(slab, off, R, cols)     # noqa: E731
    Gv = lambda off, cols: _view(bslab, off, R, cols)    # noqa: E731
    wg.defer_tn(Gv(L.dh3, D), Sv(L.hact, FF), sl["out"]._dw)
    wg.defer_tn(Gv(L.du, FF), Sv(L.y2 if cross else L.y1, D), sl["i"]._dw, sl["i"]._db)
    if cross:
        wg.defer_tn(Gv(L.dh2, D), Sv(L.c2, D), sl["o2"]._dw)
        wg.defer_tn(Gv(L.dq2, D), Sv(L.y1, D), sl["q2"]._dw, sl["q2"]._db)
        wg.defer_tn(dkv, enc, sl["kv2"]._dw, sl["kv2"]._db)   # (dK|dV comes from the side stream: the flush runs there too)
    wg.defer_tn(Gv(L.dh1, D), Sv(L.c1, D), sl["o"]._dw)
    wg.defer_tn(Gv(L.dqkv, 3 * D), x_in[:R], sl["qkv"]._dw, sl["qkv"]._db)


class _EncoderFnNative(torch.autograd.Function):
    """Layers [lo, hi) of a RobertaEncoder with ONE C-ABI call per layer and direction (csrc/encoder.hip sequences the kernels of
    the layer on the native side).  Same kernels, same order, same dropout streams as _EncoderFn -- results are bit-identical --
    but the host spends ~15 us per layer instead of ~200 us of per-kernel wrapper work, so a tower of 10-30 us kernels stops
    being bound by the Python interpreter.  Cross-attention goes through the grouped kernels (encoder_batch_index required)."""

    @staticmethod
    def forward(ctx, x, x32, enc, model, key_keep, enc_keep, lo, hi, causal, B, T, Nenc, training, enc_index, grad_batch, pack, xq, f32):
        lib = _lib.load()
        cfg = model.config
        check_pass_args(pack, key_keep, causal, grad_batch, enc, B)
        ctx.set_materialize_grads(False)
        ctx.twin_in = f32 and x32 is not None
        xt = x32.contiguous() if ctx.twin_in else None
        D, H, FF = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size
        p_att, p_hid, need_dx, need_denc = pass_needs(cfg, training, x, x32, enc)
        x = x.contiguous()
        R = x.shape[0]
        groups, U = None, 0
        if enc is not None:
            enc = enc.contiguous()
            U = enc.shape[0] // Nenc
            if xq is None:
                groups = Fx.kv_groups(enc_index, U)
        layers = [model.encoder.layer[li] for li in range(lo, hi)]
        for layer in layers:           # bf16 operand copies up to date (the arena's batched refresh when its version moved) and visible here
            for slot in layer._s.values():
                slot._ensure()
        d_att, d_hid = Fx.drop_params(p_att, 1), Fx.drop_params(p_hid, 1)
        io = RLayerIO()
        io.R, io.B, io.T, io.Nenc, io.U = R, B, T, Nenc if enc is not None else 0, U
        if pack is not None:
            io.seq_start, io.seq_len = pack.start.data_ptr(), pack.lens.data_ptr()
            io.zero_fill = int(not pack.exact)
        io.key_keep, io.enc_keep = Fx._ptr(key_keep), Fx._ptr(enc_keep)
        if groups is not None:
            io.grp_start, io.grp_rows = groups[0].data_ptr(), groups[1].data_ptr()
        if xq is not None:
            io.xq_start, io.xq_len, io.xq_max = xq[0].data_ptr(), xq[1].data_ptr(), int(xq[2])
        io.causal, io.scale = int(causal), 1.0 / math.sqrt(D // H)
        io.att_thresh, io.att_scale, io.hid_thresh, io.hid_scale = d_att[0], d_att[1], d_hid[0], d_hid[1]
        io.seed_hi = torch.initial_seed() & 0xFFFFFFFF
        io.f32_stream = int(f32)
        layouts = {}

        def layout(cross):
            if cross not in layouts:
                L = RLayerLayout()
                check(lib.xfm_rlayer_layout(R, B, T, D, H, FF, int(cross), io.Nenc, U, io.xq_max if xq is not None else 0,
                                            int(p_hid > 0) | (2 if f32 else 0), ctypes.byref(L)), "rlayer_layout")
                layouts[cross] = L
            return layouts[cross]

        kv_ready = {}
        pre = _WgradStream(x.device)
        if enc is not None:
            ahead = getattr(model, "_kv_ahead", None)   # prefetch_cross_kv(): the projections of THESE image states are already queued
            model._kv_ahead = None                      # (consumed and cleared on this route only: _EncoderFn always projects itself)
            if ahead is not None and ahead[0] == (enc.data_ptr(), tuple(enc.shape), enc._version):
                kv_ready = {k: v for k, v in ahead[1].items() if any(k == id(layer) for layer in layers)}
            for layer in layers:
                if layer.has_cross_attention and id(layer) not in kv_ready:
                    kv_ready[id(layer)] = pre.project(enc, layer._s["kv2"])
        st = Fx._stream()
        saved = []
        for layer in layers:
            cross = layer.has_cross_attention and enc is not None
            L = layout(cross)
            slab = torch.empty(L.fwd_bytes, dtype=torch.uint8, device=x.device)
            ctr = _seed_counter[0]
            _seed_counter[0] += 5 if cross else 3
            io.x, io.slab, io.seed_ctr = x.data_ptr(), slab.data_ptr(), ctr & 0xFFFFFFFF
            io.x32 = Fx._ptr(xt)
            kv = None
            if cross:
                kv, ev = kv_ready.pop(id(layer))
                io.kv, io.kv_ld, io.kv_event = kv.data_ptr(), kv.stride(0), (ev.cuda_event if ev is not None else 0)
            else:
                io.kv, io.kv_event = 0, 0
            check(lib.xfm_rlayer_fwd(ctypes.byref(_rlayer_params(layer, cfg)), ctypes.byref(io), st), "rlayer_fwd")
            saved.append((slab, x, kv, ctr, cross, xt))
            x = _view(slab, L.y3, R, D)
            xt = _view(slab, L.y3_32, R, D, F32) if f32 else None
        ctx.saved, ctx.model, ctx.enc, ctx.io, ctx.layouts, ctx.pack = saved, model, enc, io, layouts, pack
        ctx.keep = (groups, xq, key_keep, enc_keep)   # device arrays the io struct points at
        ctx.meta = (lo, hi, B, T, need_dx, need_denc, grad_batch)
        ctx.noted = need_dx or need_denc
        if ctx.noted:
            arena_note_use(model)
        return x, xt

    @staticmethod
    def backward(ctx, dy, dy32=None):
        lib = _lib.load()
        model, enc, io, pack = ctx.model, ctx.enc, ctx.io, ctx.pack
        lo, hi, B, T, need_dx, need_denc, grad_batch = ctx.meta
        cfg = model.config
        D, FF = cfg.hidden_size, cfg.intermediate_size
        layers = [model.encoder.layer[li] for li in range(lo, hi)]
        arena = layers[0]._s["qkv"]._arena
        f32 = bool(io.f32_stream)
        dy_a, dy_b = _grad_pair(dy, dy32, f32)
        dev = dy_a.device
        rows_full, R = dy_a.shape[0], dy_a.shape[0]
        if grad_batch is not None and grad_batch < B:
            # only the first `grad_batch` sequences carry gradient: the backward walks the row prefix of the saved activations
            R = head_rows(grad_batch, T, pack)
            io.R_alloc, io.B_alloc, io.R, io.B = rows_full, B, R, grad_batch
            dy_a = dy_a[:R]
            dy_b = None if dy_b is None else dy_b[:R]
            if pack is not None:
                io.zero_fill = int(not pack.head(grad_batch).exact)
        wg = _WgradStream(dev, "fusion bwd" if enc is not None else "text bwd")
        eg = EncGrad(enc, [layer for layer in layers if layer.has_cross_attention] if enc is not None else [], D, need_denc, True)
        bw, keep = _bwd_workspaces(ctx.layouts, wg, dev)
        if enc is not None:
            bw.enc = enc.data_ptr()
        bw.denc32 = Fx._ptr(eg.denc32)
        st = Fx._stream()
        # XFM_RL_DEFER_WGRAD (default on): the executor launches no weight gradient; the tower's queue runs as grouped launches at its
        # end (whole 256 x 256 tiles over all of M instead of 10 M-splits + a reduce per projection: the fusion + text towers' weight
        # gradients cost 2.8 ms of the step one by one under the activation-gradient chain, ~1.6 ms grouped)
        defer = _RL_DEFER_WGRAD and R >= 1024
        ln_items, ln_count, ln_ws, ln_stride = _ln_reduce_table(lib, bw, io.R_alloc if io.R_alloc > 0 else R, D, len(layers), dev)
        for k in reversed(range(len(layers))):
            layer = layers[k]
            slab, x_in, kv, ctr, cross, xt_in = ctx.saved[k]
            L = ctx.layouts[cross]
            bslab = torch.empty(L.bwd_bytes, dtype=torch.uint8, device=dev)
            keep.append((bslab, slab, x_in, kv, dy_a, dy_b, xt_in))
            io.x, io.slab, io.seed_ctr = x_in.data_ptr(), slab.data_ptr(), ctr & 0xFFFFFFFF
            io.x32 = Fx._ptr(xt_in)
            dkv = None
            if cross:
                io.kv, io.kv_ld, io.kv_event = kv.data_ptr(), kv.stride(0), 0
                dkv = eg.dkv_of(layer)
                keep.append(dkv)
                bw.dkv, bw.dkv_ld = dkv.data_ptr(), dkv.stride(0)
            else:
                io.kv = 0
            bw.bslab, bw.dy_a = bslab.data_ptr(), dy_a.data_ptr()
            bw.dy_b, bw.dy_b32 = (0, Fx._ptr(dy_b)) if f32 else (Fx._ptr(dy_b), 0)
            bw.need_dprev = int(k > 0 or need_dx)
            bw.defer_wgrad = int(defer)
            if ln_ws is not None:
                bw.ln_ws = ln_ws.data_ptr() + k * 3 * ln_stride * 4
            _rl_touch(layer, arena, cross)
            check(lib.xfm_rlayer_bwd(ctypes.byref(_rlayer_params(layer, cfg)), ctypes.byref(io), ctypes.byref(bw), st), "rlayer_bwd")
            if defer:
                _defer_layer_wgrads(wg, layer, L, slab, bslab, x_in, R, FF, cross, dkv, enc)
            dy_a, dy_b = _view(bslab, L.dprev, R, D), _view(bslab, L.dres1, R, D, F32 if f32 else BF16)
            ctx.saved[k] = None
        if ln_ws is not None and ln_count.value > 0:
            folds = [ln_items[i] for i in range(ln_count.value)]
            wg.defer_call(lambda: Fx.reduce_sets_batch(folds), keep=(ln_ws,))
        dx, dx32 = _input_grads(dy_a, dy_b, need_dx, ctx.twin_in, rows_full)
        denc = eg.finish(wg.sync_side)   # dK|dV of every layer (second stream) -- the queued weight gradients are launched by the join below
        if _TOWER_JOIN_END:   # (A/B knob: the tower's queued weight gradients re-join at the END of the backward pass instead of here)
            wg.join_at_end()
        else:
            wg.join()
        del keep
        if ctx.noted:
            arena_note_grad(model)
        return (dx, dx32, denc) + (None,) * 15
