"""The kernel-by-kernel passes over a RobertaEncoder's layers (`_EncoderFn`: every token row, `_LastLayerRowsFn`: one layer on the rows
somebody reads) and what they share with the native executor (roberta_native): argument checks, derived quantities, the `grad_batch` row
prefix, the gradient edges of a tower output / input, the plan for the gradient of the image states.  `f32`: xroberta._F32_STREAM at the call."""
import math

import torch

from . import functional as Fx
from .arena import arena_note_grad, arena_note_use
from .roberta_layer import _layer_drops, backward_tail, cross_bwd_split, forward_tail
from .side_stream import _WgradStream

BF16, F32 = torch.bfloat16, torch.float32


def check_pass_args(pack, key_keep, causal, grad_batch, enc, B):
    """What an encoder pass refuses, on either route."""
    if pack is not None and (key_keep is not None or causal):
        raise ValueError("packed rows take neither a key mask (lengths say it all) nor the causal mask")
    if grad_batch is not None and (enc is not None or not 0 < grad_batch <= B):
        raise ValueError("grad_batch is for self-attention-only passes: 0 < grad_batch <= batch")


def pass_needs(cfg, training, x, x32, enc):
    """-> (p_att, p_hid, need_dx, need_denc): the dropout rates of this pass and which input gradients somebody reads."""
    p_att = cfg.attention_probs_dropout_prob if training else 0.0
    p_hid = cfg.hidden_dropout_prob if training else 0.0
    return p_att, p_hid, x.requires_grad or (x32 is not None and x32.requires_grad), (enc is not None and enc.requires_grad)


def head_rows(grad_batch, T, pack):
    """Token rows of the first `grad_batch` sequences, padded or packed."""
    return grad_batch * T if pack is None else pack.rows_of_head(grad_batch)


class EncGrad:
    """The gradient w.r.t. the shared image states = sum over `layers` (the cross-attention layers of the range) of dKV_l @ Wkv_l.  With
    dK / dV per image (`per_image`: the grouped / per-image kernels; always on the native route) every layer's dKV is [enc rows, 2D], so
    several layers write column blocks of ONE buffer (`dkv_all`) and a single GEMM with K = layers * 2D against the column-concatenated
    transposed weights replaces one fp32 read-modify-write GEMM per layer; otherwise the layers accumulate into `denc32` (fp32 zeros)."""

    def __init__(self, enc, layers, D, need_denc, per_image):
        self.enc, self.layers, self.D, self.need = enc, layers, D, need_denc
        self.concat_k = need_denc and per_image and len(layers) > 1
        self.dkv_all = torch.empty((enc.shape[0], len(layers) * 2 * D), dtype=BF16, device=enc.device) if self.concat_k else None
        self.denc32 = torch.zeros((enc.shape[0], D), dtype=F32, device=enc.device) if (need_denc and not self.concat_k) else None

    def dkv_of(self, layer):
        """Where `layer` writes its per-image dK|dV: its column block of `dkv_all`, or a fresh [enc rows, 2D] buffer."""
        if self.concat_k:
            j = self.layers.index(layer)
            return self.dkv_all[:, j * 2 * self.D:(j + 1) * 2 * self.D]
        return torch.empty((self.enc.shape[0], 2 * self.D), dtype=BF16, device=self.enc.device)

    def finish(self, before_read):
        """-> denc bf16 (None when nobody reads it).  `before_read()` orders the launch stream behind whoever wrote dK|dV / denc32."""
        if not self.need:
            return None
        if self.concat_k:
            wt_cat = torch.cat([layer._s["kv2"].wt[:, :2 * self.D] for layer in self.layers], dim=1)  # [D_enc, layers*2D]
            before_read()
            return Fx.gemm_nt(self.dkv_all, wt_cat)
        before_read()
        return self.denc32.to(BF16)


def _grad_pair(dy, dy32, f32):
    """The two gradient edges of a tower output (bf16 tensor, fp32 twin) as the (dy_a bf16, dy_b) pair the layer loop starts from:
    dy_b is the fp32 part with the fp32 stream on (None when nobody read the twin), None otherwise."""
    if dy is None and dy32 is None:
        raise RuntimeError("encoder backward without a gradient")
    if dy is None:
        dy = torch.zeros(dy32.shape, dtype=BF16, device=dy32.device)
    dy_a = dy.contiguous()
    if dy_a.dtype != BF16:
        dy_a = dy_a.to(BF16)
    if dy32 is None:
        return dy_a, None
    if f32:
        return dy_a, dy32.contiguous()
    return (dy_a.float() + dy32).to(BF16), None


def _input_grads(dy_a, dy_b, need_dx, twin_in, rows_full):
    """Gradient w.r.t. the tower input from the last layer's (dprev bf16, residual-branch gradient): with an fp32 twin on the input the
    two leave on their own edges, un-rounded; otherwise they are summed and rounded once to the input's bf16."""
    if not need_dx:
        return None, None
    if twin_in and dy_b is not None and dy_b.dtype == F32:
        dx, dx32 = dy_a, dy_b
    else:
        dx, dx32 = (dy_a.float() + dy_b.float()).to(BF16), None
    pad = rows_full - dx.shape[0]
    if pad > 0:   # (a backward over the first sequences of the batch: the other rows took no gradient)
        dx = torch.cat([dx, torch.zeros((pad, dx.shape[1]), dtype=dx.dtype, device=dx.device)], dim=0)
        if dx32 is not None:
            dx32 = torch.cat([dx32, torch.zeros((pad, dx32.shape[1]), dtype=F32, device=dx32.device)], dim=0)
    return dx, dx32


def layer_saves_maps(layer):
    """Whether `layer`'s cross-attention was asked for its attention maps (RobertaSelfAttention.save_attention)."""
    return layer.has_cross_attention and layer.crossattention.self.save_attention


def save_layer_maps(layer, r, dc2, B, H, T, Nenc, scale, key_keep, pack, xq, enc_keep, enc_index, n_src, p_att):
    """The attention-map contract for one cross-attention layer from its record r (q2, kv, lse2): dc2 None = after the forward, the
    probabilities go to save_attention_map; dc2 = the gradient of the context output, dP = dc2 . V^T goes to save_attn_gradients.
    Both fp32 [B, H, T, Nenc], rows past a sequence's length zero (the lengths are the pack's, or the row sums of a prefix mask).
    Eval mode only; no key mask on the image keys; xfm_xattn_gradcam for T <= 64, the torch restatement above that."""
    from .gradcam import attention_gradcam
    if p_att > 0.0:
        raise RuntimeError("save_attention: the attention maps are defined in eval mode only (attention dropout is on)")
    if xq is not None or enc_keep is not None:
        raise NotImplementedError("save_attention: per-image row ranges and masked image keys are outside the map contract")
    q_pack = None if pack is None else pack.pair
    q_len = key_keep.sum(dim=1).to(torch.int32) if (pack is None and key_keep is not None) else None
    D = H * 64
    kv = r["kv"]
    _, P, dP = attention_gradcam(r["q2"], r["q2"] if dc2 is None else dc2, kv[:, :D], kv[:, D:], r["lse2"], B, H, T, Nenc, scale, T,
                                 q_pack=q_pack, q_len=q_len, kv_src=enc_index, n_src=n_src, cam=False, p_out=dc2 is None, dp_out=dc2 is not None)
    att = layer.crossattention.self
    if dc2 is None:
        att.save_attention_map(P)
    else:
        att.save_attn_gradients(dP)


class _EncoderFn(torch.autograd.Function):
    """Layers [lo, hi) of a RobertaEncoder.  x: bf16 [B*T, D]; x32: its fp32 twin or None; enc: bf16 [B*N, D] or None.
    -> (y bf16, y fp32 twin or None): see xroberta._F32_STREAM (here the argument `f32`)."""

    @staticmethod
    def forward(ctx, x, x32, enc, model, key_keep, enc_keep, lo, hi, causal, B, T, Nenc, training, enc_index, grad_batch, pack, xq, f32):
        cfg = model.config
        check_pass_args(pack, key_keep, causal, grad_batch, enc, B)
        ctx.set_materialize_grads(False)
        D, H = cfg.hidden_size, cfg.num_attention_heads
        scale = 1.0 / math.sqrt(D // H)
        p_att, p_hid, need_dx, need_denc = pass_needs(cfg, training, x, x32, enc)
        saved = []
        x = x.contiguous()
        xres = x32.contiguous() if (f32 and x32 is not None) else x   # what the first residual add reads
        ctx.twin_in = f32 and x32 is not None
        qp = None if pack is None else pack.pair  # packed token rows: x is [pack.cap, D], sequences at (start, len)
        zf = pack is not None and not pack.exact  # slack rows exist: attention outputs must be zero there
        groups = None
        if enc is not None:
            enc = enc.contiguous()
            if xq is None and enc_index is not None and Fx.attn_grouped_ok(T, Nenc):
                groups = Fx.kv_groups(enc_index, enc.shape[0] // Nenc)
        # The K/V projections of the image states depend on no text-side activation (xroberta.py:224-226 recomputes them in every
        # layer from the same encoder_hidden_states): all layers' projections are enqueued up front on the second stream and run under
        # the self-attention halves of the layers, off the dependent chain; each cross-attention waits for its own layer's event.
        kv_ready = {}
        if enc is not None:
            pre = _WgradStream(x.device)
            for li in range(lo, hi):
                layer = model.encoder.layer[li]
                if layer.has_cross_attention:
                    kv_ready[li] = pre.project(enc, layer._s["kv2"])
        for li in range(lo, hi):
            layer = model.encoder.layer[li]
            s, cross = layer._s, None
            drops = _layer_drops(p_att, p_hid, layer.has_cross_attention and enc is not None)
            qkv = Fx.gemm_nt(x, s["qkv"].wb, s["qkv"].b)
            c1, lse1 = Fx.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, T, T, scale, key_keep=key_keep,
                                          causal=causal, drop=drops[0], q_pack=qp, k_pack=qp, zero_fill=zf)
            if drops[2] is not None:
                def cross(q2, li=li, d_att2=drops[2]):
                    kv = pre.take(kv_ready.pop(li))
                    if xq is not None:  # RANGE mode: sequences laid out image by image -> one ragged problem per image, full query tiles
                        return (kv,) + Fx.attn_fwd(q2, kv[:, :D], kv[:, D:], enc.shape[0] // Nenc, H, xq[2], Nenc, scale, key_keep=enc_keep,
                                                   drop=d_att2, q_pack=(xq[0], xq[1]), zero_fill=zf, lo=True)
                    if groups is not None:  # one workgroup per (image, head): K/V staged once for every row that reads it
                        # (lo: the low half of the output -- the backward's delta = dO . (O + Olo) then needs no sweep over the keys)
                        return (kv,) + Fx.attn_fwd(q2, kv[:, :D], kv[:, D:], B, H, T, Nenc, scale, key_keep=enc_keep, drop=d_att2, groups=groups,
                                                   q_pack=qp, zero_fill=zf, lo=True)
                    if pack is not None:
                        raise NotImplementedError("packed rows with cross-attention need the grouped kernels (T <= 64) and an encoder_batch_index")
                    return (kv,) + Fx.attn_fwd(q2, kv[:, :D], kv[:, D:], B, H, T, Nenc, scale, key_keep=enc_keep, drop=d_att2, kv_index=enc_index) + (None,)
            y3, yres, rec = forward_tail(layer, c1, xres, drops, f32, cross)
            rec.update(x=x, qkv=qkv, lse1=lse1, layer=layer)
            if cross is not None and layer_saves_maps(layer):
                rec["maps"] = True
                save_layer_maps(layer, rec, None, B, H, T, Nenc, scale, key_keep, pack, xq, enc_keep, enc_index, enc.shape[0] // Nenc, p_att)
            saved.append(rec)
            x, xres = y3, yres
        ctx.saved, ctx.model, ctx.enc, ctx.f32 = saved, model, enc, f32
        ctx.meta = (lo, hi, causal, B, T, Nenc, key_keep, enc_keep, need_dx, need_denc, scale, enc_index, groups, grad_batch)
        ctx.pack, ctx.xq = pack, xq
        ctx.noted = need_dx or need_denc
        if ctx.noted:
            arena_note_use(model)
        return x, (xres if f32 else None)

    @staticmethod
    def backward(ctx, dy, dy32=None):
        model, enc = ctx.model, ctx.enc
        lo, hi, causal, B, T, Nenc, key_keep, enc_keep, need_dx, need_denc, scale, enc_index, groups, grad_batch = ctx.meta
        cfg = model.config
        D, H = cfg.hidden_size, cfg.num_attention_heads
        dy_a, dy_b = _grad_pair(dy, dy32, ctx.f32)
        wg = _WgradStream(dy_a.device, "fusion bwd" if enc is not None else "text bwd")
        pack = ctx.pack
        rows_full = dy_a.shape[0]
        if grad_batch is not None and grad_batch < B:
            # only the first `grad_batch` sequences carry gradient (the rest of the pass was a detached forward that shared the
            # GEMMs): every op is per token / per sequence, so the backward runs on the row prefix of the saved activations
            B = grad_batch
            G = head_rows(B, T, pack)
            if pack is not None:
                pack = pack.head(B)
            dy_a = dy_a[:G]
            dy_b = None if dy_b is None else dy_b[:G]
            key_keep = None if key_keep is None else key_keep[:B]
            for rec in ctx.saved:
                for k, v in list(rec.items()):
                    if torch.is_tensor(v):
                        rec[k] = v[:B] if k.startswith("lse") else v[:G]
        qp = None if pack is None else pack.pair
        # packed rows with slack: the attention kernels only write real-token rows, the rest must be zero gradient
        new_grad = torch.zeros_like if (pack is not None and not pack.exact) else torch.empty_like
        xq = ctx.xq
        per_image = groups is not None or xq is not None   # dK / dV come out per image (not per query sequence)
        layers = [model.encoder.layer[li] for li in range(lo, hi)]
        eg = EncGrad(enc, [layer for layer in layers if layer.has_cross_attention] if enc is not None else [], D, need_denc, per_image)

        def cross_bwd(dc2, r):
            kv = r["kv"]
            if r.get("maps"):
                save_layer_maps(r["layer"], r, dc2, B, H, T, Nenc, scale, key_keep, pack, xq, enc_keep, enc_index, enc.shape[0] // Nenc, 0.0)
            dq2 = new_grad(r["q2"])
            if per_image:  # dK/dV accumulated over each image's rows in registers, written once per image
                dkv = eg.dkv_of(r["layer"])
                if xq is not None:
                    args = (dc2, r["q2"], kv[:, :D], kv[:, D:], r["c2"], r["lse2"], dq2, dkv[:, :D], dkv[:, D:], enc.shape[0] // Nenc, H,
                            xq[2], Nenc, scale)
                    kw = dict(key_keep=enc_keep, drop=r["d_att2"], q_pack=(xq[0], xq[1]), o_lo=r["c2lo"])
                else:
                    args = (dc2, r["q2"], kv[:, :D], kv[:, D:], r["c2"], r["lse2"], dq2, dkv[:, :D], dkv[:, D:], B, H, T, Nenc, scale)
                    kw = dict(key_keep=enc_keep, drop=r["d_att2"], groups=groups, q_pack=qp, o_lo=r["c2lo"])
                cross_bwd_split(wg, args, kw)
            else:
                dkv = torch.empty((B * Nenc, 2 * D), dtype=BF16, device=dq2.device)  # per query row
                Fx.attn_bwd(dc2, r["q2"], kv[:, :D], kv[:, D:], r["c2"], r["lse2"], dq2, dkv[:, :D], dkv[:, D:], B, H, T, Nenc,
                            scale, key_keep=enc_keep, drop=r["d_att2"], kv_index=enc_index)
                if enc_index is not None:  # fold onto the unique key/value sources
                    dkv = Fx.rows_index_sum(dkv, enc_index, enc.shape[0] // Nenc, Nenc)
            return dq2, dkv

        def add_denc(dkv, r):
            s = r["layer"]._s
            if per_image:  # dkv is produced on the second stream: its consumer follows it there
                wg.run(lambda dkv=dkv, s=s: Fx.gemm_nt(dkv, s["kv2"].wt, epi=Fx.EPI_F32_ACC, out=eg.denc32, n=s["kv2"].K), keep=(dkv,))
            else:
                Fx.gemm_nt(dkv, s["kv2"].wt, epi=Fx.EPI_F32_ACC, out=eg.denc32, n=s["kv2"].K)

        for k in reversed(range(len(layers))):
            layer = layers[k]
            s, r = layer._s, ctx.saved[k]
            dc1, dres1 = backward_tail(layer, r, dy_a, dy_b, wg, enc, cross_bwd, add_denc if need_denc and not eg.concat_k else None)
            qkv = r["qkv"]
            dqkv = new_grad(qkv)
            Fx.attn_bwd(dc1, qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], r["c1"], r["lse1"], dqkv[:, :D], dqkv[:, D:2 * D],
                        dqkv[:, 2 * D:], B, H, T, T, scale, key_keep=key_keep, causal=causal, drop=r["d_att"], q_pack=qp, k_pack=qp)
            wg.gemm_tn(dqkv, r["x"], s["qkv"].dw, dbias=s["qkv"].db)
            if k > 0 or need_dx:
                dy_a, dy_b = Fx.gemm_nt(dqkv, s["qkv"].wt, n=s["qkv"].K), dres1
            ctx.saved[k] = None
        dx, dx32 = _input_grads(dy_a, dy_b, need_dx, ctx.twin_in, rows_full)
        denc = eg.finish(wg.join)   # the dK/dV blocks / the denc32 updates were written on the second stream
        wg.join()  # the weight gradients are complete in main-stream order before the tower's all-reduce / the optimizer
        if ctx.noted:
            arena_note_grad(model)
        return (dx, dx32, denc) + (None,) * 15


class _LastLayerRowsFn(torch.autograd.Function):
    """ONE RobertaLayer computed only on the token rows somebody reads afterwards.

    The consumers of the fusion tower's last layer are the [CLS] rows of the 3B matching sequences (xfm.py:795-797) and the masked
    positions of the B MLM sequences (xroberta.py:1215-1216): ~1/5 of the token rows.  No op of a layer couples token rows except
    attention, and there only through the keys: so the last layer projects K / V for every row of a sequence but runs its queries,
    both attention outputs, the three LayerNorms and the FFN on the selected rows alone (same arithmetic per selected row as the
    full layer; the other rows' outputs were dead values).  x: [R, D] packed rows (all), `rows`: int32 [S] indices into them
    (duplicates allowed), `sel` = (start, len) int32 [B] of each sequence's block inside the S-row layout, `Tq` = max block length.
    Output: [S, D].  Backward: the selected rows' gradients are scatter-added into the full-row gradient, next to dK/dV . W_kv."""

    @staticmethod
    def forward(ctx, x, x32, enc, model, li, B, T, Nenc, training, enc_index, pack, rows, sel, Tq, f32):
        cfg = model.config
        ctx.set_materialize_grads(False)
        ctx.twin_in, ctx.f32 = f32 and x32 is not None, f32
        D, H = cfg.hidden_size, cfg.num_attention_heads
        scale = 1.0 / math.sqrt(D // H)
        p_att, p_hid, need_dx, need_denc = pass_needs(cfg, training, x, x32, enc)
        layer = model.encoder.layer[li]
        s = layer._s
        cross = layer.has_cross_attention and enc is not None
        x = x.contiguous()
        kp = pack.pair
        pre = _WgradStream(x.device)
        kv_pair = pre.project(enc, s["kv2"]) if cross else None
        groups = Fx.kv_groups(enc_index, enc.shape[0] // Nenc) if cross else None
        drops = _layer_drops(p_att, p_hid, cross)
        wqkv, bqkv = s["qkv"].wb, s["qkv"].b
        kvs = Fx.gemm_nt(x, wqkv[D:3 * D], bqkv[D:3 * D])                      # K | V of every row
        xs = Fx.rows_gather(x, rows)
        xres = Fx.rows_gather(x32.contiguous(), rows) if ctx.twin_in else xs   # the selected rows' residual, un-rounded when the twin exists
        qs = Fx.gemm_nt(xs, wqkv[:D], bqkv[:D])                                # Q of the selected rows
        c1, lse1 = Fx.attn_fwd(qs, kvs[:, :D], kvs[:, D:], B, H, Tq, T, scale, drop=drops[0], q_pack=sel, k_pack=kp, zero_fill=False)

        def cross_fwd(q2):
            kv = pre.take(kv_pair)
            return (kv,) + Fx.attn_fwd(q2, kv[:, :D], kv[:, D:], B, H, Tq, Nenc, scale, drop=drops[2], groups=groups, q_pack=sel, zero_fill=False,
                                       lo=True)
        y3, yres, rec = forward_tail(layer, c1, xres, drops, f32, cross_fwd if cross else None)
        rec.update(x=x, xs=xs, kvs=kvs, qs=qs, lse1=lse1)
        ctx.rec, ctx.model, ctx.enc, ctx.layer = rec, model, enc, layer
        ctx.meta = (B, T, Nenc, scale, groups, kp, rows, sel, Tq, need_dx, need_denc)
        ctx.noted = need_dx or need_denc
        if ctx.noted:
            arena_note_use(model)
        return y3, (yres if f32 else None)

    @staticmethod
    def backward(ctx, dy, dy32=None):
        model, enc, layer, r = ctx.model, ctx.enc, ctx.layer, ctx.rec
        B, T, Nenc, scale, groups, kp, rows, sel, Tq, need_dx, need_denc = ctx.meta
        cfg = model.config
        D, H = cfg.hidden_size, cfg.num_attention_heads
        s = layer._s
        dy_a, dy_b = _grad_pair(dy, dy32, ctx.f32)
        wg = _WgradStream(dy_a.device, "fusion bwd" if enc is not None else "text bwd")
        denc = None

        def cross_bwd(dc2, r):
            kv = r["kv"]
            dq2 = torch.empty_like(r["q2"])
            dkv = torch.empty((enc.shape[0], 2 * D), dtype=BF16, device=dq2.device)
            args = (dc2, r["q2"], kv[:, :D], kv[:, D:], r["c2"], r["lse2"], dq2, dkv[:, :D], dkv[:, D:], B, H, Tq, Nenc, scale)
            cross_bwd_split(wg, args, dict(drop=r["d_att2"], groups=groups, q_pack=sel, o_lo=r["c2lo"]))
            return dq2, dkv

        def set_denc(dkv, r):
            nonlocal denc
            denc = wg.run(lambda: Fx.gemm_nt(dkv, s["kv2"].wt, n=s["kv2"].K), keep=(dkv,))
        dc1, dres1 = backward_tail(layer, r, dy_a, dy_b, wg, enc, cross_bwd, set_denc if need_denc else None)
        kvs, qs = r["kvs"], r["qs"]
        dqs, dkvs = torch.empty_like(qs), torch.empty_like(kvs)
        Fx.attn_bwd(dc1, qs, kvs[:, :D], kvs[:, D:], r["c1"], r["lse1"], dqs, dkvs[:, :D], dkvs[:, D:], B, H, Tq, T, scale, drop=r["d_att"],
                    q_pack=sel, k_pack=kp)
        dw, db = s["qkv"].dw, s["qkv"].db
        wg.gemm_tn(dqs, r["xs"], dw[:D], dbias=db[:D])
        wg.gemm_tn(dkvs, r["x"], dw[D:3 * D], dbias=db[D:3 * D])
        dx, dxt = None, None
        if need_dx:
            wt = s["qkv"].wt
            dx32 = Fx.gemm_nt(dkvs, wt[:, D:3 * D], epi=Fx.EPI_F32, n=s["qkv"].K)           # through K / V: every row
            Fx.rows_scatter_add(Fx.gemm_nt(dqs, wt[:, :D], n=s["qkv"].K), rows, dx32)     # through Q and the residual: selected rows
            if dres1.dtype == F32:   # fp32 stream: the residual-branch gradient of the selected rows stays fp32 ...
                if ctx.twin_in:      # ... and leaves on the twin's edge
                    dxt = torch.zeros_like(dx32).index_add_(0, rows.long(), dres1)
                else:
                    dx32.index_add_(0, rows.long(), dres1)
            else:
                Fx.rows_scatter_add(dres1, rows, dx32)
            dx = dx32.to(BF16)
        wg.join()
        if ctx.noted:
            arena_note_grad(model)
        ctx.rec = None
        return (dx, dxt, denc) + (None,) * 12
