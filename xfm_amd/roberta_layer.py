"""The kernel-by-kernel body of a RobertaLayer behind its self-attention, written once: the forward from the attention output
projection to the third LayerNorm and the backward from there down to the gradient of the self-attention output.  Callers
(roberta_encoder._EncoderFn: full rows, roberta_encoder._LastLayerRowsFn: selected rows, decode._run_layers: the cache) bring their own
self-attention, their cross-attention kernels as closures, and their input-gradient epilogue.  Also the towers' dropout seed bookkeeping."""
import torch

from . import functional as Fx
from .ops import grad_view

NO_DROPS = (Fx.drop_params(0.0, 0),) * 5
"""The drop tuples of an inference pass (no seed drawn)."""

_seed_counter = [0]   # the towers' dropout seed counter: ONE list, advanced in place by _next_seed and by the native executor


def _next_seed():
    _seed_counter[0] += 1
    return ((torch.initial_seed() & 0xFFFFFFFF) << 32) | (_seed_counter[0] & 0xFFFFFFFF)


def _layer_drops(p_att, p_hid, cross):
    """A layer's drop tuples (d_att, d_h1, d_att2, d_h2, d_h3), seeds drawn in that order (the two cross entries: None and no seed
    without cross-attention; the counter advances in eval mode too)."""
    d_att, d_h1 = Fx.drop_params(p_att, _next_seed()), Fx.drop_params(p_hid, _next_seed())
    d_att2, d_h2 = (Fx.drop_params(p_att, _next_seed()), Fx.drop_params(p_hid, _next_seed())) if cross else (None, None)
    return d_att, d_h1, d_att2, d_h2, Fx.drop_params(p_hid, _next_seed())


def forward_tail(layer, c1, res, drops, f32, cross=None, save=True):
    """Wo + LN1, [q2, cross-attention, Wo2 + LN2,] GELU FFN + LN3 -> (y3 bf16, the next residual operand, rec).
    c1: the self-attention output; res: what the first residual add reads (the fp32 twin of the layer input, or the input);
    drops = (d_att, d_h1, d_att2, d_h2, d_h3), the two cross entries unused without `cross`; f32: the fp32 residual stream.
    cross: q2 -> (kv, c2, lse2, c2lo); it fetches the projected K|V itself, so that a wait for a side-stream projection lands behind the
    q2 GEMM.  rec holds what backward_tail() reads (the caller adds what its own self-attention backward needs); save=False keeps
    nothing and returns rec = None."""
    s = layer._s
    d_att, d_h1, d_att2, d_h2, d_h3 = drops
    h1 = Fx.gemm_nt(c1, s["o"].wb, s["o"].b)
    ln1 = layer.attention.output.LayerNorm
    y1, z1, m1, r1, *tw = Fx.ln_post_fwd(h1, res, ln1.weight, ln1.bias, ln1.eps, d_h1, f32=f32)
    res = tw[0] if f32 else y1
    rec = {"c1": c1, "z1": z1, "m1": m1, "r1": r1, "y1": y1, "d_att": d_att, "d_h1": d_h1, "cross": cross is not None} if save else None
    y2 = y1
    if cross is not None:
        q2 = Fx.gemm_nt(y1, s["q2"].wb, s["q2"].b)
        kv, c2, lse2, c2lo = cross(q2)
        h2 = Fx.gemm_nt(c2, s["o2"].wb, s["o2"].b)
        ln2 = layer.crossattention.output.LayerNorm
        y2, z2, m2, r2, *tw = Fx.ln_post_fwd(h2, res, ln2.weight, ln2.bias, ln2.eps, d_h2, f32=f32)
        res = tw[0] if f32 else y2
        if save:
            rec.update(q2=q2, kv=kv, c2=c2, c2lo=c2lo, lse2=lse2, z2=z2, m2=m2, r2=r2, y2=y2, d_att2=d_att2, d_h2=d_h2)
    hact, u = Fx.gemm_nt(y2, s["i"].wb, s["i"].b, epi=Fx.EPI_GELU)
    h3 = Fx.gemm_nt(hact, s["out"].wb, s["out"].b)
    ln3 = layer.output.LayerNorm
    y3, z3, m3, r3, *tw = Fx.ln_post_fwd(h3, res, ln3.weight, ln3.bias, ln3.eps, d_h3, f32=f32)
    if save:
        rec.update(hact=hact, u=u, z3=z3, m3=m3, r3=r3, d_h3=d_h3)
    return y3, (tw[0] if f32 else y3), rec


def backward_tail(layer, r, dy_a, dy_b, wg, enc=None, cross_bwd=None, after_kv2=None, param_grads=True):
    """Backward of forward_tail -> (dc1, dres1): the gradient of the self-attention output and of the first residual operand.
    (dy_a bf16, dy_b) are the two gradient edges of the layer output; every weight gradient goes through wg.gemm_tn.
    cross_bwd: (dc2, r) -> (dq2, dkv), the caller's cross-attention backward; enc: the image states its K|V were projected from;
    after_kv2(dkv, r), if given, runs right behind the K|V weight gradient (the caller's gradient of the image states).
    param_grads=False (gradcam.cross_attention_gradcam: the activation-gradient chain alone): no LayerNorm or bias gradient is
    accumulated -- the caller's `wg` drops the weight gradients -- and a cross_bwd that returns (None, None) ends the layer's backward
    there (it wanted dc2 only): -> (None, None)."""
    s = layer._s
    g = grad_view if param_grads else (lambda p: None)
    # (slot.dw / slot.db mark their parameters as live in the gradient arena: not even asked for without param_grads)
    dw = (lambda name: s[name].dw) if param_grads else (lambda name: None)
    db = (lambda name: s[name].db) if param_grads else (lambda name: None)
    ln3 = layer.output.LayerNorm
    dh3, dres3 = Fx.ln_post_bwd(dy_a, r["z3"], r["m3"], r["r3"], ln3.weight, g(ln3.weight), g(ln3.bias), db("out"),
                                dy2=dy_b, drop=r["d_h3"])
    wg.gemm_tn(dh3, r["hact"], dw("out"))
    du = Fx.gemm_nt(dh3, s["out"].wt, epi=Fx.EPI_DGELU, aux=r["u"], n=s["out"].K)
    wg.gemm_tn(du, r["y2"] if r["cross"] else r["y1"], dw("i"), dbias=db("i"))
    d1a, d1b = Fx.gemm_nt(du, s["i"].wt, n=s["i"].K), dres3
    if r["cross"]:
        ln2 = layer.crossattention.output.LayerNorm
        dh2, dres2 = Fx.ln_post_bwd(d1a, r["z2"], r["m2"], r["r2"], ln2.weight, g(ln2.weight), g(ln2.bias), db("o2"),
                                    dy2=d1b, drop=r["d_h2"])
        wg.gemm_tn(dh2, r["c2"], dw("o2"))
        dc2 = Fx.gemm_nt(dh2, s["o2"].wt, n=s["o2"].K)
        dq2, dkv = cross_bwd(dc2, r)
        if dq2 is None:
            return None, None
        wg.gemm_tn(dq2, r["y1"], dw("q2"), dbias=db("q2"))
        wg.gemm_tn(dkv, enc, dw("kv2"), dbias=db("kv2"))
        if after_kv2 is not None:
            after_kv2(dkv, r)
        d1a, d1b = Fx.gemm_nt(dq2, s["q2"].wt, n=s["q2"].K), dres2
    ln1 = layer.attention.output.LayerNorm
    dh1, dres1 = Fx.ln_post_bwd(d1a, r["z1"], r["m1"], r["r1"], ln1.weight, g(ln1.weight), g(ln1.bias), db("o"),
                                dy2=d1b, drop=r["d_h1"])
    wg.gemm_tn(dh1, r["c1"], dw("o"))
    return Fx.gemm_nt(dh1, s["o"].wt, n=s["o"].K), dres1


def cross_bwd_split(wg, args, kw):
    """The per-image cross-attention backward in two phases: the dQ kernel stays on the activation-gradient chain; dK/dV (they only
    feed the K/V weight gradient and the gradient of the image states) run next to the weight-gradient GEMMs on the second stream.
    args / kw: those of Fx.attn_bwd; args[:9] are its tensors."""
    delta = Fx.attn_bwd(*args, phase=1, **kw)
    wg.run(lambda: Fx.attn_bwd(*args, phase=2, delta=delta, **kw), keep=args[:9] + (delta,))
