"""Grad-CAM grounding: the cross-attention maps of one fusion layer, their gradients, and the weakly-supervised mask evaluation.

Mirrors (names, argument meaning, ordering):
  * attention_gradcam / gradcam_torch   Grounding.py:101-115 on models/xroberta.py:182-194, 268-270 (save_attention / get_attention_map /
                                        get_attn_gradients): P, dP and cam of one cross-attention layer from (q, dO, K | V, lse)
  * grounding_eval                      dataset/utils.py:178-223 (+ :349-361 computeIoU) on xfm_cam_box_rank
What differs, on purpose:
  * the reference moves every map to the device and back and ranks the boxes in Python; here the maps of a pass stay on the device, one
    launch ranks the boxes of every ref of a pass, and the [3, 2] counts buffer is read ONCE;
  * a ref none of whose boxes scores above 0 is counted as WRONG (chosen index -1); the reference would reuse the previous ref's box, or
    raise on the first one;
  * the upsampled map is never built: the sum over a box is a^T cam b (include/xfm_hip.h, xfm_cam_box_rank).
`gradcam_torch` and `cam_box_rank_host` restate the two kernels' definitions in torch / numpy: they serve CPU tensors and the shapes above
the kernels' limits (Sq > 64; p > 32 or more than 256 boxes for one ref), never a missing kernel."""
import numpy as np
import torch

from . import _lib
from .grounding_loop import SPLITS
from .task import read as _read   # the single device-to-host read of a pass (the tests count its calls)

F32 = torch.float32


# ------------------------------------------------------------------------------------------------------------------ maps and cam
def gradcam_torch(q, dout, k, v, lse, B, H, Sq, Sk, scale, t_div, q_start=None, q_len=None, kv_src=None):
    """The definitions of xfm_xattn_gradcam in torch (fp32), any device: -> (cam [B, Sk - 1], P [B, H, Sq, Sk], dP [B, H, Sq, Sk]).
    q / dout: [rows, >= H*64]; k / v: [sources * Sk, >= H*64]; lse fp32 [B, H, >= Sq]."""
    dev = q.device
    D = H * 64
    t = torch.arange(Sq, device=dev)
    start = (torch.arange(B, device=dev) * Sq) if q_start is None else q_start.long()
    length = torch.full((B,), Sq, device=dev, dtype=torch.long) if q_len is None else q_len.long().clamp(0, Sq)
    valid = t[None, :] < length[:, None]                                          # [B, Sq]
    rows = (start[:, None] + t[None, :]).clamp(0, q.shape[0] - 1)                 # (rows past the length: any row, masked below)
    src = torch.arange(B, device=dev) if kv_src is None else kv_src.long()
    qh = q[:, :D].float()[rows].view(B, Sq, H, 64).permute(0, 2, 1, 3)             # [B, H, Sq, 64]
    dh = dout[:, :D].float()[rows].view(B, Sq, H, 64).permute(0, 2, 1, 3)
    kh = k[:, :D].float().reshape(-1, Sk, H, 64)[src].permute(0, 2, 1, 3)          # [B, H, Sk, 64]
    vh = v[:, :D].float().reshape(-1, Sk, H, 64)[src].permute(0, 2, 1, 3)
    keep = valid[:, None, :, None]
    lse_rows = torch.where(valid[:, None, :], lse[:, :, :Sq].float(), torch.zeros((), device=dev))
    P = torch.where(keep, torch.exp(qh @ kh.transpose(-1, -2) * scale - lse_rows[..., None]), torch.zeros((), device=dev))
    dP = torch.where(keep, dh @ vh.transpose(-1, -2), torch.zeros((), device=dev))
    cam = (P[..., 1:] * dP[..., 1:].clamp(min=0)).sum(dim=(1, 2)) / float(H * t_div)
    return cam, P, dP


def attention_gradcam(q, dout, k, v, lse, B, H, Sq, Sk, scale, t_div, q_pack=None, q_len=None, kv_src=None, n_src=None, cam=True,
                      p_out=False, dp_out=False):
    """(cam | None, P | None, dP | None) of one cross-attention layer: xfm_xattn_gradcam on HIP tensors with Sq <= 64, the torch
    restatement on CPU tensors and above the kernel's limit."""
    from . import functional as Fx
    if q.is_cuda and Fx.attn_grouped_ok(Sq, Sk):
        return Fx.xattn_gradcam(q, dout, k, v, lse, B, H, Sq, Sk, scale, t_div, q_pack=q_pack, q_len=q_len, kv_src=kv_src, n_src=n_src,
                                cam=cam, p_out=p_out, dp_out=dp_out)
    q_start = None
    if q_pack is not None:
        q_start, q_len = q_pack
    c, P, dP = gradcam_torch(q, dout, k, v, lse, B, H, Sq, Sk, scale, t_div, q_start=q_start, q_len=q_len, kv_src=kv_src)
    return (c if cam else None), (P if p_out else None), (dP if dp_out else None)


# ------------------------------------------------------------------------------------------------------------------ box ranking
def cubic_tap_weights(n_out, n_in):
    """ATen's bicubic taps of an align_corners=False resize n_in -> n_out (UpSample.h, A = -0.75), in fp32 and in its operation order:
    -> (index int64 [n_out, 4] clamped to the input, weight fp32 [n_out, 4])."""
    f = np.float32
    A = f(-0.75)
    scale = f(n_in) / f(n_out)
    real = scale * (np.arange(n_out, dtype=np.float32) + f(0.5)) - f(0.5)
    i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    t = np.minimum(np.maximum(real - i0.astype(np.float32), f(0.0)), f(1.0)).astype(np.float32)

    def conv1(x):
        return ((A + f(2.0)) * x - (A + f(3.0))) * x * x + f(1.0)

    def conv2(x):
        return ((A * x - f(5.0) * A) * x + f(8.0) * A) * x - f(4.0) * A
    x2 = f(1.0) - t
    w = np.stack([conv2(t + f(1.0)), conv1(t), conv1(x2), conv2(x2 + f(1.0))], axis=1).astype(np.float32)
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, w


def _slice_bound(v, hi):
    return hi if v >= hi else (int(v) if v > 0 else 0)


def box_weight_sums(lo, ext, size, p):
    """a [p] fp64: the sum over output rows int(lo) : int(lo + ext) (clamped at `size`, as a Python slice) of the weight each gives input
    row i, the taps in fp32."""
    idx, w = cubic_tap_weights(size, p)
    s0, s1 = _slice_bound(lo, size), _slice_bound(lo + ext, size)
    a = np.zeros(p, dtype=np.float64)
    for y in range(s0, s1):
        for j in range(4):
            a[idx[y, j]] += np.float64(w[y, j])
    return a


def compute_iou(box1, box2):
    """computeIoU (dataset/utils.py:349-361) in fp64; union <= 0: 0 (xfm_box_eval's rule)."""
    x1, y1 = max(box1[0], box2[0]), max(box1[1], box2[1])
    x2, y2 = min(box1[0] + box1[2] - 1, box2[0] + box2[2] - 1), min(box1[1] + box1[3] - 1, box2[1] + box2[3] - 1)
    inter = (x2 - x1 + 1) * (y2 - y1 + 1) if x1 < x2 and y1 < y2 else 0.0
    union = box1[2] * box1[3] + box2[2] * box2[3] - inter
    return 0.0 if union <= 0 else inter / union


def cam_box_rank_host(cam, img_hw, dets, ref_box, ref_split, alpha):
    """xfm_cam_box_rank's arithmetic on the host (numpy fp64 from the fp32 maps): cam [n, p, p]; img_hw [n, 2] = (height, width); dets = a
    list of n [k, 4] arrays of (x, y, w, h); ref_box [n, 4]; ref_split [n].  -> (out fp64 [n, 3] = (chosen index or -1, score, IoU),
    counts int64 [3, 2])."""
    cam = np.asarray(cam, dtype=np.float32).astype(np.float64)
    n, p = cam.shape[0], cam.shape[1]
    out = np.zeros((n, 3))
    counts = np.zeros((3, 2), dtype=np.int64)
    for i in range(n):
        Hh, Ww = int(img_hw[i][0]), int(img_hw[i][1])
        best, pick = 0.0, -1
        for d, det in enumerate(np.asarray(dets[i], dtype=np.float64).reshape(-1, 4)):
            a = box_weight_sums(det[1], det[3], Hh, p)
            b = box_weight_sums(det[0], det[2], Ww, p)
            with np.errstate(divide='ignore', invalid='ignore'):
                score = np.float64(a @ (cam[i] @ b)) / np.float64(det[2] * det[3]) ** np.float64(alpha)
            if score > best:
                best, pick = float(score), d
        iou = 0.0
        if pick >= 0:
            iou = compute_iou([float(x) for x in ref_box[i]], [float(x) for x in np.asarray(dets[i], dtype=np.float64).reshape(-1, 4)[pick]])
        out[i] = (pick, best, iou)
        s = int(ref_split[i])
        if 0 <= s < 3:
            counts[s, 1] += 1
            counts[s, 0] += int(pick >= 0 and iou >= 0.5)
    return out, counts


def _check_dets(dets, n):
    dets = [np.asarray(d, dtype=np.float64).reshape(-1, 4) for d in dets]
    if len(dets) != n:
        raise ValueError(f"grounding_eval: {len(dets)} box lists for {n} maps")
    for d in dets:
        if not np.all(np.isfinite(d)) or np.any(d < 0):
            raise ValueError("grounding_eval: detector boxes need finite, non-negative (x, y, w, h)")
    return dets


def grounding_eval(cams, refs, dets, alpha=0.5, return_rows=False):
    """dataset/utils.py:178-223 for the refs of a pass, in the order of `cams` (fp32 [n, p, p]; the `pred` of val()'s records, stacked):
    `refs` carries ref_box [n, 4] (x, y, w, h in pixels), ref_size [n, 2] = (width, height) of the image and ref_split [n] (0 val, 1 testA,
    2 testB) -- synthetic.grounding_refs' tables, the REFER object's content; `dets` = one [k, 4] array of detector boxes per ref.
    Returns {'val_d', 'testA_d', 'testB_d'} (with return_rows: also the fp64 [n, 3] rows (chosen index, score, IoU)).  On HIP tensors
    one xfm_cam_box_rank launch and ONE device read; on CPU tensors and above the kernel's caps the host form."""
    n, p = cams.shape[0], cams.shape[1]
    assert cams.dim() == 3 and cams.shape[2] == p
    dets = _check_dets(dets, n)
    size = np.asarray(refs.ref_size, dtype=np.float64).reshape(n, 2)
    img_hw = np.stack([size[:, 1], size[:, 0]], axis=1).astype(np.int32)
    if np.any(img_hw < 1):
        raise ValueError("grounding_eval: image sizes must be at least one pixel")
    ref_box = np.asarray(refs.ref_box, dtype=np.float64).reshape(n, 4)
    ref_split = np.asarray(refs.ref_split).astype(np.int32).reshape(n)
    max_dets = max((d.shape[0] for d in dets), default=0)
    if cams.is_cuda and p <= _lib.CAM_MAX_P and max_dets <= _lib.CAM_MAX_DETS:
        from . import functional as Fx
        dev = cams.device
        start = np.zeros(n + 1, dtype=np.int32)
        start[1:] = np.cumsum([d.shape[0] for d in dets])
        flat = np.concatenate(dets + [np.zeros((1, 4))], axis=0)   # (never empty)
        out = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        counts = torch.zeros(3, 2, dtype=torch.int64, device=dev)
        Fx.cam_box_rank(cams.float().contiguous(), torch.from_numpy(img_hw).to(dev), torch.from_numpy(flat).to(dev),
                        torch.from_numpy(start).to(dev), max_dets, torch.from_numpy(ref_box).to(dev), torch.from_numpy(ref_split).to(dev),
                        alpha, counts, out, 0)
        if return_rows:   # one read for both: the counts ride behind the rows as exact fp64 integers
            got = _read(torch.cat([out[:n].reshape(-1), counts.reshape(-1).double()]))
            rows, c = np.asarray(got[:3 * n]).reshape(n, 3), [[int(got[3 * n + 2 * s]), int(got[3 * n + 2 * s + 1])] for s in range(3)]
        else:
            rows, c = None, _read(counts)
    else:
        rows, c = cam_box_rank_host(_read(cams.float()) if cams.is_cuda else cams.float().numpy(), img_hw, dets, ref_box, ref_split, alpha)
        c = c.tolist()
    acc = {f'{name}_d': c[s][0] / c[s][1] for s, name in enumerate(SPLITS)}
    for metric, val_ in acc.items():
        print(f'{metric}: {val_:.3f}', flush=True)
    return (acc, rows) if return_rows else acc


# ------------------------------------------------------------------------------------------------------------------ the model side
class _NoWgrad:
    """Stand-in for side_stream._WgradStream in a pass that wants the activation-gradient chain alone: weight gradients, and the dK / dV
    kernels that only feed them and the gradient of the image states, are not run."""

    def gemm_tn(self, *a, **kw):
        return None

    def run(self, fn, keep=()):
        return None

    def join(self):
        return None


class _Ctx:
    """What _EncoderFn.forward asks of its autograd context, for a segment whose backward this module walks itself."""
    needs_input_grad = (False,) * 18

    def set_materialize_grads(self, flag):
        pass


def _fusion_roberta(model):
    fe = model.fusion_encoder
    return fe.roberta if hasattr(fe, "roberta") else fe.bert


def _itm_cls_gradient(model, cls):
    """d(itm_head(cls)[:, 1].sum()) / d cls for the B [CLS] rows, bf16 (Grounding.py:95-96, 99): the head's forward and the input-gradient
    half of its backward with the kernels its autograd nodes run (ops._LinearSlotFn / _LayerNormFn: Linear, LayerNorm + GELU, Linear),
    in their order and on their operands, without the weight, bias and LayerNorm gradients those nodes would add to the arena."""
    from . import functional as Fx
    BF16 = torch.bfloat16
    head = model.itm_head
    s0, s3, ln = head._s0, head._s3, getattr(head, "1")
    x = cls.to(BF16).contiguous()
    h0 = Fx.gemm_nt(x, s0.wb, s0.b)
    _, mean, rstd = Fx.ln_fwd(h0, ln.weight, ln.bias, ln.eps, gelu=True)
    pad = (s3.N + 63) // 64 * 64                       # the 2-way logits: columns padded to the kernels' granularity, as the node does
    dyp = torch.zeros((x.shape[0], pad), dtype=BF16, device=x.device)
    dyp[:, 1] = 1.0                                    # d(out[:, 1].sum()) / d out
    if pad <= s3.wt.shape[1]:
        dh = Fx.gemm_nt(dyp, s3.wt[:, :pad], n=s3.K)
    else:
        wtp = torch.zeros((s3.K, pad), dtype=BF16, device=x.device)
        wtp[:, :s3.N] = s3.wt[:, :s3.N]
        dh = Fx.gemm_nt(dyp, wtp, n=s3.K)
    dh0 = torch.empty_like(h0)
    Fx.ln_bwd(dh.contiguous(), h0, mean, rstd, ln.weight, None, None, dx16=dh0, gelu_b=ln.bias)
    return Fx.gemm_nt(dh0, s0.wt[:, :s0.N], n=s0.K) if s0.N % 64 == 0 and s0.N <= s0.wt.shape[1] else None


def _gradcam_fused(model, image, text_ids, text_atts, block_num):
    """cross_attention_gradcam(fused=True): see there."""
    import math

    from . import functional as Fx
    from . import xroberta as XR
    from .roberta_encoder import _EncoderFn
    from .roberta_layer import backward_tail
    BF16 = torch.bfloat16
    rm = _fusion_roberta(model)
    cfg = rm.config
    L, D, H = cfg.num_hidden_layers, cfg.hidden_size, cfg.num_attention_heads
    if not cfg.fusion_layer <= block_num < L:
        raise ValueError(f"block_num {block_num}: the cross-attention layers of the fusion tower are {cfg.fusion_layer} .. {L - 1}")
    scale = 1.0 / math.sqrt(D // H)
    f32 = XR._F32_STREAM
    B, T = text_ids.shape
    with torch.no_grad():
        model._ready()
        image_embeds, _ = model.get_vision_embeds(image)            # the image keys are never masked on this path
        Nenc = image_embeds.shape[1]
        enc = (image_embeds if image_embeds.dtype == BF16 else image_embeds.to(BF16)).reshape(-1, image_embeds.shape[-1]).contiguous()
        key_keep = text_atts.to(device=enc.device, dtype=torch.int32).contiguous()
        x, x32 = XR._EmbedFn.apply(rm.embeddings.word_embeddings.weight, rm.embeddings, text_ids, Fx.drop_params(0.0, 0), rm, None, f32)
        y, y32 = x.reshape(B * T, -1), (None if x32 is None else x32.reshape(B * T, -1))
        args = (key_keep, None, False, B, T, Nenc, False, None, None, None, None, f32)
        if block_num > 0:   # layers [0, block_num): plain forward, nothing kept
            y, y32 = _EncoderFn.apply(y, y32, enc, rm, key_keep, None, 0, block_num, *args[2:])
        ctx = _Ctx()        # layers [block_num, L): one _EncoderFn segment whose records stay for the walk below
        y, y32 = _EncoderFn.forward(ctx, y, y32, enc, rm, key_keep, None, block_num, L, *args[2:])
        dcls = _itm_cls_gradient(model, y.view(B, T, D)[:, 0, :])
        dy_a = torch.zeros((B * T, D), dtype=BF16, device=y.device)
        assert dcls is not None, "itm_head: the first Linear's width is not a multiple of 64"
        dy_a.view(B, T, D)[:, 0, :] = dcls
        dy_b = None         # (nobody read the output's fp32 twin: its gradient edge is empty)
        wg = _NoWgrad()
        layers = [rm.encoder.layer[li] for li in range(block_num, L)]
        q_len = key_keep.sum(dim=1).to(torch.int32)
        cam = []

        def cross_dq(dc2, r):   # a layer above block_num: the dQ kernel alone
            kv = r["kv"]
            dq2 = torch.empty_like(r["q2"])
            dkv = torch.empty((B * Nenc, 2 * D), dtype=BF16, device=dq2.device)   # (phase 1 writes neither half)
            Fx.attn_bwd(dc2, r["q2"], kv[:, :D], kv[:, D:], r["c2"], r["lse2"], dq2, dkv[:, :D], dkv[:, D:], B, H, T, Nenc, scale,
                        drop=r["d_att2"], phase=1, o_lo=r["c2lo"])
            return dq2, dkv

        def cross_cam(dc2, r):  # layer block_num: the Grad-CAM kernel on what is live here, and the walk ends
            kv = r["kv"]
            c, _, _ = attention_gradcam(r["q2"], dc2, kv[:, :D], kv[:, D:], r["lse2"], B, H, T, Nenc, scale, T, q_len=q_len)
            cam.append(c)
            return None, None
        for k in reversed(range(len(layers))):
            layer, r = layers[k], ctx.saved[k]
            dc1, dres1 = backward_tail(layer, r, dy_a, dy_b, wg, enc, cross_cam if k == 0 else cross_dq, None, param_grads=False)
            if k == 0:
                break
            s, qkv = layer._s, r["qkv"]
            dqkv = torch.empty_like(qkv)
            Fx.attn_bwd(dc1, qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], r["c1"], r["lse1"], dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:],
                        B, H, T, T, scale, key_keep=key_keep, drop=r["d_att"])
            dy_a, dy_b = Fx.gemm_nt(dqkv, s["qkv"].wt, n=s["qkv"].K), dres1
            ctx.saved[k] = None
    return cam[0]


def cross_attention_gradcam(model, image, text_ids, text_atts, block_num, fused=True):
    """The Grad-CAM maps of Grounding.py:91-115 (gradcam_mode 'itm') for one batch: fp32 [B, p, p], p = image_res // patch_size.
    cls = get_cross_embeds(get_vision_embeds(image), text_ids, text_atts)[:, 0], loss = itm_head(cls)[:, 1].sum(); at fusion layer
    `block_num`, cam = mean over heads and (padded) tokens of P[..., 1:] * clamp(dP[..., 1:], min=0) * mask.  Eval mode only.
    fused=True: the vision tower and fusion layers [0, block_num) run without autograd; layers [block_num, end) run as one _EncoderFn
      segment; the backward is the activation-gradient chain alone (no weight gradient, no dK / dV kernel, no gradient of the image
      states), and at layer block_num xfm_xattn_gradcam is called on (dc2, q2, kv, lse2) and the pass returns: that layer's own
      self-attention backward and everything below it never run, no parameter's .grad and no arena gradient buffer is touched.
    fused=False: the reference's recipe on the module contract (RobertaSelfAttention.save_attention): full backward, then the ATen
      lines of Grounding.py:101-115."""
    if model.training:
        raise RuntimeError("cross_attention_gradcam: eval mode only (call model.eval(): the maps are undefined under attention dropout)")
    if fused:
        cam = _gradcam_fused(model, image, text_ids, text_atts, block_num)
    else:
        rm = _fusion_roberta(model)
        att = rm.encoder.layer[block_num].crossattention.self
        att.save_attention = True
        try:
            image_embeds, image_atts = model.get_vision_embeds(image)
            cls = model.get_cross_embeds(image_embeds, image_atts, text_ids=text_ids, text_atts=text_atts)[:, 0, :]
            loss = model.itm_head(cls)[:, 1].sum()
            model.zero_grad()
            loss.backward()
            with torch.no_grad():
                B, Hh = image.size(0), model.num_attention_heads
                mask = text_atts.view(B, 1, -1, 1, 1)
                grads, cams = att.get_attn_gradients().detach(), att.get_attention_map().detach()
                p = int(round((cams.shape[-1] - 1) ** 0.5))
                cams = cams[:, :, :, 1:].reshape(B, Hh, -1, p, p) * mask
                grads = grads[:, :, :, 1:].clamp(min=0).reshape(B, Hh, -1, p, p) * mask
                return (cams * grads).mean(1).mean(1)
        finally:
            att.save_attention = False
            att.save_attention_map(None)
            att.save_attn_gradients(None)
    p = int(round(cam.shape[1] ** 0.5))
    return cam.view(cam.shape[0], p, p)


def val(model, data_loader, device, block_num, num_patches, fused=True):
    """Grounding.py:76-126 (gradcam_mode 'itm') on token-id batches (image, (text_ids, text_atts), ref_ids): -> (cams fp32 [N, num_patches,
    num_patches] on the device, ref ids in order).  The reference keeps one record per ref with its map; here the maps of the pass stay
    stacked on the device for grounding_eval."""
    from .task import to_device
    model.eval()
    cams, ref_ids = [], []
    for image, text, ref_id in data_loader:
        image, (text_ids, text_atts) = to_device(device, (image, text))
        cam = cross_attention_gradcam(model, image, text_ids, text_atts, block_num, fused=fused)
        assert cam.shape[1:] == (num_patches, num_patches), (cam.shape, num_patches)
        cams.append(cam)
        ref_ids.extend(int(r) for r in (ref_id.tolist() if torch.is_tensor(ref_id) else ref_id))
    return torch.cat(cams, dim=0), ref_ids
