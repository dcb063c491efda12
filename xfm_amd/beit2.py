"""BEiT-v2 vision tower on the HIP hot path, behind the reference's interface.

Mirrors `models/beit2.py::VisionTransformer` of the reference (constructor keywords :272-281, forward :477-481,
forward_avgpool :423-466, state_dict keys) for the configuration every shipped YAML uses: relative-position bias
per block, layer-scale gammas, q/v-only bias, mean-pooled pseudo-cls, no absolute position embedding.  The twelve
blocks run as ONE autograd node whose forward/backward are explicit sequences of C-ABI kernel launches
(xfm_amd.functional); PyTorch autograd only sees the patch/cls assembly before it and the pooling after it.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import functional as Fx
from .arena import grad_of
# the containers, the trunk node and its knobs live in vit_trunk.py and stay importable from here; the knob names are read-only copies
# (the live values are vit_trunk's: assigning to one here changes nothing)
from .vit_trunk import (_DEFER_LN, _DEFER_WGRAD, _FAST_DELTA, _GRAD_CHUNK_BLOCKS, _RELPOS_AHEAD, _VIT_FUSED_BWD,  # noqa: F401
                        _WGRAD_GROUP_BLOCKS, PatchEmbed, _Affine, _Dense, _FusedViT, _TrunkFn)


class BlockMaskGenerator:
    """Block-wise MIM mask sampler with the distribution of the reference's MaskingGenerator
    (models/masking_generator.py:27-105): rectangles of area U[min, remaining] and log-uniform aspect in [0.3, 1/0.3],
    accepted when they add between 1 and `remaining` new patches, then trimmed / topped up to exactly `num_masking`."""

    def __init__(self, input_size, num_masking_patches, min_num_patches=4, min_aspect=0.3, seed=None):
        self.h = self.w = int(input_size)
        self.num = num_masking_patches
        self.min_num = min_num_patches
        self.log_aspect = (math.log(min_aspect), math.log(1.0 / min_aspect))
        self.rng = np.random.default_rng(seed)
        self._seed0 = 0 if seed is None else int(seed)

    def _one(self):
        rng, H, W = self.rng, self.h, self.w
        mask = np.zeros((H, W), dtype=bool)
        count = 0
        while count < self.num:
            budget = self.num - count
            delta = 0
            for _ in range(10):
                area = self.min_num + (budget - self.min_num) * rng.random()  # like random.uniform: fine when budget < min
                ar = math.exp(rng.uniform(*self.log_aspect))
                h, w = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
                if w < W and h < H:
                    top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
                    sub = mask[top:top + h, left:left + w]
                    new = h * w - int(sub.sum())
                    if 0 < new <= budget:
                        sub[...] = True
                        delta = new
                        break
            if delta == 0:
                break
            count += delta
        flat = mask.reshape(-1)
        if count < self.num:
            free = np.flatnonzero(~flat)
            flat[rng.choice(free, self.num - count, replace=False)] = True
        elif count > self.num:
            used = np.flatnonzero(flat)
            flat[rng.choice(used, count - self.num, replace=False)] = False
        return flat

    def batch(self, n, device=None):
        """[n, h*w] bool.  On a HIP device the masks are DRAWN there (csrc/mim.hip mim_masks_kernel: one wavefront per image
        runs the same rejection loop with a counter-based generator; ~10 us for a batch instead of n Python rejection loops on the
        thread that also enqueues the step's kernels, beit2.py:432-439 of the reference).  On the CPU: the numpy sampler."""
        if device is not None and torch.device(device).type == "cuda":
            self._draws = getattr(self, "_draws", 0) + 1
            seed = ((torch.initial_seed() & 0xFFFFFFFF) << 32) | ((self._seed0 + self._draws) & 0xFFFFFFFF)
            return Fx.mim_masks(n, self.h, self.num, self.min_num, device, seed, min_aspect=math.exp(self.log_aspect[0]),
                                max_aspect=math.exp(self.log_aspect[1]))
        return torch.from_numpy(np.stack([self._one() for _ in range(n)], 0))


def build_relative_position_index(gh, gw):
    """[gh*gw+1]^2 int64 index into the (2gh-1)(2gw-1)+3 row bias table; last three rows are cls->tok, tok->cls,
    cls->cls (same values as beit2.py:92-116)."""
    n = gh * gw
    nrd = (2 * gh - 1) * (2 * gw - 1) + 3
    r = torch.arange(n)
    y, x = r // gw, r % gw
    rel = (y[:, None] - y[None, :] + gh - 1) * (2 * gw - 1) + (x[:, None] - x[None, :] + gw - 1)
    idx = torch.full((n + 1, n + 1), nrd - 1, dtype=torch.int64)
    idx[1:, 1:] = rel
    idx[0, 1:] = nrd - 3
    idx[1:, 0] = nrd - 2
    return idx


class Attention(nn.Module):
    def __init__(self, dim, num_heads, window_size):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = _Dense(dim, dim * 3, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(dim))
        self.v_bias = nn.Parameter(torch.zeros(dim))
        self.window_size = window_size
        nrd = (2 * window_size[0] - 1) * (2 * window_size[1] - 1) + 3
        self.relative_position_bias_table = nn.Parameter(torch.zeros(nrd, num_heads))
        self.register_buffer("relative_position_index", build_relative_position_index(*window_size))
        self.proj = _Dense(dim, dim)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = _Dense(dim, hidden)
        self.fc2 = _Dense(hidden, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, init_values, window_size, drop_path, eps):
        super().__init__()
        self.norm1 = _Affine(dim, eps)
        self.attn = Attention(dim, num_heads, window_size)
        self.norm2 = _Affine(dim, eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.gamma_1 = nn.Parameter(init_values * torch.ones(dim))
        self.gamma_2 = nn.Parameter(init_values * torch.ones(dim))
        self.drop_path_prob = float(drop_path)


class _RegionPoolFn(torch.autograd.Function):
    """xfm_region_pool_fwd / bwd: the gather and the pooled row in one pass; the backward sums the samples of an image in ascending
    order without atomics (ATen's index_select backward is an atomic index_add: not reproducible once two samples share an image)."""

    @staticmethod
    def forward(ctx, full, idx32, atts_u8):
        out, wsum = Fx.region_pool_fwd(full, idx32, atts_u8)
        ctx.save_for_backward(idx32, atts_u8, wsum)
        ctx.n_img = full.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        idx32, atts_u8, wsum = ctx.saved_tensors
        return Fx.region_pool_bwd(dout.contiguous(), idx32, atts_u8, wsum, ctx.n_img), None, None


REGION_GLUE_FUSED = os.environ.get("XFM_REGION_GLUE", "1") != "0"   # A/B knob (tools/bench_region_step.py): 0 = the ATen glue on the device too


def region_outputs(full, idx_to_group_img, image_atts):
    """The region call form's per-sample output (beit2.py:467-475): sample i reads the normalised patch rows of image
    idx_to_group_img[i] and pools its own pseudo-cls as their image_atts-weighted mean (fp32 sums, one rounding to the tower's
    bf16).  HIP tensors: one kernel each way (_RegionPoolFn).  CPU tensors: the same arithmetic as differentiable ATen ops."""
    if full.is_cuda and full.dtype == torch.bfloat16 and REGION_GLUE_FUSED:
        atts = image_atts.to(device=full.device)[:, 1:]
        assert atts.shape == (idx_to_group_img.numel(), full.shape[1] - 1), "image_atts is [bs, 1 + patches]"
        return _RegionPoolFn.apply(full.contiguous(), idx_to_group_img.to(device=full.device, dtype=torch.int32).view(-1).contiguous(),
                                   atts.to(torch.uint8).contiguous())
    idx = idx_to_group_img.to(device=full.device, dtype=torch.long).view(-1)
    x_bs = full[:, 1:, :].index_select(0, idx)
    w = image_atts.to(device=full.device)[:, 1:].to(torch.float32)
    assert w.shape == x_bs.shape[:2], "image_atts is [bs, 1 + patches]"
    cls = torch.einsum("bp,bpd->bd", w, x_bs.float()) / w.sum(dim=1, keepdim=True)
    return torch.cat([cls.to(full.dtype).unsqueeze(1), x_bs], dim=1)


class _TokensFn(torch.autograd.Function):
    """x0 = cat(cls, where(mask, mask_token, tok[b mod Bt])) in fp32; the cls / mask-token gradients are accumulated straight into
    the gradient arena."""

    @staticmethod
    def forward(ctx, tok, cls_token, mask_token, mask_u8, Bx):
        ctx.mask, ctx.Bt = mask_u8, tok.shape[0]
        ctx.cls_token, ctx.mask_token = cls_token, mask_token
        return Fx.vit_tokens_fwd(tok.contiguous(), cls_token.detach().reshape(-1), mask_token.detach().reshape(-1), mask_u8, Bx)

    @staticmethod
    def backward(ctx, dx0):
        dmask = grad_of(ctx.mask_token).view(-1) if ctx.mask is not None else None
        dtok = Fx.vit_tokens_bwd(dx0.contiguous(), ctx.mask, ctx.Bt, grad_of(ctx.cls_token).view(-1), dmask)
        return dtok, None, None, None, None


class VisionTransformer(_FusedViT):
    """Drop-in for models.beit2.VisionTransformer (BEiT-v2 configuration used by XFM)."""
    _rel_pos = True
    _pool_tail = True  # forward_avgpool (beit2.py:455-466): the trunk node replaces the cls row by the mean of the patch rows
    _draw_at_rate_zero = True  # drop-path scales are drawn on every training forward: the device RNG advances even when no block drops

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 norm_layer=None, init_values=0.1, use_abs_pos_emb=False, use_rel_pos_bias=True,
                 use_shared_rel_pos_bias=False, use_mean_pooling=True, init_scale=0.001, local_attn_depth=-1,
                 num_masking_patches=75, min_num_patches=16, layer_norm_eps=1e-6):
        super().__init__()
        unsupported = []
        if use_abs_pos_emb: unsupported.append("use_abs_pos_emb")
        if not use_rel_pos_bias: unsupported.append("use_rel_pos_bias=False")
        if use_shared_rel_pos_bias: unsupported.append("use_shared_rel_pos_bias")
        if not use_mean_pooling: unsupported.append("use_mean_pooling=False")
        if local_attn_depth > 0: unsupported.append("local_attn_depth>0")
        if not qkv_bias: unsupported.append("qkv_bias=False")
        if not init_values or init_values <= 0: unsupported.append("init_values<=0")
        if drop_rate or attn_drop_rate: unsupported.append("drop_rate/attn_drop_rate")
        if (embed_dim // num_heads) != 64: unsupported.append("head_dim != 64")
        if unsupported:
            raise NotImplementedError("xfm_amd.beit2 implements the BEiT-v2 configuration XFM ships "
                                      f"(xfm.py:206-234); unsupported: {unsupported}")
        self.local_attn_depth = local_attn_depth
        self.depth, self.num_heads = depth, num_heads
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.mask_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = None
        self.generator = BlockMaskGenerator(img_size // patch_size, num_masking_patches, min_num_patches)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth, device="cpu")]
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, init_values, self.patch_embed.patch_shape,
                                           dpr[i], layer_norm_eps) for i in range(depth)])
        self.fc_norm = _Affine(embed_dim, layer_norm_eps)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        nn.init.trunc_normal_(self.mask_token, std=.02)
        for i, blk in enumerate(self.blocks):  # fix_init_weight, beit2.py:327-333
            blk.attn.proj.weight.data.div_(math.sqrt(2.0 * (i + 1)))
            blk.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (i + 1)))

    @property
    def _final_norm(self):
        return self.fc_norm

    def _qkv_bias_parts(self, blk):
        return [blk.attn.q_bias, self.embed_dim, blk.attn.v_bias]   # no k bias: D structural zeros between the two

    def attach(self, arena):
        super().attach(arena)
        self._index32 = self.blocks[0].attn.relative_position_index.to(device=arena.device, dtype=torch.int32).contiguous()
        self._relpos_order, self._relpos_start = Fx.relpos_sorted_index(
            self._index32, self.blocks[0].attn.relative_position_bias_table.shape[0])

    # ---- forward --------------------------------------------------------------------------------
    def forward(self, x, idx_to_group_img=None, image_atts=None, do_mask=False, ids_mask=None, drop_path_scales=None, split_stream=None):
        """`split_stream` (extension; with `ids_mask` holding k = 2 views of the B images): the views share the patch embedding and
        the token assembly, but each runs the trunk as its own pass -- view 0 on the current stream, view 1 on `split_stream` -- and
        the result is the pair (out0, out1) instead of one [2B, N, D] tensor; out1 lives on `split_stream` (the caller joins).
        Autograd replays each pass's backward on its forward stream."""
        if (idx_to_group_img is None) != (image_atts is None):
            raise ValueError("the region call form takes idx_to_group_img AND image_atts (beit2.py:467-475)")
        if idx_to_group_img is not None and (do_mask or split_stream is not None):
            raise ValueError("the region call form has no masked view (beit2.py:467-475)")
        self._ready()
        B = x.shape[0]
        tok = self._patch_tokens(x)
        mask_u8 = None
        if do_mask:
            if ids_mask is None:
                ids_mask = self.generator.batch(B, x.device)
            ids_mask = ids_mask.to(device=x.device, dtype=torch.bool).contiguous()
            # several masked views of the SAME images in one pass: ids_mask [k * B, P] against B images (the pre-training step's
            # clean + MIM-masked pair) -- patch gather, patch-embed GEMM and its weight gradient run once per image
            assert ids_mask.shape[0] % B == 0, "ids_mask rows must be a multiple of the image batch"
            mask_u8 = ids_mask.view(torch.uint8)
            B = ids_mask.shape[0]
        # mask-token mix + cls concat (beit2.py:432-446) as one kernel, forward and backward
        x0 = _TokensFn.apply(tok, self.cls_token, self.mask_token, mask_u8, B)
        dp = drop_path_scales if drop_path_scales is not None else self._drop_path_scales(B, x.device)
        if split_stream is not None and do_mask and B == 2 * x.shape[0]:
            Bh = x.shape[0]
            main = torch.cuda.current_stream(x.device)
            out0 = _TrunkFn.apply(x0[:Bh], self, None if dp is None else dp[:, :, :Bh].contiguous())
            split_stream.wait_stream(main)   # (x0 and the drop-path draws are ready; the first view's kernels are merely queued ahead)
            with torch.cuda.stream(split_stream):
                out1 = _TrunkFn.apply(x0[Bh:], self, None if dp is None else dp[:, :, Bh:].contiguous())
            x0.record_stream(split_stream)
            return (out0, out1), ids_mask
        out = _TrunkFn.apply(x0, self, dp)           # bf16 [B, N, D]: fc_norm on every row, then row 0 <- mean of the patch rows
        if idx_to_group_img is not None:
            return region_outputs(out, idx_to_group_img, image_atts), out
        return (out, ids_mask) if do_mask else out


def interpolate_rel_pos_bias(rel_pos_bias, dst_num_pos, dst_patch_shape):
    """Relative-position table [src_num_pos, heads] -> [dst_num_pos, heads] for another patch grid (fine-tuning at 384 / 480 px),
    beit2.py:763-821: the (2s-1)^2 grid part is resampled from geometric-progression source coordinates to the integer target
    coordinates with a bicubic interpolating spline, the 3 extra (cls) entries are carried over.

    The reference calls `scipy.interpolate.interp2d(x, y, z, kind='cubic')`, removed in SciPy 1.14 (this image has 1.15); for a regular
    grid that was FITPACK's interpolating tensor-product spline (`regrid_smth` with s = 0, evaluated by `bispev`), which
    `RectBivariateSpline(kx=3, ky=3, s=0)` reaches through the same routines.  Pinned by tests/golden/relpos_interp.npz: the
    reference's own `interpolate_pos_embed` run on a formula table (224 -> 384 / 480 px) with the removed call supplied by a
    from-source restatement of it (the CPU suite holds this function to that fixture at 1e-6)."""
    import numpy as np
    from scipy.interpolate import RectBivariateSpline
    src_num_pos, num_attn_heads = rel_pos_bias.shape
    if dst_patch_shape[0] != dst_patch_shape[1]:
        raise NotImplementedError()
    num_extra_tokens = dst_num_pos - (dst_patch_shape[0] * 2 - 1) * (dst_patch_shape[1] * 2 - 1)
    src_size = int((src_num_pos - num_extra_tokens) ** 0.5)
    dst_size = int((dst_num_pos - num_extra_tokens) ** 0.5)
    if src_size == dst_size:
        return rel_pos_bias
    extra_tokens = rel_pos_bias[-num_extra_tokens:, :]
    grid = rel_pos_bias[:-num_extra_tokens, :]
    x = rel_pos_source_coordinates(src_size, dst_size)
    t = dst_size // 2.0
    dx = np.arange(-t, t + 0.1, 1.0)
    out = []
    for i in range(num_attn_heads):
        z = grid[:, i].view(src_size, src_size).float().numpy().astype(np.float64)  # z[j, i] sits at (x[i], y[j]), interp2d's convention
        f = RectBivariateSpline(x, x, z, kx=3, ky=3, s=0)                            # first axis = y: f(dy, dx)[j, i]
        out.append(torch.tensor(f(dx, dx), dtype=torch.float32).contiguous().view(-1, 1).to(rel_pos_bias.device))
    return torch.cat((torch.cat(out, dim=-1), extra_tokens), dim=0)


def rel_pos_source_coordinates(src_size, dst_size):
    """beit2.py:780-803: source relative offsets placed on a geometric progression whose half-extent matches the target's."""
    def geometric_progression(a, r, n):
        return a * (1.0 - r ** n) / (1.0 - r)

    left, right = 1.01, 1.5
    while right - left > 1e-6:
        q = (left + right) / 2.0
        gp = geometric_progression(1, q, src_size // 2)
        if gp > dst_size // 2:
            right = q
        else:
            left = q
    dis, cur = [], 1
    for i in range(src_size // 2):
        dis.append(cur)
        cur += q ** (i + 1)
    return [-d for d in reversed(dis)] + [0] + dis


def load_pretrained_beit2(model, ckpt_rpath):
    """beit2.py:572-660: unwrap `model` / `module`, drop the classification head and the `relative_position_index` buffers, expand
    a shared relative-position table to every block, resample tables of another grid size (`interpolate_rel_pos_bias`), load with
    strict=False."""
    checkpoint = torch.load(ckpt_rpath, map_location='cpu')
    checkpoint_model = None
    for model_key in ('model', 'module'):
        if model_key in checkpoint:
            checkpoint_model = checkpoint[model_key]
            break
    if checkpoint_model is None:
        checkpoint_model = checkpoint
    for k in ('head.weight', 'head.bias'):
        checkpoint_model.pop(k, None)
    if "rel_pos_bias.relative_position_bias_table" in checkpoint_model:
        shared = checkpoint_model.pop("rel_pos_bias.relative_position_bias_table")
        for i in range(len(model.blocks)):
            checkpoint_model["blocks.%d.attn.relative_position_bias_table" % i] = shared.clone()
    own = model.state_dict()
    for key in list(checkpoint_model.keys()):
        if "relative_position_index" in key:
            checkpoint_model.pop(key)
        elif "relative_position_bias_table" in key and key in own and own[key].shape != checkpoint_model[key].shape:
            checkpoint_model[key] = interpolate_rel_pos_bias(checkpoint_model[key], own[key].shape[0], model.patch_embed.patch_shape)
    msg = model.load_state_dict(checkpoint_model, strict=False)
    if getattr(model, "_arena", None) is not None:
        model._arena.bump()
    return msg


def beit_base_patch16(img_size, depth=12, **kwargs):
    return VisionTransformer(img_size=img_size, patch_size=16, embed_dim=768, depth=depth, num_heads=12, mlp_ratio=4,
                             layer_norm_eps=1e-6, **kwargs)
