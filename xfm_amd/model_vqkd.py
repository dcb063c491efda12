"""The frozen VQ-KD visual tokenizer (BEiT v2) behind the reference's `models/model_vqkd.py` interface, `as_tokenzer=True` side only:
`pre_process`, `encode`, `get_tokens`, `get_codebook_indices`, `get_number_of_tokens` and the constructor function
`vqkd_encoder_base_decoder_3x768x12_clip`.  It turns raw images into the codebook indices that the pre-training step's MIM head is
trained on (models/xfm.py:624-629).

  encoder             models/vqkd_vit.py VisionTransformer as model_vqkd.py:242-246 configures it: a plain pre-LN ViT-B, learned absolute
                      position embedding, no relative-position bias, no layer scale (init_values 0), `use_mean_pooling` -- so `norm` is the
                      identity, `fc_norm` the final LayerNorm, and `return_patch_tokens=True` (vqkd_vit.py:397-399) normalises the patch
                      rows.  It runs on the fused trunk node (xfm_amd/vit_trunk.py) as xfm_amd/vit.py does, with two differences: `fc_norm` is the node's final norm
                      (the CLS row is dropped afterwards: a LayerNorm is per row), and the qkv bias is the reference's `q_bias` /
                      `v_bias` pair, composed once -- cat(q_bias, 0, v_bias), vqkd_vit.py:126 -- when the arena is built.
  encode_task_layer   Linear - Tanh - Linear to code_dim (model_vqkd.py:86-90, 155): two bf16 MFMA GEMMs with fp32 outputs.
  quantize            xfm_amd.norm_ema_quantizer.NormEMAVectorQuantizer: one `xfm_vq_assign` launch.

state_dict keys of `encoder.*`, `encode_task_layer.*` and `quantize.*` equal the reference's.  The decoder, `decode_task_layer`, the
teacher and the scaling layer exist only to train the tokenizer: their keys (`decoder.*`, `decode_task_layer.*`) are ACCEPTED by
load_state_dict and NOT KEPT -- this module's state_dict does not contain them.  Every parameter has requires_grad=False and lives in
the tokenizer's own arena, outside the model's optimizer arena.  `process_type` is 'default' or 'imagenet_norm'.
"""
import math

import torch
import torch.nn as nn

from . import functional as Fx
from . import vit as _vit
from .arena import LinearSlot
from .vit_trunk import _Affine, _Dense
from .norm_ema_quantizer import NormEMAVectorQuantizer

IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # timm.data.constants


class _Attention(nn.Module):
    """vqkd_vit.py:66-121 containers: qkv without a bias of its own, q_bias / v_bias beside it."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = _Dense(dim, dim * 3, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(dim))
        self.v_bias = nn.Parameter(torch.zeros(dim))
        self.proj = _Dense(dim, dim)


class TokenizerEncoder(_vit.VisionTransformer):
    """models.vqkd_vit.VisionTransformer in the tokenizer's configuration (see the module docstring)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., layer_norm_eps=1e-6):
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, num_classes=0, embed_dim=embed_dim, depth=depth,
                         num_heads=num_heads, mlp_ratio=mlp_ratio, layer_norm_eps=layer_norm_eps)
        for blk in self.blocks:
            blk.attn = _Attention(embed_dim, num_heads)
        del self.norm                                      # nn.Identity() in the reference (use_mean_pooling): no keys
        self.fc_norm = _Affine(embed_dim, layer_norm_eps)

    @property
    def _final_norm(self):
        return self.fc_norm

    def _qkv_bias_parts(self, blk):
        return [blk.attn.q_bias, self.embed_dim, blk.attn.v_bias]   # cat(q_bias, 0, v_bias), vqkd_vit.py:126

    def forward(self, x, return_patch_tokens=True):
        if not return_patch_tokens:
            raise NotImplementedError("the tokenizer reads the patch tokens only (model_vqkd.py:152)")
        return super().forward(x)[:, 1:]   # bf16 [B, N, D]: fc_norm of the patch rows


class VQKD(nn.Module):
    def __init__(self, encoder_config, decoder_config=None, n_embed=8192, embed_dim=32, decay=0.99, process_type='default',
                 quantize_kmeans_init=True, teacher_model_type='None', decoder_out_dim=512, rec_loss_type='cosine', **kwargs):
        super().__init__()
        if teacher_model_type not in (None, 'None'):
            raise NotImplementedError("VQKD: only the tokenizer side (as_tokenzer=True, no teacher) is built; training the tokenizer is out of scope")
        if process_type not in ('default', 'imagenet_norm'):
            raise NotImplementedError(f"VQKD: process_type {process_type!r} (model_vqkd.py:125-136 handles 'default' and 'imagenet_norm')")
        ec = dict(encoder_config)
        expect = dict(in_chans=3, qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., init_values=0.,
                      use_abs_pos_emb=True, use_rel_pos_bias=False, use_shared_rel_pos_bias=False, use_mean_pooling=True)
        bad = {k: ec[k] for k, v in expect.items() if k in ec and ec[k] != v}
        if bad:
            raise NotImplementedError(f"VQKD encoder: unsupported {bad} (model_vqkd.py:242-246 is the configuration built)")
        self.encoder = TokenizerEncoder(img_size=ec['img_size'], patch_size=ec['patch_size'], embed_dim=ec['embed_dim'], depth=ec['depth'],
                                        num_heads=ec['num_heads'], mlp_ratio=ec.get('mlp_ratio', 4.))
        self.quantize = NormEMAVectorQuantizer(n_embed=n_embed, embedding_dim=embed_dim, beta=1.0, kmeans_init=quantize_kmeans_init,
                                               decay=decay)
        self.patch_size = ec['patch_size']
        self.token_shape = (ec['img_size'] // self.patch_size, ec['img_size'] // self.patch_size)
        self.encode_task_layer = nn.Sequential(nn.Linear(ec['embed_dim'], ec['embed_dim']), nn.Tanh(), nn.Linear(ec['embed_dim'], embed_dim))
        for m in (self.encode_task_layer[0], self.encode_task_layer[2]):   # model_vqkd.py:107-111
            nn.init.trunc_normal_(m.weight, std=.02)
            nn.init.constant_(m.bias, 0)
        self.process_type = process_type
        self.kwargs = kwargs
        for p in self.parameters():
            p.requires_grad = False
        self._arena = None
        self._register_load_state_dict_pre_hook(self._drop_training_half)
        self.eval()

    @staticmethod
    def _drop_training_half(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """`decoder.*` and `decode_task_layer.*` -- the half of a VQ-KD checkpoint that only trains the tokenizer -- are accepted and
        dropped, whether the tokenizer is loaded on its own or as the `vqkd.` part of a model."""
        for k in [k for k in state_dict if k.startswith((prefix + "decoder.", prefix + "decode_task_layer."))]:
            del state_dict[k]

    # ---- plumbing -------------------------------------------------------------------------------
    def train(self, mode=True):
        """The tokenizer is frozen: it stays in eval mode whatever the model around it is switched to (the reference builds it with
        .eval(), xfm.py:107-109, and runs it under no_grad; its encoder has no dropout and no drop path, so only the quantizer's
        code-usage bookkeeping tells the modes apart -- and training the quantizer is out of scope)."""
        return super().train(False)

    @property
    def device(self):
        return self.encoder.cls_token.device

    def finalize(self, device=None):
        """The tokenizer's own arena (outside the optimizer arena of the model that holds it) and the two task-layer GEMM operands."""
        from .arena import ParamArena
        device = device or self.device
        l0, l2 = self.encode_task_layer[0], self.encode_task_layer[2]
        self._s_task0 = LinearSlot("encode_task_layer.0", [l0.weight], [l0.bias])
        self._s_task2 = LinearSlot("encode_task_layer.2", [l2.weight], [l2.bias])
        for s in (self._s_task0, self._s_task2):
            s.need_t = False   # no backward: the transposed copies are never read
        self._arena = ParamArena(self, self.encoder.linear_slots() + [self._s_task0, self._s_task2], device)
        self.encoder.attach(self._arena)
        return self

    def _ready(self):
        if self._arena is None or not self._arena.attached():
            self.finalize()

    # ---- the reference's interface --------------------------------------------------------------
    def pre_process(self, data):
        """model_vqkd.py:125-136.  'default': images in [0, 1] are scaled to [0, 255] first -- the reference's `if data.max() <= 1.` as a
        device-side select, so no host read sits on the step (x * 1.0 is x: the same bits either way)."""
        data = data.to(self.device)
        if self.process_type == 'default':
            scale = torch.where(data.max() <= 1., 255., 1.).to(data.dtype)
            data = data * scale
            data = data / 127.5 - 1.0
        else:
            mean = torch.as_tensor(IMAGENET_DEFAULT_MEAN, device=self.device)[None, :, None, None]
            std = torch.as_tensor(IMAGENET_DEFAULT_STD, device=self.device)[None, :, None, None]
            data = (data - mean) / std
        return data

    def get_number_of_tokens(self):
        return self.quantize.num_tokens

    def encode_features(self, x):
        """Pre-processed images -> the features handed to the quantizer, fp32 [B, N, code_dim] (model_vqkd.py:152-155)."""
        self._ready()
        with torch.no_grad():
            feats = self.encoder(x, return_patch_tokens=True)
            B, N, D = feats.shape
            h = Fx.gemm_nt(feats.reshape(B * N, D).contiguous(), self._s_task0.wb, self._s_task0.b, epi=Fx.EPI_F32)
            h = torch.tanh(h).to(torch.bfloat16)
            return Fx.gemm_nt(h, self._s_task2.wb, self._s_task2.b, epi=Fx.EPI_F32).view(B, N, -1)

    def encode(self, x):
        """(quantize [B, c, h, w], embed_ind [B*h*w], loss) as model_vqkd.py:151-163."""
        f = self.encode_features(x)
        B, N, C = f.shape
        h = w = int(math.sqrt(N))
        with torch.no_grad():
            quantize, loss, embed_ind = self.quantize(f.view(B, h, w, C).permute(0, 3, 1, 2))
        return quantize, embed_ind, loss

    def get_tokens(self, data, **kwargs):
        """model_vqkd.py:141-149.  z_q and the commitment loss are not needed here, so they are not computed."""
        data = self.pre_process(data)
        f = self.encode_features(data)
        with torch.no_grad():
            embed_ind = self.quantize.assign(f.view(-1, f.shape[-1]))
        return {'token': embed_ind.view(data.shape[0], -1), 'input_img': data}

    def get_codebook_indices(self, x, **kwargs):
        return self.get_tokens(x, **kwargs)['token']

    def forward(self, x, **kwargs):
        raise NotImplementedError("VQKD.forward is the tokenizer's training step (teacher, decoder, reconstruction loss): out of scope")


def get_model_default_params():
    return dict(img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.,
                qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., init_values=0., use_abs_pos_emb=True,
                use_rel_pos_bias=False, use_shared_rel_pos_bias=False, use_mean_pooling=True, init_scale=0.001)


def vqkd_encoder_base_decoder_3x768x12_clip(pretrained=False, pretrained_weight=None, as_tokenzer=False, img_size=224, n_code=8192,
                                            code_dim=32, encoder_depth=12, **kwargs):
    """model_vqkd.py:292-334 with as_tokenzer=True.  `pretrained_weight`: a checkpoint path ({'model' | 'state_dict': ...}; `loss*`,
    `teacher*` and `scaling*` keys are dropped as there); None builds the module with fresh weights for a later load_state_dict
    (extension: the reference asserts a path).  `encoder_depth` (extension): a shallower encoder for tests."""
    if not as_tokenzer:
        raise NotImplementedError("vqkd_encoder_base_decoder_3x768x12_clip: only as_tokenzer=True is built (training the tokenizer is out of scope)")
    encoder_config = get_model_default_params()
    encoder_config['img_size'] = img_size
    encoder_config['num_classes'] = 0
    encoder_config['depth'] = encoder_depth
    kwargs.pop("teacher_model_type", None)
    model = VQKD(encoder_config, None, n_code, code_dim, teacher_model_type='None', decoder_out_dim=512, **kwargs)
    if pretrained_weight is not None:
        if pretrained_weight.startswith('https'):
            raise NotImplementedError("downloading tokenizer weights: pass a local checkpoint path")
        weights = torch.load(pretrained_weight, map_location='cpu')
        weights = weights['model'] if 'model' in weights else weights["state_dict"]
        for k in list(weights.keys()):
            if k.startswith(("loss", "teacher", "scaling")):
                del weights[k]
        model.load_state_dict(weights)
    return model
