"""RoBERTa text / fusion towers on the HIP hot path, behind the reference's interface.

Mirrors `models/xroberta.py` of the reference: RobertaModel.forward (:817-957, incl. the `encoder_embeds` bypass
:920-929 and `mode` layer ranges :504-516), RobertaForMaskedLM (:1157-1310, `.bert()` method, `masked_pos` gather,
two LM heads), RobertaForCausalLM-style decoding mask (`is_decoder`), and the state_dict key names.  The layer stack
runs as ONE autograd node: per layer a fused QKV GEMM, LDS-resident attention, output GEMM, fused
dropout+residual+LayerNorm, (cross-attention with a fused K/V GEMM over the image tokens), GELU-fused FFN.
`scale_after_qk=True` selects the xbert.py:329-330 ordering (same kernels: the scale is applied to the fp32 scores).
"""
import json
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import functional as Fx
from .arena import LinearSlot, OwnsArena, ParamArena, arena_note_grad, arena_note_use
from .vit_trunk import _Affine
from .decode import GenerationMixin, cached_forward
from .ops import grad_view, lm_head_ce, lm_head_logits
from .roberta_encoder import _EncoderFn, _LastLayerRowsFn, layer_saves_maps
from .roberta_layer import _next_seed, _seed_counter  # noqa: F401  (_seed_counter: THE list the executors advance, written as XR._seed_counter[0])
from .roberta_native import _KV_AHEAD, _RL_DEFER_LN, _RL_DEFER_WGRAD, _EncoderFnNative  # noqa: F401  (the knobs' defaults are read here)
from .side_stream import _WgradStream

BF16, F32 = torch.bfloat16, torch.float32


class RobertaConfig:
    """The subset of transformers' RobertaConfig the path reads (xfm.py:273-284,482-486,528-531)."""

    def __init__(self, **kw):
        d = dict(vocab_size=50265, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, max_position_embeddings=514,
                 type_vocab_size=1, initializer_range=0.02, layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0,
                 eos_token_id=2, fusion_layer=12, encoder_width=768, add_cross_attention=False)
        d.update(kw)
        self.__dict__.update(d)

    @classmethod
    def from_json_file(cls, path):
        with open(path) as f:
            return cls(**json.load(f))


class _Lin(nn.Module):
    def __init__(self, fin, fout, std):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(fout, fin).normal_(0.0, std))
        self.bias = nn.Parameter(torch.zeros(fout))


class _Emb(nn.Module):
    def __init__(self, n, dim, std, padding_idx=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, dim).normal_(0.0, std))
        self.padding_idx = padding_idx
        if padding_idx is not None:
            with torch.no_grad():
                self.weight[padding_idx].zero_()


class RobertaEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        std = config.initializer_range
        self.word_embeddings = _Emb(config.vocab_size, config.hidden_size, std, config.pad_token_id)
        self.position_embeddings = _Emb(config.max_position_embeddings, config.hidden_size, std, config.pad_token_id)
        self.token_type_embeddings = _Emb(config.type_vocab_size, config.hidden_size, std)
        self.LayerNorm = _Affine(config.hidden_size, config.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(config.max_position_embeddings).expand((1, -1)))
        self.padding_idx = config.pad_token_id
        self.p_drop = config.hidden_dropout_prob


_F32_STREAM = os.environ.get("XFM_F32_STREAM", "1") != "0"
"""The residual stream of the text / fusion towers in fp32 (A/B knob; 0 = the bf16 stream of rounds 1-4).  The reference trains in mixed
precision: its Linears produce 16-bit outputs, but LayerNorm and the residual add run in fp32 (apex O1 / autocast lists), so every
post-LN sum `LayerNorm(dropout(h) + x)` (xroberta.py:300-304, 381-385) sees the UN-ROUNDED output of the previous LayerNorm and the
gradient of the residual branch travels in fp32 too.  With the stream on, every tower hand-over is a (bf16, fp32) pair: the bf16 tensor
feeds the GEMMs, its fp32 twin the next residual add; the two are separate autograd edges (bf16 gradient from the GEMM side, fp32 from
the LayerNorm side)."""

_NATIVE_LAYERS = os.environ.get("XFM_NATIVE_LAYERS", "1") != "0"  # A/B knob: one C-ABI call per RobertaLayer (roberta_native, csrc/encoder.hip)


def twin_of(t):
    """The fp32 twin of a tower output (None when there is none)."""
    return getattr(t, "_xfm_f32", None) if _F32_STREAM else None


def with_twin(t, t32):
    """Attach the fp32 twin to a tower output / to a row-wise image of one (cat / index_select / gather of both)."""
    if t32 is not None and _F32_STREAM:
        t._xfm_f32 = t32
    return t


def rowwise(fn, *tensors):
    """fn applied to tower outputs AND, when every one of them has one, to their fp32 twins: for the row-wise glue between towers
    (torch.cat / index_select / detach / row gathers), so the twin follows the rows into the next tower."""
    out = fn(*tensors)
    twins = [twin_of(t) for t in tensors]
    if all(tw is not None for tw in twins):
        with_twin(out, fn(*twins))
    return out


class _EmbedFn(torch.autograd.Function):
    """-> (y bf16, y fp32 twin or None).  The twin exists when the fp32 stream is on; its gradient (fp32) is added to y's."""

    @staticmethod
    def forward(ctx, anchor, emb, input_ids, drop, owner, pack, f32):
        ids = input_ids.contiguous()
        ctx.owner = owner if ctx.needs_input_grad[0] else None
        if ctx.owner is not None:
            arena_note_use(owner)
        ctx.set_materialize_grads(False)
        ln = emb.LayerNorm
        row_map = None if pack is None else pack.row_map()  # packed (unpadded) output rows, xfm_amd.packing
        out = Fx.embed_ln_fwd(ids, emb.word_embeddings.weight, emb.position_embeddings.weight,
                              emb.token_type_embeddings.weight, ln.weight, ln.bias, ln.eps,
                              emb.padding_idx, drop, getattr(emb, "pos_mode", 0), row_map=row_map,
                              out_rows=None if pack is None else pack.cap, y32=f32)
        y, mean, rstd, pos_ids = out[:4]
        y32 = out[4] if f32 else None
        ctx.emb, ctx.saved, ctx.drop, ctx.row_map = emb, (ids, mean, rstd, pos_ids), drop, row_map
        if pack is None:
            y = y.view(ids.shape[0], ids.shape[1], -1)
            y32 = None if y32 is None else y32.view(ids.shape[0], ids.shape[1], -1)
        return y, y32

    @staticmethod
    def backward(ctx, dy, dy32=None):
        emb = ctx.emb
        ids, mean, rstd, pos_ids = ctx.saved
        ln = emb.LayerNorm
        if dy is None and dy32 is None:
            return (None,) * 7
        if dy is None:
            dy = torch.zeros(dy32.shape, dtype=BF16, device=dy32.device)
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        if dy2.dtype != BF16:
            dy2 = dy2.to(BF16)
        if dy32 is not None:
            dy32 = dy32.reshape(-1, dy32.shape[-1]).contiguous()
        Fx.embed_ln_bwd(dy2, ids, emb.word_embeddings.weight, emb.position_embeddings.weight,
                        emb.token_type_embeddings.weight, ln.weight, ln.bias, ln.eps, emb.padding_idx, mean, rstd, pos_ids,
                        grad_view(emb.word_embeddings.weight), grad_view(emb.position_embeddings.weight),
                        grad_view(emb.token_type_embeddings.weight).view(-1), grad_view(ln.weight), grad_view(ln.bias), ctx.drop,
                        getattr(emb, "pos_mode", 0), row_map=ctx.row_map, dy32=dy32)
        if ctx.owner is not None:
            arena_note_grad(ctx.owner)
        return (None,) * 7


class RobertaSelfAttention(nn.Module):
    def __init__(self, config, is_cross_attention):
        super().__init__()
        std = config.initializer_range
        kv_in = config.encoder_width if is_cross_attention else config.hidden_size
        self.query = _Lin(config.hidden_size, config.hidden_size, std)
        self.key = _Lin(kv_in, config.hidden_size, std)
        self.value = _Lin(kv_in, config.hidden_size, std)
        # The attention-map contract of the reference's cross-attention (xroberta.py:182-194, 268-270), on cross-attention layers only and
        # in eval mode only: with save_attention = True the layer's pass runs kernel by kernel on every query row, the forward leaves
        # softmax(scores) and a backward the gradient that reaches it, both fp32 [B, H, T, Sk] with the rows past a sequence's length zero
        # (roberta_encoder.save_layer_maps; the fused attention itself never materialises a probability).
        self.save_attention = False
        self.attention_map = None
        self.attn_gradients = None

    def save_attn_gradients(self, attn_gradients):
        self.attn_gradients = attn_gradients

    def get_attn_gradients(self):
        return self.attn_gradients

    def save_attention_map(self, attention_map):
        self.attention_map = attention_map

    def get_attention_map(self):
        return self.attention_map


class RobertaSelfOutput(nn.Module):
    def __init__(self, config, fin=None):
        super().__init__()
        self.dense = _Lin(fin or config.hidden_size, config.hidden_size, config.initializer_range)
        self.LayerNorm = _Affine(config.hidden_size, config.layer_norm_eps)


class RobertaAttention(nn.Module):
    def __init__(self, config, is_cross_attention=False):
        super().__init__()
        self.self = RobertaSelfAttention(config, is_cross_attention)
        self.output = RobertaSelfOutput(config)


class RobertaIntermediate(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = _Lin(config.hidden_size, config.intermediate_size, config.initializer_range)


class RobertaLayer(nn.Module):
    def __init__(self, config, layer_num):
        super().__init__()
        self.attention = RobertaAttention(config)
        self.has_cross_attention = layer_num >= config.fusion_layer
        if self.has_cross_attention:
            self.layer_num = layer_num
            self.crossattention = RobertaAttention(config, is_cross_attention=True)
        self.intermediate = RobertaIntermediate(config)
        self.output = RobertaSelfOutput(config, fin=config.intermediate_size)

    def linear_slots(self, prefix):
        a = self.attention
        s = {"qkv": LinearSlot(prefix + "qkv", [a.self.query.weight, a.self.key.weight, a.self.value.weight],
                               [a.self.query.bias, a.self.key.bias, a.self.value.bias]),
             "o": LinearSlot(prefix + "o", [a.output.dense.weight], [a.output.dense.bias]),
             "i": LinearSlot(prefix + "i", [self.intermediate.dense.weight], [self.intermediate.dense.bias]),
             "out": LinearSlot(prefix + "out", [self.output.dense.weight], [self.output.dense.bias])}
        if self.has_cross_attention:
            c = self.crossattention
            s["q2"] = LinearSlot(prefix + "q2", [c.self.query.weight], [c.self.query.bias])
            s["kv2"] = LinearSlot(prefix + "kv2", [c.self.key.weight, c.self.value.weight], [c.self.key.bias, c.self.value.bias])
            s["o2"] = LinearSlot(prefix + "o2", [c.output.dense.weight], [c.output.dense.bias])
        self._s = s
        self._rlp = None  # (cached native-call pointers belong to the previous arena)
        return list(s.values())


class RobertaEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.layer = nn.ModuleList([RobertaLayer(config, i) for i in range(config.num_hidden_layers)])


class RobertaModel(nn.Module):
    embeddings_class = RobertaEmbeddings

    def __init__(self, config, add_pooling_layer=False):
        super().__init__()
        if add_pooling_layer:
            raise NotImplementedError("pooler is never built on the XFM path (xroberta.py:1167)")
        if config.hidden_size // config.num_attention_heads != 64:
            raise NotImplementedError("head_dim must be 64")
        self.config = config
        self.embeddings = self.embeddings_class(config)
        self.encoder = RobertaEncoder(config)
        self.pooler = None
        self._arena = None

    def linear_slots(self, prefix=""):
        out = []
        for i, layer in enumerate(self.encoder.layer):
            out.extend(layer.linear_slots(f"{prefix}layer.{i}."))
        return out

    def prefetch_cross_kv(self, encoder_hidden_states):
        """Queue the K|V projections of the image states for every cross-attention layer NOW, on the second stream (extension; the next
        forward with these very states picks them up).  In the pre-training step the launch stream idles ~0.5 ms between the ViT's last
        kernel and the fusion tower's first one -- the ITC logits, the draw of the negatives, their read-back and the host building the
        packed layout -- and the 12 projections (64 x 197 rows, 0.4 ms of GEMM) depend on none of that."""
        enc = encoder_hidden_states
        if not (_KV_AHEAD and enc.is_cuda and enc.dtype == BF16 and enc.is_contiguous() and self._arena is not None):
            return
        enc = enc.reshape(-1, enc.shape[-1])
        layers = [layer for layer in self.encoder.layer if layer.has_cross_attention]
        if not layers:
            return
        arena = layers[0]._s["kv2"]._arena
        for layer in layers:   # bf16 operand copies up to date and visible on this stream
            layer._s["kv2"]._ensure()
        pre = _WgradStream(enc.device)
        # (the entry holds `enc`: its memory cannot be handed to another tensor while the projections wait to be picked up)
        self._kv_ahead = ((enc.data_ptr(), tuple(enc.shape), enc._version), {id(layer): pre.project(enc, layer._s["kv2"]) for layer in layers}, enc)

    def attach(self, arena):
        self._arena = arena

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, head_mask=None,
                inputs_embeds=None, encoder_embeds=None, encoder_hidden_states=None, encoder_attention_mask=None,
                past_key_values=None, use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                is_decoder=False, mode='multi_modal', encoder_batch_index=None, grad_batch=None, pack=None, encoder_row_ranges=None,
                output_rows=None, cache_capacity=None):
        """`encoder_batch_index` (extension, default None = reference behaviour): int tensor [B] mapping every text row to the
        row of `encoder_hidden_states` it attends to, so duplicated images are projected to K/V once per layer.
        `grad_batch` (extension): only the first grad_batch sequences of the batch propagate gradient through the layer stack
        (a detached pass batched behind a differentiable one, e.g. the masked-text pass of get_fuse_mlm_loss).
        `pack` (extension, xfm_amd.packing.Pack): run on unpadded token rows -- `attention_mask` is then implied by the pack's lengths,
        `encoder_embeds` is a 2-D [pack.cap, D] row buffer and `last_hidden_state` comes back in the same packed layout.
        `encoder_row_ranges` (extension, with `pack`): (start int32 [U], count int32 [U], max count) -- the packed sequences are laid
        out image by image, so the queries of image u are the contiguous rows start[u] .. + count[u]: cross-attention then runs as one
        ragged problem per image on full 16-row query tiles instead of per-sequence tiles that are mostly padding.
        `output_rows` (extension, with `pack`): (rows int32 [S], start int32 [B], len int32 [B], max len) -- the caller reads only these
        token rows of the last layer (sequence b's are the block start[b] .. + len[b] of the S-row result): the last layer then runs
        its queries / FFN / LayerNorms on them alone (_LastLayerRowsFn) and `last_hidden_state` is the [S, D] result.
        `use_cache` / `past_key_values` (the causal decoder in eval mode under torch.no_grad(); xfm_amd.decode): the prompt, then one token
        per call, against a `decode.KVCache` returned as `.past_key_values`; a plain tuple of `[B, H, len, 64]` tensors is accepted and
        copied (the slow path).  `cache_capacity` (extension): tokens per row a fresh cache holds, default the position-table size."""
        if any(v is not None for v in (token_type_ids, position_ids, head_mask, inputs_embeds)):
            raise NotImplementedError("token_type_ids/position_ids/head_mask/inputs_embeds are not used on the XFM path")
        if use_cache or past_key_values is not None:
            if any(v is not None for v in (encoder_embeds, grad_batch, pack, encoder_row_ranges, output_rows)):
                raise NotImplementedError("use_cache / past_key_values take input_ids only (no encoder_embeds, grad_batch, pack, row ranges)")
            return cached_forward(self, input_ids, attention_mask=attention_mask, past_key_values=past_key_values,
                                  encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=encoder_attention_mask,
                                  is_decoder=is_decoder, mode=mode, encoder_batch_index=encoder_batch_index, cache_capacity=cache_capacity)
        if isinstance(encoder_hidden_states, (list, tuple)):
            raise NotImplementedError("per-layer encoder_hidden_states lists (xroberta.py:435-444) are outside the hot-path scope")
        if self._arena is None:
            raise RuntimeError("RobertaModel is not attached to a parameter arena; build it through XFMBase or call finalize()")
        cfg = self.config
        f32 = _F32_STREAM   # read at every call: an assignment to the switch takes effect at the next forward, in the moved passes too
        if pack is not None and is_decoder:
            raise NotImplementedError("packed rows are for the bidirectional towers")
        if encoder_embeds is None:
            if input_ids is None:
                raise ValueError("You have to specify either input_ids or inputs_embeds")
            B, T = input_ids.shape
            drop = Fx.drop_params(cfg.hidden_dropout_prob if self.training else 0.0, _next_seed())
            x, x32 = _EmbedFn.apply(self.embeddings.word_embeddings.weight, self.embeddings, input_ids, drop, self, pack, f32)
        else:
            if pack is not None:
                assert encoder_embeds.dim() == 2 and encoder_embeds.shape[0] == pack.cap, "packed encoder_embeds are [pack.cap, D] rows"
                B, T = pack.B, pack.T
            else:
                B, T = encoder_embeds.shape[:2]
            x32 = twin_of(encoder_embeds)   # the producing tower's fp32 twin, if this is its output (or a row-wise image of it: with_twin)
            if encoder_embeds.dtype == BF16:
                x = encoder_embeds
            else:   # fp32 states from outside: they ARE the un-rounded stream
                x, x32 = encoder_embeds.to(BF16), (encoder_embeds if encoder_embeds.dtype == F32 and f32 else None)
        if pack is not None:
            assert (B, T) == (pack.B, pack.T)
            attention_mask = None  # implied by the lengths: keys past a sequence's end do not exist
        dev = x.device
        key_keep = None if attention_mask is None else attention_mask.to(device=dev, dtype=torch.int32).contiguous()
        enc, enc_keep, Nenc = None, None, 0
        if encoder_hidden_states is not None:
            enc = encoder_hidden_states if encoder_hidden_states.dtype == BF16 else encoder_hidden_states.to(BF16)
            Nenc = enc.shape[1]
            enc = enc.reshape(-1, enc.shape[-1])
            if encoder_attention_mask is not None and not getattr(encoder_attention_mask, "_xfm_all_ones", False):
                enc_keep = encoder_attention_mask.to(device=dev, dtype=torch.int32).contiguous()
            if encoder_batch_index is not None:
                encoder_batch_index = encoder_batch_index.to(device=dev, dtype=torch.int32).contiguous()
                assert encoder_batch_index.numel() == B
        if mode == 'text':
            lo, hi = 0, cfg.fusion_layer
        elif mode == 'fusion':
            lo, hi = cfg.fusion_layer, cfg.num_hidden_layers
        elif mode == 'multi_modal':
            lo, hi = 0, cfg.num_hidden_layers
        else:
            raise ValueError(f"mode {mode} is not supported")
        y = x.reshape(B * T, -1) if pack is None else x
        y32 = None if x32 is None else (x32.reshape(B * T, -1) if pack is None else x32)
        if hi > lo:
            # one native call per layer whenever cross-attention (if any) can take the grouped kernels; else kernel by kernel
            xq = None
            if encoder_row_ranges is not None and enc is not None:
                assert pack is not None and Nenc <= 256, "per-image row ranges need packed rows and <= 256 image tokens"
                xq = (encoder_row_ranges[0].to(device=dev, dtype=torch.int32).contiguous(),
                      encoder_row_ranges[1].to(device=dev, dtype=torch.int32).contiguous(), int(encoder_row_ranges[2]))
            native = _NATIVE_LAYERS and y.is_cuda and (enc is None or xq is not None or
                                                       (encoder_batch_index is not None and Fx.attn_grouped_ok(T, Nenc)))
            saving = enc is not None and any(layer_saves_maps(self.encoder.layer[li]) for li in range(lo, hi))
            fn = _EncoderFn if saving else (_EncoderFnNative if native else _EncoderFn)   # (a layer that saves its maps runs kernel by kernel)
            if output_rows is not None:
                assert pack is not None and xq is None and grad_batch is None and not is_decoder and key_keep is None
                assert enc is None or (encoder_batch_index is not None and Fx.attn_grouped_ok(int(output_rows[3]), Nenc))
                if saving and layer_saves_maps(self.encoder.layer[hi - 1]):
                    # the last layer saves its maps, so it runs all its query rows: the rows somebody reads are gathered from its output
                    from .packing import rows_gather
                    y, y32 = fn.apply(y, y32, enc, self, key_keep, enc_keep, lo, hi, bool(is_decoder), B, T, Nenc, self.training,
                                      encoder_batch_index, grad_batch, pack, xq, f32)
                    rows = output_rows[0].to(torch.int32).contiguous()
                    y, y32 = rows_gather(y, rows), (None if y32 is None else rows_gather(y32, rows))
                    return SimpleNamespace(last_hidden_state=with_twin(y, y32), pooler_output=None, past_key_values=None,
                                           hidden_states=None, attentions=None, cross_attentions=None)
                hi -= 1
            if hi > lo:
                y, y32 = fn.apply(y, y32, enc, self, key_keep, enc_keep, lo, hi, bool(is_decoder), B, T, Nenc, self.training,
                                  encoder_batch_index if enc is not None else None, grad_batch, pack, xq, f32)
            if output_rows is not None:
                rows, sel_start, sel_len, tq = output_rows
                y, y32 = _LastLayerRowsFn.apply(y, y32, enc, self, hi, B, T, Nenc, self.training,
                                                encoder_batch_index if enc is not None else None,
                                                pack, rows.to(torch.int32).contiguous(),
                                                (sel_start.to(torch.int32).contiguous(), sel_len.to(torch.int32).contiguous()), int(tq), f32)
        if pack is None:
            y, y32 = y.view(B, T, -1), (None if y32 is None else y32.view(B, T, -1))
        return SimpleNamespace(last_hidden_state=with_twin(y, y32), pooler_output=None, past_key_values=None,
                               hidden_states=None, attentions=None, cross_attentions=None)


class RobertaLMHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        std = config.initializer_range
        self.dense = _Lin(config.hidden_size, config.hidden_size, std)
        self.layer_norm = _Affine(config.hidden_size, config.layer_norm_eps)
        self.decoder = _Lin(config.hidden_size, config.vocab_size, std)
        self.bias = nn.Parameter(torch.zeros(config.vocab_size))
        self.decoder.bias = self.bias  # tied, xroberta.py:1322-1323

    def linear_slots(self, prefix):
        self._slot_dense = LinearSlot(prefix + "dense", [self.dense.weight], [self.dense.bias])
        self._slot_decoder = LinearSlot(prefix + "decoder", [self.decoder.weight], [self.bias], pad_k_to=64)
        return [self._slot_dense, self._slot_decoder]


class RobertaForMaskedLM(OwnsArena, nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.roberta = RobertaModel(config, add_pooling_layer=False)
        self.lm_head = RobertaLMHead(config)
        self.lm_cap_head = RobertaLMHead(config)
        self._arena = None

    def linear_slots(self, prefix=""):
        return self.roberta.linear_slots(prefix + "roberta.") + self.lm_head.linear_slots(prefix + "lm_head.") + \
            self.lm_cap_head.linear_slots(prefix + "lm_cap_head.")

    def attach(self, arena):
        self._arena = arena
        self.roberta.attach(arena)

    def finalize(self, device=None):
        device = device or self.lm_head.bias.device
        self.attach(ParamArena(self, self.linear_slots(), device))
        self._own_arena = True
        return self

    def bert(self, input_ids=None, **kw):  # accepts the reference's keywords plus `encoder_batch_index`
        return self.roberta(input_ids, **kw)

    def gather_seq_out_by_pos(self, seq, pos):
        return torch.gather(seq, 1, pos.unsqueeze(2).expand(-1, -1, seq.size(-1)))

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, head_mask=None,
                inputs_embeds=None, encoder_embeds=None, encoder_hidden_states=None, encoder_attention_mask=None,
                labels=None, output_attentions=None, output_hidden_states=None, return_dict=None, is_decoder=False,
                reduction='mean', mode='multi_modal', return_logits=False, masked_pos=None):
        outputs = self.roberta(input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids,
                               position_ids=position_ids, head_mask=head_mask, inputs_embeds=inputs_embeds,
                               encoder_embeds=encoder_embeds, encoder_hidden_states=encoder_hidden_states,
                               encoder_attention_mask=encoder_attention_mask, is_decoder=is_decoder, mode=mode)
        seq = outputs.last_hidden_state
        if masked_pos is not None:
            seq = self.gather_seq_out_by_pos(seq, masked_pos)
        head = self.lm_cap_head if is_decoder else self.lm_head
        V = self.config.vocab_size
        if return_logits or labels is None:
            logits = lm_head_logits(seq.reshape(-1, seq.shape[-1]), head).view(*seq.shape[:2], V)
            if return_logits:
                return logits
            return SimpleNamespace(loss=None, logits=logits, hidden_states=None, attentions=None)
        if is_decoder:
            seq, labels = seq[:, :-1, :], labels[:, 1:]
        Bq, Tq = seq.shape[:2]
        loss, logits = lm_head_ce(seq.reshape(-1, seq.shape[-1]), head, labels.reshape(-1), reduction)
        return SimpleNamespace(loss=loss, logits=logits[:, :V].view(Bq, Tq, V), hidden_states=None, attentions=None)


class RobertaForCausalLM(GenerationMixin, OwnsArena, nn.Module):
    """Causal decoder with cross-attention to encoder states (the VQA answer decoder): mirrors models/xroberta.py:963-1153 --
    `roberta` + `lm_head`, causal self-attention mask, next-token shift, `reduction='none'` CE summed per sequence
    (:1107-1114).  `label_smoothing` is the keyword model_generation.py:275 passes to this class; the reference's own class does not
    take it (only its BERT sibling does, xbert.py:1240), so that call raises there.  Here it has the sibling's meaning
    (LabelSmoothSoftmaxCEV1, xbert.py:1190-1229: 1 - s at the label, s / V elsewhere); 0 is the plain CE, kernel for kernel.
    Generation (xfm_amd.decode): `use_cache` / `past_key_values`, `prepare_inputs_for_generation` and `_reorder_cache` are the reference's
    (xroberta.py:1130-1153).  `_generate_no_beam_search` exists in the reference only on the BERT sibling (xbert.py:1393-1484), yet
    model_generation.py:353 calls it on this class -- an AttributeError there; here the class has the sibling's method, as with
    `label_smoothing`.  Beam search and HF's generate() are not built."""

    def __init__(self, config, label_smoothing=0.0):
        super().__init__()
        self.config = config
        self.roberta = RobertaModel(config, add_pooling_layer=False)
        self.lm_head = RobertaLMHead(config)
        self.label_smoothing = label_smoothing
        self._arena = None

    def linear_slots(self, prefix=""):
        return self.roberta.linear_slots(prefix + "roberta.") + self.lm_head.linear_slots(prefix + "lm_head.")

    def attach(self, arena):
        self._arena = arena
        self.roberta.attach(arena)

    def finalize(self, device=None):
        device = device or self.lm_head.bias.device
        self.attach(ParamArena(self, self.linear_slots(), device))
        self._own_arena = True
        return self

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, head_mask=None,
                inputs_embeds=None, encoder_hidden_states=None, encoder_attention_mask=None, labels=None, past_key_values=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, is_decoder=True,
                reduction='mean', mode='multi_modal', return_logits=False, encoder_batch_index=None, cache_capacity=None):
        # `encoder_batch_index` (extension, default None = the reference's call): row b cross-attends to encoder_hidden_states[index[b]], so
        # rows that share a source (rank_answer's k candidates per question) have its K/V projected once per layer (RobertaModel.forward)
        outputs = self.roberta(input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, position_ids=position_ids,
                               head_mask=head_mask, inputs_embeds=inputs_embeds, encoder_hidden_states=encoder_hidden_states,
                               encoder_attention_mask=encoder_attention_mask, is_decoder=is_decoder, mode=mode, encoder_batch_index=encoder_batch_index,
                               past_key_values=past_key_values, use_cache=use_cache, cache_capacity=cache_capacity)
        seq = outputs.last_hidden_state
        V = self.config.vocab_size
        B, T = seq.shape[:2]
        if return_logits or labels is None:
            logits = lm_head_logits(seq.reshape(-1, seq.shape[-1]), self.lm_head).view(B, T, V)
            if return_logits:
                return logits[:, :-1, :].contiguous()
            return SimpleNamespace(loss=None, logits=logits, hidden_states=seq, past_key_values=outputs.past_key_values, attentions=None,
                                   cross_attentions=None)
        shifted, lab = seq[:, :-1, :], labels[:, 1:]
        loss, logits = lm_head_ce(shifted.reshape(-1, seq.shape[-1]), self.lm_head, lab.reshape(-1), reduction, self.label_smoothing)
        if reduction == 'none':
            loss = loss.view(B, -1).sum(1)
        return SimpleNamespace(loss=loss, logits=logits[:, :V].view(B, T - 1, V), hidden_states=seq, past_key_values=outputs.past_key_values,
                               attentions=None, cross_attentions=None)

    def _generation_parts(self):
        return self.roberta, self.lm_head
