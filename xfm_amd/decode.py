"""Cached incremental decoding and greedy / sampled generation for the causal decoders (shared by xroberta.py and xbert.py).

What the reference does with `use_cache` / `past_key_values` (models/xroberta.py:224-262, models/xbert.py:1368-1484) on the HIP path:
  * `KVCache`: the `past_key_values` object.  A tuple of per-layer `(k, v)` in the reference's `[B, H, len, 64]` shape -- views of
    token-major bf16 buffers `[B, cap, 2 D]` (K | V side by side, the layout of the fused QKV projection), so appending a token is one row
    write inside the attention kernel.  It also holds the K | V projections of the encoder states of every cross-attention layer, which
    the reference recomputes at every step (xroberta.py:224-226), keyed by the identity of those states.
  * `cached_forward`: RobertaModel / BertModel.forward with a cache.  Without a past the prompt runs through the causal kernels of the
    ordinary forward (the shared layer body, `roberta_layer.forward_tail`, in inference form) and its K / V rows are kept; with a past, ONE new token per
    row runs through `Fx.decode_attn` in place of the two `Fx.attn_fwd` calls.
  * `GenerationMixin`: `prepare_inputs_for_generation`, `_reorder_cache`, `_generate_no_beam_search` with the reference's signatures;
    one `Fx.next_token` launch per step does the penalty, the choice, the score and the finished-row bookkeeping on the device.
    With `do_sample` and `fused_sampling=True` that launch is `Fx.sample_token`, which also filters (top-k / top-p) and draws on the device.
Inference only: eval mode under torch.no_grad().  Beam search and HF's generate() are not built."""
import math
from types import SimpleNamespace

import torch

from . import functional as Fx
from .roberta_layer import NO_DROPS, forward_tail

BF16, F32 = torch.bfloat16, torch.float32


def _enc_identity(enc):
    return (enc.data_ptr(), tuple(enc.shape), enc._version, enc.dtype)


class KVCache(tuple):
    """`past_key_values` of the cached decoders.  len(cache) = number of layers; cache[i] = (k, v), each `[B, H, len, 64]` bf16 (views).
    Attributes: `self_kv` (per layer, bf16 [B, capacity, 2 D]: keys in columns [0, D), values in [D, 2 D)), `length` (tokens cached),
    `capacity` (rows per entry), `cross_kv` ({layer index: bf16 [sources * keys, 2 D]}), `cross_keys`, `cross_id` (identity of the
    encoder states the cross K / V were projected from: data_ptr, shape, _version, dtype).
    A step appends IN PLACE: the cache it returns shares its buffers with the one it was given, which must not be extended a second
    time with another token while the first continuation is still in use (`_reorder_cache` copies)."""

    def __new__(cls, self_kv, length, cross_kv=None, cross_keys=0, cross_id=None):
        B, cap, D2 = self_kv[0].shape
        H = D2 // 128
        items = []
        for buf in self_kv:
            k = buf[:, :length, :D2 // 2].unflatten(-1, (H, 64)).permute(0, 2, 1, 3)
            v = buf[:, :length, D2 // 2:].unflatten(-1, (H, 64)).permute(0, 2, 1, 3)
            items.append((k, v))
        self = super().__new__(cls, items)
        self.self_kv, self.length, self.capacity = list(self_kv), length, cap
        self.cross_kv, self.cross_keys, self.cross_id = cross_kv or {}, cross_keys, cross_id
        return self

    @classmethod
    def empty(cls, n_layers, B, cap, D, device):
        return cls([torch.zeros((B, cap, 2 * D), dtype=BF16, device=device) for _ in range(n_layers)], 0)

    @classmethod
    def from_tuple(cls, past, cap, device):
        """The slow path: a plain tuple of (k, v) `[B, H, len, 64]` tensors of any float dtype, copied into fresh bf16 buffers."""
        B, H, L, hd = past[0][0].shape
        if hd != 64:
            raise ValueError("past_key_values: head_dim must be 64")
        if L > cap:
            raise ValueError(f"past_key_values hold {L} tokens, the cache capacity is {cap}")
        c = cls.empty(len(past), B, cap, H * 64, device)
        for buf, (k, v) in zip(c.self_kv, past):
            buf[:, :L, :H * 64] = k.to(device=device).permute(0, 2, 1, 3).reshape(B, L, H * 64).to(BF16)
            buf[:, :L, H * 64:] = v.to(device=device).permute(0, 2, 1, 3).reshape(B, L, H * 64).to(BF16)
        return cls(c.self_kv, L)

    def grown(self, length):
        return KVCache(self.self_kv, length, self.cross_kv, self.cross_keys, self.cross_id)

    def reordered(self, beam_idx):
        """Rows beam_idx of the self caches, copied (xbert.py:1387-1391).  The cross K / V stay as they are: they belong to the encoder
        states (row i, or encoder_batch_index[i], of what the next forward is given), which the reference does not reorder either."""
        idx = beam_idx.to(device=self.self_kv[0].device, dtype=torch.int64)
        return KVCache([buf.index_select(0, idx) for buf in self.self_kv], self.length, self.cross_kv, self.cross_keys, self.cross_id)


def _position_ids(model, input_ids, past_len):
    """xroberta.py:1747-1757 create_position_ids_from_input_ids(input_ids, pad, past_len) / xbert.py:205-206 position_ids[:, past:past + T]"""
    emb = model.embeddings
    B, T = input_ids.shape
    if getattr(emb, "pos_mode", 0):
        return torch.arange(past_len, past_len + T, device=input_ids.device).expand(B, T)
    mask = input_ids.ne(emb.padding_idx).long()
    return (torch.cumsum(mask, dim=1) + past_len) * mask + emb.padding_idx


def _embed_step(model, input_ids, past_len, f32):
    """Embedding + LayerNorm of the new tokens at their positions behind the past -> (y bf16 [B*T, D], fp32 twin or None)."""
    emb = model.embeddings
    pos = _position_ids(model, input_ids, past_len)
    x = emb.word_embeddings.weight[input_ids] + emb.token_type_embeddings.weight[0] + emb.position_embeddings.weight[pos]
    x = x.reshape(-1, x.shape[-1]).float().contiguous()
    ln = emb.LayerNorm
    out = Fx.ln_fwd(x, ln.weight, ln.bias, ln.eps, y32=f32)
    return out[0], (out[3] if f32 else None)


def _run_layers(model, x, xres, cache, B, T, key_keep, enc_keep, enc_index, f32):
    """The layer loop in inference form: roberta_layer.forward_tail with no dropout and nothing saved behind this path's own attentions.
    T == 1: both are Fx.decode_attn on the cache; T > 1 (the prompt, empty cache): Fx.attn_fwd, causal, and the K | V columns of the QKV
    projection are copied into the cache rows."""
    cfg = model.config
    D, H = cfg.hidden_size, cfg.num_attention_heads
    scale = 1.0 / math.sqrt(D // H)
    pos, cap, Nenc = cache.length, cache.capacity, cache.cross_keys
    for li, layer in enumerate(model.encoder.layer):
        s = layer._s
        buf = cache.self_kv[li]
        qkv = Fx.gemm_nt(x, s["qkv"].wb, s["qkv"].b)
        if T == 1:
            rows = buf.view(B * cap, 2 * D)
            c1 = Fx.decode_attn(qkv[:, :D], rows[:, :D], rows[:, D:], cap, H, scale, k_new=qkv[:, D:2 * D], v_new=qkv[:, 2 * D:], pos=pos,
                                key_keep=key_keep)
        else:
            c1, _ = Fx.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, T, T, scale, key_keep=key_keep, causal=True)
            buf[:, :T] = qkv[:, D:].view(B, T, 2 * D)
        cross = None
        if layer.has_cross_attention and li in cache.cross_kv:
            def cross(q2, kv=cache.cross_kv[li]):
                if T == 1:
                    return kv, Fx.decode_attn(q2, kv[:, :D], kv[:, D:], Nenc, H, scale, Sk=Nenc, key_keep=enc_keep, kv_index=enc_index), None, None
                return kv, Fx.attn_fwd(q2, kv[:, :D], kv[:, D:], B, H, T, Nenc, scale, key_keep=enc_keep, kv_index=enc_index)[0], None, None
        x, xres, _ = forward_tail(layer, c1, xres, NO_DROPS, f32, cross, save=False)
    return x, (xres if f32 else None)


def cached_forward(model, input_ids, attention_mask=None, past_key_values=None, encoder_hidden_states=None, encoder_attention_mask=None,
                   is_decoder=False, mode='multi_modal', encoder_batch_index=None, cache_capacity=None):
    """RobertaModel / BertModel.forward with `use_cache=True` or a past (see the module docstring).  `attention_mask` covers past and new
    tokens ([B, past + T]), as in the reference; None = all ones."""
    from .xroberta import _F32_STREAM, with_twin
    if not is_decoder:
        raise NotImplementedError("use_cache / past_key_values: only the causal decoder (is_decoder=True) keeps a cache")
    if mode != 'multi_modal':
        raise NotImplementedError("use_cache / past_key_values: only mode='multi_modal' (the whole layer stack) keeps a cache")
    if model.training or torch.is_grad_enabled():
        raise RuntimeError("use_cache / past_key_values are inference-only: call model.eval() and run under torch.no_grad()")
    if input_ids is None:
        raise ValueError("use_cache / past_key_values need input_ids")
    if isinstance(encoder_hidden_states, (list, tuple)):
        raise NotImplementedError("per-layer encoder_hidden_states lists (xroberta.py:435-444) are outside the hot-path scope")
    if model._arena is None:
        raise RuntimeError("the model is not attached to a parameter arena; build it through its task model or call finalize()")
    cfg = model.config
    f32 = _F32_STREAM
    dev = model.embeddings.word_embeddings.weight.device
    input_ids = input_ids.to(dev).contiguous()
    B, T = input_ids.shape
    D, L = cfg.hidden_size, cfg.num_hidden_layers
    cap = int(cache_capacity) if cache_capacity is not None else cfg.max_position_embeddings
    cache = past_key_values
    if cache is None:
        cache = KVCache.empty(L, B, cap, D, dev)
    elif not isinstance(cache, KVCache):
        cache = KVCache.from_tuple(cache, cap, dev)
    if len(cache) != L or cache.self_kv[0].shape[0] != B or cache.self_kv[0].shape[2] != 2 * D:
        raise ValueError("past_key_values do not fit this model / batch")
    pos = cache.length
    if pos > 0 and T != 1:
        raise NotImplementedError(f"with a past, one new token per row is decoded at a time (got {T})")
    if pos + T > cache.capacity:
        raise ValueError(f"the cache holds {cache.capacity} tokens per row; {pos} cached + {T} new do not fit (cache_capacity / max_length)")
    key_keep = None
    if attention_mask is not None and not getattr(attention_mask, "_xfm_all_ones", False):
        if tuple(attention_mask.shape) != (B, pos + T):
            raise ValueError(f"attention_mask must cover past and new tokens: [{B}, {pos + T}], got {tuple(attention_mask.shape)}")
        key_keep = attention_mask.to(device=dev, dtype=torch.int32).contiguous()
    # cross-attention K | V: projected once per set of encoder states, kept in the cache
    enc_keep = enc_index = None
    if encoder_hidden_states is not None:
        ident = _enc_identity(encoder_hidden_states)
        if cache.cross_id != ident:
            enc = encoder_hidden_states if encoder_hidden_states.dtype == BF16 else encoder_hidden_states.to(BF16)
            enc = enc.to(dev).reshape(-1, enc.shape[-1]).contiguous()
            cache.cross_kv = {li: Fx.gemm_nt(enc, layer._s["kv2"].wb, layer._s["kv2"].b)
                              for li, layer in enumerate(model.encoder.layer) if layer.has_cross_attention}
            cache.cross_keys, cache.cross_id = encoder_hidden_states.shape[1], ident
        if encoder_attention_mask is not None and not getattr(encoder_attention_mask, "_xfm_all_ones", False):
            enc_keep = encoder_attention_mask.to(device=dev, dtype=torch.int32).contiguous()
        if encoder_batch_index is not None:
            enc_index = encoder_batch_index.to(device=dev, dtype=torch.int32).contiguous()
            assert enc_index.numel() == B
        elif encoder_hidden_states.shape[0] != B:
            raise ValueError("encoder_hidden_states need one entry per row, or an encoder_batch_index")
    else:
        cache.cross_kv, cache.cross_keys, cache.cross_id = {}, 0, None
    if pos == 0:   # the embedding kernel of the ordinary forward
        emb, ln = model.embeddings, model.embeddings.LayerNorm
        out = Fx.embed_ln_fwd(input_ids, emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight,
                              ln.weight, ln.bias, ln.eps, emb.padding_idx, pos_mode=getattr(emb, "pos_mode", 0), y32=f32)
        x, x32 = out[0], (out[4] if f32 else None)
    else:
        x, x32 = _embed_step(model, input_ids, pos, f32)
    y, y32 = _run_layers(model, x, x32 if f32 else x, cache, B, T, key_keep, enc_keep, enc_index, f32)
    y, y32 = y.view(B, T, -1), (None if y32 is None else y32.view(B, T, -1))
    return SimpleNamespace(last_hidden_state=with_twin(y, y32), pooler_output=None, past_key_values=cache.grown(pos + T),
                           hidden_states=None, attentions=None, cross_attentions=None)


def head_logits(head, x, out=None):
    """ops.lm_head_logits for rows x [R, D], into an fp32 [R, ld >= V] buffer (columns past V are not written)."""
    sd, sv = head._slot_dense, head._slot_decoder
    hact, _ = Fx.gemm_nt(x.contiguous(), sd.wb, sd.b, epi=Fx.EPI_GELU)
    y, _, _ = Fx.ln_fwd(hact, head.layer_norm.weight, head.layer_norm.bias, head.layer_norm.eps)
    return Fx.gemm_nt(y, sv.wb, sv.b, epi=Fx.EPI_F32, out=out, n=sv.N)


def top_k_top_p_filtering(logits, top_k=0, top_p=1.0, filter_value=-float("inf"), min_tokens_to_keep=1):
    """xbert.py:1487-1519 with out-of-place torch ops on the device (no host read)."""
    if top_k > 0:
        top_k = min(max(top_k, min_tokens_to_keep), logits.size(-1))
        logits = logits.masked_fill(logits < torch.topk(logits, top_k)[0][..., -1, None], filter_value)
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(logits, descending=True)
        remove = torch.cumsum(torch.softmax(sorted_logits, dim=-1), dim=-1) > top_p
        if min_tokens_to_keep > 1:
            remove[..., :min_tokens_to_keep] = False
        remove[..., 1:] = remove[..., :-1].clone()
        remove[..., 0] = False
        logits = logits.masked_fill(remove.scatter(1, sorted_indices, remove), filter_value)
    return logits


def repetition_penalised(logits, ids, penalty):
    """xbert.py:1425-1432 as torch ops (the sampling path; the greedy path does it inside Fx.next_token)."""
    seen = torch.zeros(logits.shape, dtype=torch.bool, device=logits.device).scatter_(1, ids, True)
    return torch.where(seen, torch.where(logits < 0, logits * penalty, logits / penalty), logits)


SYNC_EVERY = 8
"""Default `sync_every` of _generate_no_beam_search: the host reads the unfinished-row counter every that many steps."""


class GenerationMixin:
    """The generation surface of the reference's causal LMs (xbert.py:1368-1484, xroberta.py:1130-1153).  The host class names its tower
    and head through `_generation_parts()`."""

    def prepare_inputs_for_generation(self, input_ids, past=None, attention_mask=None, **model_kwargs):
        if attention_mask is None:
            attention_mask = input_ids.new_ones(input_ids.shape)
        if past is not None:
            input_ids = input_ids[:, -1:]
        return {"input_ids": input_ids, "attention_mask": attention_mask, "past_key_values": past,
                "encoder_hidden_states": model_kwargs.get("encoder_hidden_states", None),
                "encoder_attention_mask": model_kwargs.get("encoder_attention_mask", None), "is_decoder": True}

    def _reorder_cache(self, past, beam_idx):
        if isinstance(past, KVCache):
            return past.reordered(beam_idx)
        return tuple(tuple(t.index_select(0, beam_idx) for t in layer_past) for layer_past in past)

    @torch.no_grad()
    def _generate_no_beam_search(self, input_ids, cur_len, max_length, do_sample, temperature, top_k, top_p, repetition_penalty,
                                 pad_token_id, eos_token_ids, batch_size, sync_every=SYNC_EVERY, fused_sampling=False, seed=None, uniforms=None,
                                 **model_kwargs):
        """xbert.py:1393-1484: greedy (or sampled) decoding without beams -> (input_ids [B, max_length] padded with pad_token_id, the mean
        log-probability of every row's own tokens).  model_kwargs: encoder_hidden_states, encoder_attention_mask, encoder_batch_index
        (extension), past.  Every step is the cached forward of one token and ONE Fx.next_token launch; the host reads nothing inside the
        loop but the unfinished-row counter, every `sync_every` steps (extension).  Where the reference breaks once every row has
        finished, running on changes nothing: finished rows only receive pads and their history entries are masked, so the result does
        not depend on sync_every.
        fused_sampling (extension, default off): with do_sample, the penalty, the temperature, top_k_top_p_filtering, the draw and the
        score of a step are ONE Fx.sample_token launch on the head's logits in place of the torch ops below.  The draws come from the
        library's counter generator keyed by `seed` (None: one 64-bit seed per call from torch's CPU generator, so torch.manual_seed
        makes a call reproducible), or from `uniforms` fp32 [B, steps] in [0, 1), column `step` at that step."""
        unknown = set(model_kwargs) - {"encoder_hidden_states", "encoder_attention_mask", "encoder_batch_index", "past"}
        if unknown:
            raise TypeError(f"_generate_no_beam_search: unsupported model keywords {sorted(unknown)} (the decoder attends to every id it is given)")
        tower, head = self._generation_parts()
        dev = head._slot_decoder.wb.device
        B, V = batch_size, self.config.vocab_size
        steps = max_length - cur_len
        ids = torch.full((B, max_length), pad_token_id, dtype=torch.int64, device=dev)
        ids[:, :cur_len] = input_ids[:, :cur_len]
        eos = [int(e) for e in eos_token_ids]
        if steps <= 0:
            return ids, torch.full((B,), float("nan"), device=dev)
        unfinished = torch.ones(B, dtype=torch.int32, device=dev)
        hist_u = torch.zeros((B, steps), dtype=torch.int32, device=dev)
        hist_lp = torch.zeros((B, steps), dtype=F32, device=dev)
        counts = torch.zeros(steps, dtype=torch.int32, device=dev)
        logits = torch.empty((B, (V + 63) // 64 * 64), dtype=F32, device=dev)
        past = model_kwargs.get("past", None)
        kw = {k: model_kwargs.get(k, None) for k in ("encoder_hidden_states", "encoder_attention_mask", "encoder_batch_index")}
        fused = bool(do_sample and fused_sampling)
        if fused:
            if uniforms is not None:
                assert uniforms.shape == (B, steps) and uniforms.dtype == F32, "uniforms: fp32 [batch_size, max_length - cur_len]"
                uniforms = uniforms.to(dev).t().contiguous()   # row `step` = that step's [B] draws
            elif seed is None:
                seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device="cpu"))
        step = 0
        while cur_len < max_length:
            inp = ids[:, :cur_len] if past is None else ids[:, cur_len - 1:cur_len]
            out = tower(inp, past_key_values=past, use_cache=True, is_decoder=True, cache_capacity=max_length, **kw)
            past = out.past_key_values
            head_logits(head, out.last_hidden_state[:, -1, :], out=logits)
            if fused:
                Fx.sample_token(logits, V, ids, cur_len, unfinished, hist_u, hist_lp, step, pad_token_id, eos, temperature, top_k, top_p,
                                0 if seed is None else seed, penalty=repetition_penalty, n_unfinished=counts[step:step + 1],
                                uniforms=None if uniforms is None else uniforms[step])
            elif do_sample:
                lg = logits[:, :V]
                if repetition_penalty != 1.0:
                    lg = repetition_penalised(lg, ids[:, :cur_len], repetition_penalty)
                if temperature != 1.0:
                    lg = lg / temperature
                lg = top_k_top_p_filtering(lg, top_k=top_k, top_p=top_p).contiguous()
                drawn = torch.multinomial(torch.softmax(lg, dim=-1), num_samples=1).squeeze(1)
                Fx.next_token(lg, V, ids, cur_len, unfinished, hist_u, hist_lp, step, pad_token_id, eos, next_token=drawn,
                              n_unfinished=counts[step:step + 1])
            else:
                Fx.next_token(logits, V, ids, cur_len, unfinished, hist_u, hist_lp, step, pad_token_id, eos, penalty=repetition_penalty,
                              n_unfinished=counts[step:step + 1])
            cur_len, step = cur_len + 1, step + 1
            if step % sync_every == 0 and cur_len < max_length and int(counts[step - 1]) == 0:
                break
        if cur_len == max_length:
            ids[:, -1].masked_fill_(unfinished.bool(), eos[0])
        u = hist_u.float()
        logprobs = torch.where(hist_u > 0, hist_lp, torch.zeros_like(hist_lp)).sum(dim=1) / u.sum(dim=1)
        return ids, logprobs
