"""Host side of cached decoding / generation without a GPU: the ABI of the two decoding kernels and their argument checks, the CPU-tensor
refusals, prepare_inputs_for_generation, and the generation fixtures (tests/golden/generation_*_2L.npz, from the reference's own cached
forward and _generate_no_beam_search; tools/oracle/gen_generation.py) pinned by the fp32 oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

from decode_util import decisive, finishing_invariants, generate_ref, next_token_ref
from golden_util import check, load
from oracle import xfm_oracle as O
from test_oracle_golden import ATOL, RTOL, _params
from xfm_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("roberta", "bert")


def test_abi_and_new_symbols():
    from xfm_amd import _lib
    assert _lib.ABI_VERSION >= 17
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "xfm_hip.h")) as f:
        hdr = f.read()
    for sym in ("xfm_decode_attn", "xfm_next_token"):
        assert sym in _lib.SIGNATURES and getattr(lib, sym) is not None and f"int {sym}(" in hdr
    assert "xbert.py:1422-1462" in hdr and "xroberta.py:224-234" in hdr
    with open(os.path.join(ROOT, "xfm_amd", "csrc", "capi.hip")) as f:
        assert f.read().count('#include "decode.hip"') == 1


def _attn_args(**kw):
    from xfm_amd._lib import DecodeAttnArgs
    P = 0x10000   # non-NULL, 16-byte aligned, never read: every case below is refused before anything is launched
    a = dict(q=P, q_rs=2304, k_new=P, k_new_rs=2304, v_new=P, v_new_rs=2304, k_cache=P, v_cache=P, rs=1536, o=P, o_rs=768, n_src=2,
             B=2, H=12, cap=8, pos=3, Sk=4, scale=0.125)
    a.update(kw)
    return DecodeAttnArgs(**a)


@pytest.mark.parametrize("bad,word", [(dict(pos=8, Sk=9), b"capacity"), (dict(pos=7, Sk=9), b"keys"), (dict(rs=760), b"row stride"),
                                      (dict(k_new=0, v_new=0, Sk=0), b"Sk"), (dict(k_new=0, v_new=0, Sk=9), b"capacity"),
                                      (dict(k_new=0, v_new=0, rs=767), b"row stride"), (dict(q=0x10002), b"16 bytes"),
                                      (dict(k_new=0x10000, v_new=0), b"v_new")])
def test_decode_attn_refuses_bad_arguments(bad, word):
    """pos + 1 > cap, Sk < 1, Sk > cap, H * 64 > rs: an error code and no launch (an out-of-range append would be a GPU fault)."""
    from xfm_amd import _lib
    lib = _lib.load()
    a = _attn_args(**bad)
    assert lib.xfm_decode_attn(ctypes.byref(a), None) == -1
    msg = lib.xfm_last_error()
    assert b"decode_attn" in msg and word in msg, msg
    assert lib.xfm_decode_attn(None, None) == -1


@pytest.mark.parametrize("bad,word", [(dict(cur_len=9), b"cur_len"), (dict(cur_len=-1), b"cur_len"), (dict(step=4), b"step"),
                                      (dict(V=65), b"V="), (dict(V=131073, ld=131080), b"exceeds"), (dict(n_eos=9), b"eos"),
                                      (dict(penalty=0.0), b"penalty"), (dict(logits=0), b"null")])
def test_next_token_refuses_bad_arguments(bad, word):
    from xfm_amd import _lib
    lib = _lib.load()
    P = 0x10000
    kw = dict(logits=P, ld=64, V=50, ids=P, ids_ld=9, cur_len=3, penalty=1.0, unfinished=P, hist_unfinished=P, hist_logprob=P, hist_ld=4,
              step=1, pad_id=1, n_eos=1, B=2)
    kw.update(bad)
    a = _lib.NextTokenArgs(**kw)
    assert lib.xfm_next_token(ctypes.byref(a), None) == -1
    msg = lib.xfm_last_error()
    assert b"next_token" in msg and word in msg, msg


def test_cpu_tensors_raise():
    from xfm_amd import _lib
    from xfm_amd import functional as Fx
    bf = torch.bfloat16
    with pytest.raises(_lib.XfmHipError):
        Fx.decode_attn(torch.zeros(2, 64, dtype=bf), torch.zeros(8, 64, dtype=bf), torch.zeros(8, 64, dtype=bf), 4, 1, 0.125, Sk=4)
    with pytest.raises(_lib.XfmHipError):
        Fx.next_token(torch.zeros(2, 8), 8, torch.zeros(2, 4, dtype=torch.int64), 1, torch.ones(2, dtype=torch.int32),
                      torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3), 0, 1, [2])


def _tiny(kind):
    if kind == "roberta":
        from xfm_amd.xroberta import RobertaConfig, RobertaForCausalLM
        return RobertaForCausalLM(RobertaConfig(vocab_size=97, hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128,
                                                fusion_layer=0, encoder_width=64))
    from xfm_amd.xbert import BertConfig, BertLMHeadModel
    return BertLMHeadModel(BertConfig(vocab_size=97, hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=128,
                                      fusion_layer=0, encoder_width=64))


@pytest.mark.parametrize("kind", KINDS)
def test_generation_surface_on_the_host(kind):
    """prepare_inputs_for_generation cuts to the last id when a past is given; _reorder_cache on a plain tuple is the reference's; a cache
    outside eval / no_grad is refused with a clear error (before any kernel)."""
    m = _tiny(kind)
    ids = torch.arange(12).view(2, 6)
    enc = torch.zeros(2, 3, 64)
    got = m.prepare_inputs_for_generation(ids, encoder_hidden_states=enc)
    assert torch.equal(got["input_ids"], ids) and torch.equal(got["attention_mask"], torch.ones_like(ids)) and got["past_key_values"] is None
    assert got["encoder_hidden_states"] is enc and got["is_decoder"] is True
    past = ((torch.zeros(2, 1, 5, 64), torch.ones(2, 1, 5, 64)),)
    got = m.prepare_inputs_for_generation(ids, past=past)
    assert got["input_ids"].tolist() == [[5], [11]] and got["attention_mask"].shape == (2, 6) and got["past_key_values"] is past
    k = torch.arange(3.0).view(3, 1, 1, 1).expand(3, 1, 5, 64)
    re = m._reorder_cache(((k, k + 10),), torch.tensor([2, 0, 0]))
    assert re[0][0][:, 0, 0, 0].tolist() == [2, 0, 0] and re[0][1][:, 0, 0, 0].tolist() == [12, 10, 10]
    for name in ("prepare_inputs_for_generation", "_reorder_cache", "_generate_no_beam_search"):
        assert callable(getattr(m, name))
    with pytest.raises(RuntimeError, match="arena|inference-only"):
        m(ids, use_cache=True)


def test_next_token_restatement_follows_the_reference_rules():
    """decode_util.next_token_ref against a hand-worked row: penalty once per distinct id, lowest index among equal maxima, pad for a
    finished row, eos clears the flag."""
    x = torch.tensor([[1.0, 4.0, 4.0, -2.0], [0.5, 0.25, 3.0, -1.0], [9.0, 0.0, 0.0, 0.0]])
    ids = torch.tensor([[3, 3, 0], [2, 2, 2], [1, 1, 1]])
    r = next_token_ref(x, 4, ids, 3, 2.0, torch.tensor([1, 1, 0]), 7, [1])
    assert r["tok"].tolist() == [1, 2, 0] and r["add"].tolist() == [1, 2, 7] and r["unfinished"].tolist() == [0, 1, 0] and r["count"] == 1
    want = torch.log_softmax(torch.tensor([0.5, 4.0, 4.0, -4.0], dtype=torch.float64), 0)[1]
    assert abs(float(r["lp"][0]) - float(want)) < 1e-12
    want = torch.log_softmax(torch.tensor([0.5, 0.25, 1.5, -1.0], dtype=torch.float64), 0)[2]   # id 2 three times: divided ONCE
    assert abs(float(r["lp"][1]) - float(want)) < 1e-12


def _oracle_logits(kind, P, ids, enc, enc_atts):
    att = torch.ones_like(ids)
    if kind == "roberta":
        return O.causal_lm_logits(P, ids, att, enc, enc_atts, 2)[:, -1, :]
    seq = O.bert_model(P, "bert.", ids, att, enc, enc_atts, num_layers=2, fusion_layer=0, causal=True)
    return O.bert_lm_head(P, "cls.predictions.", seq[:, -1:, :])[:, 0, :]


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_is_pinned_by_the_oracle(kind):
    """A greedy loop over the oracle's causal decoder (uncached, fp32), teacher-forced on the fixture's tokens, reproduces the fixture's
    logit probes at the oracle tests' tolerance and its token at every decisive step; the restated generation loop driven by the same
    oracle reproduces the reference's _generate_no_beam_search outputs."""
    z, meta = load(f"generation_{kind}_2L")
    B, S, NEW = meta["B"], meta["S"], meta["new_tokens"]
    P = _params(meta["spec"], requires_grad=False)
    enc = syn.gaussian("gen.image_states", (B, S, 768), 0.7)
    enc_atts = torch.tensor(meta["enc_atts"])
    prompt = torch.tensor(meta["prompt"])
    dec = decisive(z)
    assert 2 * int(dec.sum()) >= dec.numel() and int(dec.sum()) == meta["decisive"]
    assert z["past_shapes"].shape == (2, 2, 4) and z["past_shapes"][0, 0].tolist() == [B, 12, len(meta["prompt"][0]) + NEW - 1, 64]   # (the last token is never fed)
    tokens = torch.from_numpy(z["tokens"])
    ids = prompt.clone()
    with torch.no_grad():
        for t in range(NEW):
            logits = _oracle_logits(kind, P, ids, enc, enc_atts)
            check(z, f"step{t}/logits", logits, ATOL, RTOL, what=f"{kind} ")
            top = logits.argmax(-1)
            for b in range(B):
                if dec[t, b]:
                    assert int(top[b]) == int(tokens[t, b]), (kind, t, b)
                else:
                    assert int(top[b]) in z["top_ids"][t, b, :2].tolist(), (kind, t, b)
            ids = torch.cat([ids, tokens[t].view(B, 1)], dim=1)
        assert int(tokens[4, 0]) == meta["eos"]
        for p in meta["penalties"]:
            want_ids, want_lp = torch.from_numpy(z[f"gen_ids_{p}"]), torch.from_numpy(z[f"gen_logprobs_{p}"])
            finishing_invariants(want_ids, prompt.shape[1], meta["pad"], [meta["eos"]])
            assert want_ids.shape == (B, meta["max_length"]) and want_ids[0].tolist().count(meta["pad"]) >= 1
            got_ids, got_lp = generate_ref(lambda cur: _oracle_logits(kind, P, cur, enc, enc_atts), prompt, prompt.shape[1], meta["max_length"],
                                           p, meta["pad"], [meta["eos"]], B)
            assert torch.equal(got_ids, want_ids), (kind, p, got_ids, want_ids)
            assert np.allclose(got_lp.numpy(), want_lp.numpy(), rtol=1e-5, atol=1e-4)
