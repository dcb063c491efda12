"""Generate tests/golden/generation_roberta_2L.npz and generation_bert_2L.npz from the REAL reference (behind ref_shim, as gen_golden.py does).

Run in the build container only:   python tools/oracle/gen_generation.py [--only roberta|bert]

The models are the reference's RobertaForCausalLM / BertLMHeadModel: 2 layers, cross-attention in both (fusion_layer = 0), formula
weights, eval mode.  B = 4 rows, encoder states syn.gaussian("gen.image_states", (4, 30, 768), 0.7) with row 1 masked past key 20, the
prompt is the first 3 ids of syn.pretrain_batch(4, seed=13) (BERT: vocab 30522, id 0 -> 5), 12 new tokens.  Nothing but probes and small
integer arrays is stored.

Stored per step t = 0 .. 11, from the reference's own CACHED forward (use_cache / past_key_values), teacher-forced on its own greedy tokens:
  step<t>/logits/*   strided probe + moments of the last-position logits [4, V];
  top_ids / top_vals [12, 4, 8], tokens [12, 4], margin [12, 4] (top-1 minus top-2) and e [12, 4]: the largest |bf16-autocast - fp32| of
  the reference's own uncached forward over those 8 entries.  A pair (row, step) is DECISIVE when margin >= 4 e; the generator asserts
  that at least half of the 48 pairs are, and that the cached logits agree with the uncached ones to 2e-5 (the oracle tests' ATOL; 1.05e-5 was
  the largest difference seen).
  past_shapes: the shapes of the reference's past_key_values after the last step.
  gen_ids_<p> / gen_logprobs_<p> for repetition_penalty p in (1.0, 1.3): the outputs of the reference's _generate_no_beam_search (greedy),
  eos_token_ids = [the token row 0 emits at its fifth new position], so that row finishes early and the others run to max_length.
  The installed transformers has no _update_model_kwargs_for_generation any more, so the method raises as it stands: the generator sets
  that helper on the INSTANCE with the meaning HF 4.x gave it (model_kwargs["past"] = outputs.past_key_values), and asserts that the
  uncached run (the helper returning model_kwargs unchanged) gives the same tokens.  RobertaForCausalLM has no _generate_no_beam_search in
  the reference (only the BERT sibling does): the sibling's function is bound to the instance, which is what model_generation.py:353
  expects to find."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402  (puts the repository root on sys.path)
import ref_shim  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

B, S, PROMPT, NEW, TOPK = 4, 30, 3, 12, 8
PENALTIES = (1.0, 1.3)


def build(kind):
    torch.manual_seed(0)
    if kind == "roberta":
        from models.xroberta import RobertaForCausalLM
        m = RobertaForCausalLM(G.roberta_cfg(2, 0))
        ids = syn.pretrain_batch(B, seed=13, with_image=False)["text_ids"][:, :PROMPT].clone()
        pad = 1
    else:
        from models.xbert import BertConfig, BertLMHeadModel
        cfg = BertConfig(**G.BERT_BASE_CONFIG)
        cfg.num_hidden_layers, cfg.fusion_layer, cfg.encoder_width = 2, 0, 768
        m = BertLMHeadModel(cfg)
        ids = syn.pretrain_batch(B, seed=13, with_image=False, vocab=30522)["text_ids"][:, :PROMPT].clone()
        ids[ids == 0] = 5
        pad = 0
    G.load_formula(m)
    m.eval()
    if not hasattr(m, "_generate_no_beam_search"):
        from models.xbert import BertLMHeadModel as Sibling
        m._generate_no_beam_search = types.MethodType(Sibling._generate_no_beam_search, m)
    return m, ids, pad


def generate(kind):
    m, prompt, pad = build(kind)
    enc = syn.gaussian("gen.image_states", (B, S, 768), 0.7)
    enc_atts = torch.ones(B, S, dtype=torch.long)
    enc_atts[1, 20:] = 0
    kw = dict(encoder_hidden_states=enc, encoder_attention_mask=enc_atts, return_dict=True, is_decoder=True)
    out = {}
    ids, past = prompt.clone(), None
    top_ids, top_vals, tokens, margins, es = [], [], [], [], []
    with torch.no_grad():
        for t in range(NEW):
            atts = torch.ones_like(ids)
            res = m(ids if past is None else ids[:, -1:], attention_mask=atts, past_key_values=past, use_cache=True, **kw)
            logits = res.logits[:, -1, :].float()
            full = m(ids, attention_mask=atts, **kw).logits[:, -1, :].float()
            assert float((logits - full).abs().max()) <= 2e-5, (t, float((logits - full).abs().max()))
            with torch.autocast("cpu", dtype=torch.bfloat16):
                amp = m(ids, attention_mask=atts, **kw).logits[:, -1, :].float()
            vals, idx = logits.topk(TOPK, dim=-1)
            G.pack(f"step{t}/logits", logits, out)
            top_ids.append(idx)
            top_vals.append(vals)
            tokens.append(idx[:, 0])
            margins.append(vals[:, 0] - vals[:, 1])
            es.append((amp.gather(1, idx) - vals).abs().max(dim=1).values)
            past = res.past_key_values
            ids = torch.cat([ids, idx[:, :1]], dim=1)
        out["past_shapes"] = np.asarray([[list(t.shape) for t in layer] for layer in past], dtype=np.int64)
    margin, e = torch.stack(margins), torch.stack(es)
    decisive = int((margin >= 4 * e).sum())
    print(f"{kind}: {decisive} of {margin.numel()} (row, step) pairs are decisive", flush=True)
    assert 2 * decisive >= margin.numel(), decisive
    out.update(top_ids=torch.stack(top_ids).numpy(), top_vals=torch.stack(top_vals).numpy().astype(np.float32),
               tokens=torch.stack(tokens).numpy(), margin=margin.numpy().astype(np.float32), e=e.numpy().astype(np.float32))
    eos = int(tokens[4][0])
    max_length = PROMPT + NEW
    m.config.is_encoder_decoder = False
    for p in PENALTIES:
        got = {}
        for route, helper in (("cached", lambda outputs, model_kwargs, is_encoder_decoder=False: {**model_kwargs, "past": outputs.past_key_values}),
                              ("uncached", lambda outputs, model_kwargs, is_encoder_decoder=False: model_kwargs)):
            m._update_model_kwargs_for_generation = helper
            with torch.no_grad():
                got[route] = m._generate_no_beam_search(prompt.clone(), PROMPT, max_length, False, 1.0, 0, 1.0, p, pad, [eos], B,
                                                        encoder_hidden_states=enc, encoder_attention_mask=enc_atts)
        assert torch.equal(got["cached"][0], got["uncached"][0]), (p, got["cached"][0], got["uncached"][0])
        assert torch.allclose(got["cached"][1], got["uncached"][1], atol=1e-5)
        out[f"gen_ids_{p}"] = got["cached"][0].numpy()
        out[f"gen_logprobs_{p}"] = got["cached"][1].numpy().astype(np.float32)
        print(f"{kind}: penalty {p}:\n{got['cached'][0]}\n{got['cached'][1]}", flush=True)
    G.save(f"generation_{kind}_2L", out, {"spec": G.spec_of(m), "kind": kind, "B": B, "S": S, "layers": 2, "prompt": prompt.tolist(),
                                          "enc_atts": enc_atts.tolist(), "new_tokens": NEW, "max_length": max_length, "pad": pad,
                                          "eos": eos, "penalties": list(PENALTIES), "decisive": decisive,
                                          "route": "cached forward (use_cache / past_key_values), teacher-forced; "
                                                   "_update_model_kwargs_for_generation set on the instance"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=("roberta", "bert"))
    a = ap.parse_args()
    torch.set_num_threads(int(os.environ.get("GEN_THREADS", "8")))
    ref_shim.install()
    for kind in ("roberta", "bert"):
        if a.only in (None, kind):
            generate(kind)


if __name__ == "__main__":
    main()
