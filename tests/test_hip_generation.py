"""Cached incremental decoding and greedy / sampled generation of the causal decoders on a real MI355X, against the fixtures taken from the
reference's own cached forward and _generate_no_beam_search (tests/golden/generation_{roberta,bert}_2L.npz, tools/oracle/gen_generation.py)
and against the project's own uncached forward.  Tolerances are the module tests' (tests/test_hip_modules.py): tower outputs rel-L2 <= 2e-2
and cosine >= 0.996, per-sequence log-probabilities rtol = atol = 3e-3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from decode_util import decisive, finishing_invariants, generate_ref  # noqa: E402
from golden_util import load, rel_l2, state_from_spec  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

OUT_TOL, COS_TOL = 2e-2, 0.996
LP_TOL = 3e-3


class Case:
    def __init__(self, kind):
        self.kind = kind
        self.z, self.meta = load(f"generation_{kind}_2L")
        meta = self.meta
        if kind == "roberta":
            from xfm_amd.xroberta import RobertaConfig, RobertaForCausalLM
            m = RobertaForCausalLM(RobertaConfig(num_hidden_layers=meta["layers"], fusion_layer=0, encoder_width=768))
        else:
            from xfm_amd.xbert import BertConfig, BertLMHeadModel
            m = BertLMHeadModel(BertConfig(num_hidden_layers=meta["layers"], fusion_layer=0, encoder_width=768))
        ours = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()}
        assert ours == meta["spec"]
        m.load_state_dict(state_from_spec(meta["spec"]), strict=True)
        self.m = m.cuda().finalize().eval()
        self.B, self.S, self.NEW, self.max_length = meta["B"], meta["S"], meta["new_tokens"], meta["max_length"]
        self.enc = syn.gaussian("gen.image_states", (self.B, self.S, 768), 0.7).cuda()
        self.enc_atts = torch.tensor(meta["enc_atts"]).cuda()
        self.prompt = torch.tensor(meta["prompt"]).cuda()
        self.tokens = torch.from_numpy(self.z["tokens"]).cuda()
        self.pad, self.eos = meta["pad"], [meta["eos"]]
        self.kw = dict(encoder_hidden_states=self.enc, encoder_attention_mask=self.enc_atts)
        self._steps = None

    def teacher_forced(self):
        """The cached forward, teacher-forced on the fixture's tokens: ([logits [B, V] per step], [past after each step]), computed once."""
        if self._steps is None:
            logits, pasts = [], []
            ids, past = self.prompt.clone(), None
            with torch.no_grad():
                for t in range(self.NEW):
                    out = self.m(ids if past is None else ids[:, -1:], attention_mask=torch.ones_like(ids), past_key_values=past,
                                 use_cache=True, cache_capacity=self.max_length, **self.kw)
                    past = out.past_key_values
                    logits.append(out.logits[:, -1, :].float().clone())
                    pasts.append(past)
                    ids = torch.cat([ids, self.tokens[t].view(-1, 1)], dim=1)
            self._steps, self.full_ids = (logits, pasts), ids
        return self._steps


@pytest.fixture(scope="module", params=["roberta", "bert"])
def case(request):
    return Case(request.param)


def _rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30)), float((a @ b) / (a.norm() * b.norm() + 1e-30))


def test_teacher_forced_cached_steps_vs_reference(case):
    """(a) every step's last-position logits against the reference's cached forward; our argmax is the reference's token on every
    decisive (row, step) pair and its top-1 or top-2 elsewhere; at least half of the pairs must be decisive."""
    z = case.z
    logits, _ = case.teacher_forced()
    dec = decisive(z)
    assert 2 * int(dec.sum()) >= dec.numel(), "fewer than half of the (row, step) pairs are decisive: the fixture compares too little"
    for t in range(case.NEW):
        err, cos = rel_l2(z, f"step{t}/logits", logits[t])
        print(f"{case.kind} step {t}: rel-L2 {err:.3e} cos {cos:.6f}")
        assert err <= OUT_TOL and cos >= COS_TOL, (case.kind, t, err, cos)
        top = logits[t].argmax(-1).cpu()
        for b in range(case.B):
            if dec[t, b]:
                assert int(top[b]) == int(z["tokens"][t, b]), (case.kind, t, b, int(top[b]), z["top_ids"][t, b].tolist())
            else:
                assert int(top[b]) in z["top_ids"][t, b, :2].tolist(), (case.kind, t, b, int(top[b]), z["top_ids"][t, b].tolist())


def test_cached_steps_vs_uncached_forward(case):
    """(b) step t from the cache against row t of the existing full forward on the same prefix (causal: row t sees the prefix only),
    at every step, the step after the prompt included."""
    logits, _ = case.teacher_forced()
    P = case.prompt.shape[1]
    with torch.no_grad():
        full = case.m(case.full_ids, attention_mask=torch.ones_like(case.full_ids), **case.kw).logits.float()
    for t in range(case.NEW):
        err, cos = _rel(logits[t], full[:, P - 1 + t])
        print(f"{case.kind} step {t}: cached vs uncached rel-L2 {err:.3e} cos {cos:.6f}")
        assert err <= OUT_TOL and cos >= COS_TOL, (case.kind, t, err, cos)


def test_cache_contract(case):
    """(c) len(past) = layers, (k, v) are [B, 12, len, 64]; fp32 clones fed back as a plain tuple give the same logits as the KVCache;
    _reorder_cache + one step = that step on the permuted batch."""
    from xfm_amd.decode import KVCache
    logits, pasts = case.teacher_forced()
    t = 5
    past = pasts[t - 1]                      # the cache BEFORE step t: prompt + t tokens
    L = case.prompt.shape[1] + t - 1
    assert isinstance(past, KVCache) and isinstance(past, tuple) and len(past) == case.meta["layers"]
    for k, v in past:
        assert tuple(k.shape) == tuple(v.shape) == (case.B, 12, L, 64)
    assert [list(x.shape) for x in pasts[-1][0]] == case.z["past_shapes"][0].tolist()
    ids = case.full_ids[:, :L + 1]
    plain = tuple((k.float().clone(), v.float().clone()) for k, v in past)
    with torch.no_grad():
        out = case.m(ids[:, -1:], attention_mask=torch.ones_like(ids), past_key_values=plain, use_cache=True, cache_capacity=case.max_length,
                     **case.kw)
        err, cos = _rel(out.logits[:, -1], logits[t])
        assert err <= OUT_TOL and cos >= COS_TOL, (err, cos)
        assert isinstance(out.past_key_values, KVCache) and out.past_key_values.length == L + 1
        beam = torch.tensor([2, 0, 0, 3], device="cuda")
        re = case.m._reorder_cache(past, beam)
        assert isinstance(re, KVCache) and torch.equal(re[1][0], past[1][0][beam])
        kw = dict(encoder_hidden_states=case.enc[beam].contiguous(), encoder_attention_mask=case.enc_atts[beam].contiguous())
        out = case.m(ids[beam][:, -1:], attention_mask=torch.ones_like(ids), past_key_values=re, use_cache=True, **kw)
        err, cos = _rel(out.logits[:, -1], logits[t][beam])
        assert err <= OUT_TOL and cos >= COS_TOL, (err, cos)
        with pytest.raises(NotImplementedError):
            case.m(ids[:, -2:], past_key_values=past, use_cache=True, **case.kw)
        with pytest.raises(ValueError):
            case.m(ids[:, -1:], past_key_values=pasts[-1].grown(case.max_length), use_cache=True, **case.kw)


def _own_logits(case):
    """The logits callback of decode_util.generate_ref, on our own cached forward: the same kernels on the same shapes as
    _generate_no_beam_search runs, so the tokens must be the same."""
    from xfm_amd.decode import head_logits
    tower, head = case.m._generation_parts()
    state = {"past": None}

    def fn(input_ids):
        ids = input_ids.cuda()
        with torch.no_grad():
            out = tower(ids if state["past"] is None else ids[:, -1:].contiguous(), past_key_values=state["past"], use_cache=True,
                        is_decoder=True, cache_capacity=case.max_length, **case.kw)
            state["past"] = out.past_key_values
            return head_logits(head, out.last_hidden_state[:, -1, :])[:, :case.m.config.vocab_size]
    return fn


def _generate(case, penalty, sync_every=None, **kw):
    extra = {} if sync_every is None else {"sync_every": sync_every}
    return case.m._generate_no_beam_search(case.prompt, case.prompt.shape[1], case.max_length, kw.get("do_sample", False),
                                           kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0), penalty, case.pad, case.eos,
                                           case.B, **extra, **case.kw)


@pytest.mark.parametrize("penalty", [1.0, 1.3])
def test_generate_no_beam_search_greedy(case, penalty):
    """(d) exactly the restatement of xbert.py:1418-1484 driven step by step by our own cached forward; the same for sync_every 1 and 100;
    [B, max_length]; only pads after an eos; eos forced at the last column of unfinished rows; mean log-probabilities within 3e-3."""
    ids, lp = _generate(case, penalty)
    want_ids, want_lp = generate_ref(_own_logits(case), case.prompt.cpu(), case.prompt.shape[1], case.max_length, penalty, case.pad, case.eos,
                                     case.B)
    print(f"{case.kind} penalty {penalty}: ours\n{ids.cpu()}\n{lp.cpu()}\nreference (fixture)\n{case.z[f'gen_ids_{penalty}']}\n"
          f"{case.z[f'gen_logprobs_{penalty}']}")
    assert tuple(ids.shape) == (case.B, case.max_length) and ids.dtype == torch.int64
    assert torch.equal(ids.cpu(), want_ids), (ids.cpu(), want_ids)
    assert torch.allclose(lp.float().cpu(), want_lp, rtol=LP_TOL, atol=LP_TOL), (lp, want_lp)
    finishing_invariants(ids.cpu(), case.prompt.shape[1], case.pad, case.eos)
    for se in (1, 100):
        ids2, lp2 = _generate(case, penalty, sync_every=se)
        assert torch.equal(ids2, ids) and torch.equal(lp2, lp), se
    # the reference's own output: equal wherever every step of the row was decisive in the teacher-forced run (penalty 1.0 follows it)
    if penalty == 1.0:
        dec = decisive(case.z)
        ref_ids = torch.from_numpy(case.z["gen_ids_1.0"])
        for b in range(case.B):
            if bool(dec[:, b].all()):
                assert ids[b].cpu().tolist() == ref_ids[b].tolist(), b


def test_generate_sampling(case):
    """(e) top_k = 1 reproduces greedy; with do_sample and a fixed seed the shapes and the finishing invariants hold."""
    greedy, lp = _generate(case, 1.0)
    torch.manual_seed(1234)
    ids, lp1 = _generate(case, 1.0, do_sample=True, top_k=1)
    assert torch.equal(ids, greedy)
    assert torch.allclose(lp1, torch.zeros_like(lp1))       # one candidate left: its log-probability is 0
    torch.manual_seed(1234)
    ids, lps = _generate(case, 1.3, do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
    assert tuple(ids.shape) == (case.B, case.max_length) and tuple(lps.shape) == (case.B,) and bool(torch.isfinite(lps).all())
    assert torch.equal(ids[:, :case.prompt.shape[1]], case.prompt)
    finishing_invariants(ids.cpu(), case.prompt.shape[1], case.pad, case.eos)
    torch.manual_seed(1234)
    again, _ = _generate(case, 1.3, do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
    assert torch.equal(again, ids)
