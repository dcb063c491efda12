"""_generate_no_beam_search(do_sample=True, fused_sampling=True) on a real MI355X: the two-layer causal decoders of
tests/golden/generation_{roberta,bert}_2L.npz, built as test_hip_generation.py builds its case (that file is imported, not edited).
A step is the cached forward, the LM head and ONE Fx.sample_token launch; the returned mean log-probabilities are checked against the
project's own UNCACHED forward, teacher-forced on the generated ids."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from decode_util import finishing_invariants  # noqa: E402
from test_hip_generation import LP_TOL, Case  # noqa: E402


@pytest.fixture(scope="module", params=["roberta", "bert"])
def case(request):
    return Case(request.param)


def _generate(case, max_length=None, penalty=1.0, prompt=None, kw=None, **opt):
    prompt = case.prompt if prompt is None else prompt
    return case.m._generate_no_beam_search(prompt, prompt.shape[1], case.max_length if max_length is None else max_length,
                                           opt.pop("do_sample", True), opt.pop("temperature", 1.0), opt.pop("top_k", 0), opt.pop("top_p", 1.0),
                                           penalty, case.pad, case.eos, prompt.shape[0], **opt, **(case.kw if kw is None else kw))


def test_top_k_1_is_greedy(case):
    greedy, _ = _generate(case, do_sample=False)
    ids, lp = _generate(case, top_k=1, fused_sampling=True, seed=3)
    assert torch.equal(ids, greedy)
    assert torch.equal(lp, torch.zeros_like(lp))   # one candidate left: exp(0) = 1, log 1 = 0, exactly


def test_seeds_and_finishing(case):
    """The same torch.manual_seed gives the same ids (the call draws its 64-bit seed from torch's CPU generator); two fixed seeds give
    different ids; only pads follow an eos and unfinished rows end in eos."""
    P = case.prompt.shape[1]
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        runs.append(_generate(case, penalty=1.3, temperature=0.7, top_k=50, top_p=0.9, fused_sampling=True))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ids, lps = runs[0]
    assert tuple(ids.shape) == (case.B, case.max_length) and tuple(lps.shape) == (case.B,) and bool(torch.isfinite(lps).all())
    assert torch.equal(ids[:, :P], case.prompt)
    finishing_invariants(ids.cpu(), P, case.pad, case.eos)
    a, _ = _generate(case, temperature=2.0, fused_sampling=True, seed=5)
    b, _ = _generate(case, temperature=2.0, fused_sampling=True, seed=6)
    a2, _ = _generate(case, temperature=2.0, fused_sampling=True, seed=5)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    finishing_invariants(a.cpu(), P, case.pad, case.eos)
    u = torch.rand((case.B, case.max_length - P), generator=torch.Generator().manual_seed(9))
    c, _ = _generate(case, fused_sampling=True, uniforms=u)
    c2, _ = _generate(case, fused_sampling=True, uniforms=u.cuda(), seed=77)   # given uniforms: the seed plays no part
    assert torch.equal(c, c2)


def _teacher_forced_mean(case, ids, kw, eos):
    """Mean over a row's own steps (those before and including its first eos) of log_softmax of the UNCACHED forward at the id."""
    P = case.prompt.shape[1]
    with torch.no_grad():
        logits = case.m(ids, attention_mask=torch.ones_like(ids), **kw).logits.float()
    lp = torch.log_softmax(logits[:, P - 1:-1].double(), dim=-1).gather(2, ids[:, P:].unsqueeze(-1)).squeeze(-1)   # [B, steps]
    is_eos = torch.zeros_like(ids[:, P:], dtype=torch.bool)
    for e in eos:
        is_eos |= ids[:, P:] == e
    before = torch.cumsum(is_eos.long(), 1) - is_eos.long()    # eos tokens strictly before the step
    own = (before == 0).double()
    return (lp * own).sum(1) / own.sum(1)


def _check_logprobs(case, prompt, kw_gen, kw_full, seed):
    """Penalty 1, temperature 1, no filter: the returned score is the model's own log-probability of what it drew.  The last column of
    an unfinished row is overwritten by eos, so the drawn ids are read from a second run with one more column (same seed, same rows,
    same steps: the same draws), which must agree with the first run everywhere else."""
    L = case.max_length
    ids, lp = _generate(case, prompt=prompt, kw=kw_gen, fused_sampling=True, seed=seed)
    longer, _ = _generate(case, max_length=L + 1, prompt=prompt, kw=kw_gen, fused_sampling=True, seed=seed)
    drawn = longer[:, :L].contiguous()
    assert torch.equal(drawn[:, :L - 1], ids[:, :L - 1])
    finishing_invariants(ids.cpu(), prompt.shape[1], case.pad, case.eos)
    want = _teacher_forced_mean(case, drawn, kw_full, case.eos)
    print(f"{case.kind}: returned {lp.cpu().tolist()}\nteacher-forced {want.cpu().tolist()}")
    assert torch.allclose(lp.double().cpu(), want.cpu(), rtol=LP_TOL, atol=LP_TOL), (lp, want)
    return ids


def test_logprobs_are_the_models_own(case):
    _check_logprobs(case, case.prompt, case.kw, case.kw, seed=21)


def test_shared_encoder_states(case):
    """n samples per image through encoder_batch_index over DISTINCT encoder states: the scores match the uncached forward on the tiled
    states, which fails if a sample attends to the wrong image."""
    n = 2
    index = torch.arange(case.B, device="cuda").repeat_interleave(n)
    prompt = case.prompt.repeat_interleave(n, 0).contiguous()
    kw_gen = dict(case.kw, encoder_batch_index=index)
    kw_full = dict(encoder_hidden_states=case.enc.repeat_interleave(n, 0).contiguous(),
                   encoder_attention_mask=case.enc_atts.repeat_interleave(n, 0).contiguous())
    ids = _check_logprobs(case, prompt, kw_gen, kw_full, seed=22)
    assert not torch.equal(ids[0::2], ids[1::2]), "the two samples of every image are the same draw"


def test_default_path_is_unchanged(case):
    """fused_sampling=False runs the torch sampling lines as before: the same outputs under the same torch seed as a call without the
    keyword."""
    outs = []
    for opt in ({}, {"fused_sampling": False}, {"fused_sampling": False, "seed": 4}):
        torch.manual_seed(1234)
        outs.append(_generate(case, penalty=1.3, temperature=0.7, top_k=50, top_p=0.9, **opt))
    for ids, lp in outs[1:]:
        assert torch.equal(ids, outs[0][0]) and torch.equal(lp, outs[0][1])
