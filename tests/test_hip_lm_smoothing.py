"""Label smoothing in the causal LM heads on a real MI355X: xbert.BertLMHeadModel(config, label_smoothing) against the reference's own class
(bert_causal_lm_smooth_2L.npz: xbert.py:1346-1347 -> LabelSmoothSoftmaxCEV1 on the inputs of bert_causal_lm_2L), and
xroberta.RobertaForCausalLM(config, label_smoothing), the keyword model_generation.py:275 passes, with the same convention."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, rel_l2  # noqa: E402
from test_hip_modules import COS_TOL, GRAD_TOL, _check_grads, _check_out, _load_into  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402


def _spec(m):
    return {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()}


def _v1_rows(x, label, s):
    """LabelSmoothSoftmaxCEV1.forward (xbert.py:1210-1223) with reduction 'none', written out."""
    ignore = label.eq(-100)
    label = label.clone()
    label[ignore] = 0
    lb_pos, lb_neg = 1. - s, s / x.size(1)
    lb_one_hot = torch.empty_like(x).fill_(lb_neg).scatter_(1, label.unsqueeze(1), lb_pos)
    loss = -torch.sum(torch.log_softmax(x, dim=1) * lb_one_hot, dim=1)
    return loss.masked_fill(ignore, 0.0), ignore.eq(0).sum()


def test_bert_causal_lm_label_smoothing_vs_golden():
    """The case of test_hip_modules.test_bert_causal_lm_answer_decoder_vs_golden with label_smoothing = 0.1, same comparator and bounds;
    the fixture also holds the reduction='mean' loss."""
    from xfm_amd.xbert import BertConfig, BertLMHeadModel
    z, meta = load("bert_causal_lm_smooth_2L")
    B, L, S = meta["B"], meta["L"], meta["S"]
    assert meta["label_smoothing"] == 0.1
    m = BertLMHeadModel(BertConfig(num_hidden_layers=meta["layers"], fusion_layer=0, encoder_width=768), label_smoothing=meta["label_smoothing"])
    assert _spec(m) == meta["spec"] == load("bert_causal_lm_2L")[1]["spec"]   # state-dict keys unchanged
    _load_into(m, meta["spec"])
    m.cuda().finalize().eval()
    ids, atts, enc_atts = (torch.tensor(meta[k]).cuda() for k in ("ids", "atts", "enc_atts"))
    enc = syn.gaussian("causal.question_states", (B, S, 768), 0.7).cuda().requires_grad_(True)
    weights = (syn.gaussian("causal.weights", (B,), 1.0).abs() + 0.1).cuda()
    labels = ids.masked_fill(ids == 0, -100)
    with torch.no_grad():
        full = m(ids, attention_mask=atts, encoder_hidden_states=enc, encoder_attention_mask=enc_atts)
        mean = m(ids, attention_mask=atts, encoder_hidden_states=enc, encoder_attention_mask=enc_atts, labels=labels, return_dict=True,
                 reduction="mean")
    _check_out(z, "logits", full.logits)
    ref_mean = float(z["loss_mean"])
    assert abs(float(mean.loss) - ref_mean) <= 2e-3 * abs(ref_mean), (float(mean.loss), ref_mean)
    res = m(ids, attention_mask=atts, encoder_hidden_states=enc, encoder_attention_mask=enc_atts, labels=labels, return_dict=True,
            reduction="none")
    ref_rows = torch.from_numpy(z["loss_rows"])
    assert torch.allclose(res.loss.float().cpu(), ref_rows, rtol=3e-3, atol=3e-3), (res.loss, ref_rows)
    loss = (weights * res.loss).sum() / B
    ref = float(z["loss"])
    assert abs(float(loss) - ref) <= 2e-3 * abs(ref), (float(loss), ref)
    loss.backward()
    _check_grads(z, "grad", m)
    err, cos = rel_l2(z, "grad_in/question_states", enc.grad)
    assert err <= GRAD_TOL and cos >= COS_TOL, (err, cos)


def _roberta_case(**kw):
    from xfm_amd.xroberta import RobertaConfig, RobertaForCausalLM
    z, meta = load("causal_lm_2L")
    m = RobertaForCausalLM(RobertaConfig(num_hidden_layers=meta["layers"], fusion_layer=0, encoder_width=768), **kw)
    assert _spec(m) == meta["spec"]
    _load_into(m, meta["spec"])
    m.cuda().finalize().eval()
    ids, atts, enc_atts = (torch.tensor(meta[k]).cuda() for k in ("ids", "atts", "enc_atts"))
    enc = syn.gaussian("causal.question_states", (meta["B"], meta["S"], 768), 0.7).cuda().requires_grad_(True)
    call = dict(attention_mask=atts, encoder_hidden_states=enc, encoder_attention_mask=enc_atts, labels=ids.masked_fill(ids == 1, -100),
                return_dict=True)
    return m, ids, enc, call


def test_roberta_causal_lm_label_smoothing_is_the_v1_expression_of_its_own_logits():
    m, ids, enc, call = _roberta_case(label_smoothing=0.1)
    B, V = ids.shape[0], m.config.vocab_size
    with torch.no_grad():
        none = m(ids, reduction="none", **call)
        mean = m(ids, reduction="mean", **call)
        total = m(ids, reduction="sum", **call)
    rows, n_valid = _v1_rows(none.logits.reshape(-1, V).float(), call["labels"][:, 1:].reshape(-1), 0.1)
    for what, got, ref in (("none", none.loss, rows.view(B, -1).sum(1)), ("mean", mean.loss.reshape(1), (rows.sum() / n_valid).reshape(1)),
                           ("sum", total.loss.reshape(1), rows.sum().reshape(1))):
        err = float((got.float() - ref).abs().max()) / float(ref.abs().max())
        print(f"reduction {what}: max err / max|ref| = {err:.3e}")
        assert err <= 1e-5, (what, err)


def test_roberta_causal_lm_label_smoothing_zero_is_the_plain_path_bit_for_bit(monkeypatch):
    """label_smoothing = 0.0 launches what the model without the keyword launches: loss and every gradient bit-identical.  (With
    XFM_DETERMINISTIC=1, as in the accelerator's bit-reproducibility test: by default a few small gradients end in float atomics and
    differ between any two runs.)"""
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    weights = (syn.gaussian("causal.weights", (6,), 1.0).abs() + 0.1).cuda()
    runs = []
    for kw in ({}, {"label_smoothing": 0.0}):
        m, ids, enc, call = _roberta_case(**kw)
        res = m(ids, reduction="none", **call)
        (weights * res.loss).sum().backward()
        torch.cuda.synchronize()
        runs.append((res.loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, enc.grad.clone()))
    (l0, g0, e0), (l1, g1, e1) = runs
    assert torch.equal(l0, l1) and torch.equal(e0, e1) and sorted(g0) == sorted(g1) and len(g0) > 10
    assert [n for n in g0 if not torch.equal(g0[n], g1[n])] == []
