"""The GLUE metric kernels, the regression loss and the loop on a real MI355X: xfm_cls_eval against torch.argmax and a bincount,
xfm_corr_rank against an fp64 restatement written in tests/glue_loop_util.py, xfm_mse_fwd / bwd against fp64 under elementwise bounds, the
regression branch of XFMForClassification and the three loop runs through RCCLDDPAccelerator against tests/golden/glue_loop_small.npz.
In every kernel test every operand lies at an unaligned offset inside a larger buffer filled with a poison value, and everything outside
the documented outputs must still hold the poison afterwards.

Tolerances:
  correlations  1e-10 against the fp64 restatement.  Derived, not measured: the absolute error of r from ordered fp64 sums of N terms is at
                most a small multiple of N * 2^-53 (Cauchy-Schwarz bounds |Sxy| by sqrt(Sxx Syy), so the relative errors of the three sums
                add), under 1e-12 at N = 8192; 1e-10 leaves two orders of margin.  Ranks are compared for equality.
  MSE           fp64 of the ACTUAL inputs; per element one rounding each for the difference, the product and the division (bwd: 2 U32
                |ref| covers four); the forward sum of B non-negative terms is charged B roundings relative to itself, plus the
                difference, the fma and the division: (B / 2 + 4) U32 ref  (U32 = 2^-23 = two fp32 unit roundoffs, as tests/rowwise_util.py).
  model         the rule tests/test_hip_modules.py uses for the task models: logits by its _check_out (rel-L2 <= 2e-2, cosine >= 0.996),
                the loss of the text-only classification branch within 5e-3 relative
                (test_classification_multimodal_and_text_branches_vs_golden)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from glue_loop_util import (correlations_restated, eval_batches, fixture, loop_config, ranks_restated, run_spec, train_batches)  # noqa: E402
from golden_util import state_from_spec  # noqa: E402
from test_hip_modules import _check_out  # noqa: E402
from xfm_amd import glue_loop as GL  # noqa: E402

F32, BF16, I64, F64 = torch.float32, torch.bfloat16, torch.int64, torch.float64
U32 = 2.0 ** -23
LOSS_TOL = 5e-3
CORR_TOL = 1e-10


def _fx():
    from xfm_amd import functional as Fx
    return Fx


def _lib():
    from xfm_amd import _lib
    return _lib


def _inside(t, before, after, fill):
    """(view, parent): t copied into a longer 1-D buffer filled with `fill`, `before` elements in (so that the view's base is not on 16
    bytes for the 4- and 2-byte types and odd `before`)."""
    flat = t.reshape(-1)
    parent = torch.full((before + flat.numel() + after,), fill, dtype=t.dtype, device="cuda")
    view = parent[before:before + flat.numel()]
    view.copy_(flat)
    return view, parent


def _poison_kept(parent, lo, hi, fill, what):
    """every element of the 1-D parent outside [lo, hi) still holds the fill"""
    want = torch.full((), fill, dtype=parent.dtype, device=parent.device)
    bad = int((parent[:lo] != want).sum()) + int((parent[hi:] != want).sum())
    assert bad == 0, f"{what}: {bad} elements outside the output changed"


# ---------------------------------------------------------------------------------------------------------------- xfm_cls_eval
def _cls_case(B, L, seed):
    """Logits over +-4 with, where the batch has the rows: row 0 all equal, row 1 a tie between the LAST two columns (the maximum), row 2
    a NaN row (two NaNs: the first wins), row 3 a -0.0 before a +0.0 above negative values.  Labels: random, with a -1 and an L."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, L), generator=g) * 8.0 - 4.0
    labels = torch.randint(0, L, (B,), generator=g)
    x[0] = 0.75
    if B > 1:
        x[1, L - 2:] = 5.0
    if B > 2:
        x[2, L - 1] = float("nan")
        x[2, L // 2] = float("nan")
    if B > 3:
        x[3] = -1.0 - torch.rand(L, generator=g)
        x[3, L - 1] = 0.0
        x[3, max(L - 2, 0)] = -0.0
    if B > 4:
        labels[4] = -1
    if B > 5:
        labels[5] = L
    return x, labels


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", [1, 7, 8, 33, 300])
@pytest.mark.parametrize("L", [2, 3, 5, 32])
def test_cls_eval_matches_torch_argmax_and_bincount(L, B, pad):
    Fx = _fx()
    assert L <= Fx.METRIC_MAX_L == 32
    ld = L + pad
    x, labels = _cls_case(B, L, 100 * L + B)
    ref_pred = torch.argmax(x, dim=-1)
    if B > 3:
        assert int(ref_pred[0]) == 0 and int(ref_pred[1]) == L - 2 and int(ref_pred[2]) == L // 2 and int(ref_pred[3]) == max(L - 2, 0)
    ok = (labels >= 0) & (labels < L)
    ref_conf = torch.bincount(labels[ok] * L + ref_pred[ok], minlength=L * L)
    POISON = 3.0e30   # a padding column that is read would win every argmax
    rows = torch.full((B, ld), POISON)
    rows[:, :L] = x
    lg_view, lg_parent = _inside(rows, 3, 5, POISON)
    logits = lg_view.view(B, ld)[:, :L]
    assert logits.data_ptr() % 16 != 0
    lab, lab_parent = _inside(labels, 1, 2, -7)
    conf, conf_parent = _inside(torch.zeros(L * L, dtype=I64), 1, 3, 1234567)
    off = 5
    pred_parent = torch.full((1 + off + B + 4,), -99, dtype=I64, device="cuda")
    pred = pred_parent[1:]
    before = lg_parent.clone()
    Fx.cls_eval(logits, L, lab, conf, pred, off)
    assert pred_parent[1 + off:1 + off + B].cpu().tolist() == ref_pred.tolist()
    _poison_kept(pred_parent, 1 + off, 1 + off + B, -99, "pred")
    assert conf.cpu().tolist() == ref_conf.tolist()
    _poison_kept(conf_parent, 1, 1 + L * L, 1234567, "conf")
    _poison_kept(lab_parent, 1, 1 + B, -7, "labels")
    assert torch.equal(lg_parent.view(torch.int32), before.view(torch.int32))
    Fx.cls_eval(logits, L, lab, conf, None, 0)          # conf accumulates: a second call doubles it exactly; pred may be NULL
    assert conf.cpu().tolist() == (2 * ref_conf).tolist()
    _poison_kept(pred_parent, 1 + off, 1 + off + B, -99, "pred (NULL call)")
    _poison_kept(conf_parent, 1, 1 + L * L, 1234567, "conf (second call)")


def test_cls_eval_argument_errors_launch_nothing():
    Fx, lib = _fx(), _lib().load()
    x = torch.zeros((4, 3), device="cuda")
    labels = torch.zeros(4, dtype=I64, device="cuda")
    conf = torch.full((9,), 5, dtype=I64, device="cuda")
    for bad in (dict(B=0), dict(L=1), dict(L=33), dict(ld=2), dict(off=-1)):
        kw = dict(ld=3, B=4, L=3, off=0)
        kw.update(bad)
        rc = lib.xfm_cls_eval(x.data_ptr(), kw["ld"], kw["B"], kw["L"], labels.data_ptr(), conf.data_ptr(), None, kw["off"], None)
        assert rc == -1 and b"cls_eval" in lib.xfm_last_error(), bad
    with pytest.raises(_lib().XfmHipError, match="cls_eval"):
        Fx.cls_eval(x, 3, labels, conf, torch.zeros(8, dtype=I64, device="cuda"), -1)
    torch.cuda.synchronize()
    assert conf.tolist() == [5] * 9


# ---------------------------------------------------------------------------------------------------------------- xfm_corr_rank
def _corr_call(x, y, ranks=True):
    """The C entry point on operands inside poisoned buffers (x, y one float past a 16-byte boundary) -> (out [2], rank_x, rank_y) on
    the host, after checking that nothing outside the outputs changed."""
    Fx, lib = _fx(), _lib().load()
    N = x.numel()
    POISON = -6.5e9
    xv, xp = _inside(x.to(F32), 1, 3, POISON)
    yv, yp = _inside(y.to(F32), 5, 2, POISON)
    assert xv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 4
    xb, yb = xp.clone(), yp.clone()
    outp = torch.full((5,), POISON, dtype=F64, device="cuda")
    rxp = torch.full((N + 4,), POISON, dtype=F32, device="cuda")
    ryp = torch.full((N + 6,), POISON, dtype=F32, device="cuda")
    rc = lib.xfm_corr_rank(xv.data_ptr(), yv.data_ptr(), N, outp[2:].data_ptr(), rxp[1:].data_ptr() if ranks else None,
                           ryp[3:].data_ptr() if ranks else None, Fx._stream())
    assert rc == 0, lib.xfm_last_error()
    torch.cuda.synchronize()
    _poison_kept(outp, 2, 4, POISON, "out")
    _poison_kept(rxp, 1, 1 + N if ranks else 1, POISON, "rank_x")
    _poison_kept(ryp, 3, 3 + N if ranks else 3, POISON, "rank_y")
    assert torch.equal(xp.view(torch.int32), xb.view(torch.int32)) and torch.equal(yp.view(torch.int32), yb.view(torch.int32))
    return outp[2:4].cpu().numpy(), rxp[1:1 + N].cpu().numpy(), ryp[3:3 + N].cpu().numpy()


def _corr_inputs(N, seed):
    """x: Gaussian predictions with a few repeated values; y: scores on the 0.2 grid in [0, 5] (tie-heavy), correlated with x."""
    g = np.random.default_rng(seed)
    x = g.standard_normal(N).astype(np.float32)
    if N >= 5:
        x[N // 2] = x[0]
        x[N - 1] = x[1]
    y = np.clip(np.round((2.5 + 1.2 * x + g.standard_normal(N)) * 5.0) / 5.0, 0.0, 5.0).astype(np.float32)
    if N == 2:
        y = np.asarray([0.2, 3.4], dtype=np.float32)
    return x, y


@pytest.mark.parametrize("N", [2, 3, 5, 257, 1500, 8192])
def test_corr_rank_matches_the_fp64_restatement(N):
    assert _fx().CORR_MAX_N == 8192
    x, y = _corr_inputs(N, 7 + N)
    out, rx, ry = _corr_call(torch.from_numpy(x), torch.from_numpy(y))
    assert np.array_equal(rx.astype(np.float64), ranks_restated(x)), "rank_x"
    assert np.array_equal(ry.astype(np.float64), ranks_restated(y)), "rank_y"
    if N >= 257:
        assert len(set(ry.tolist())) <= 26 and float(ry.max()) != float(N)   # tie runs in the labels
    want = correlations_restated(x, y)
    print(f"N={N}: kernel {out.tolist()} restatement {want} diff {abs(out[0] - want[0]):.3e} {abs(out[1] - want[1]):.3e}")
    assert abs(out[0] - want[0]) <= CORR_TOL and abs(out[1] - want[1]) <= CORR_TOL
    again, _, _ = _corr_call(torch.from_numpy(x), torch.from_numpy(y), ranks=False)   # NULL rank outputs; the same bits
    assert again.tobytes() == out.tobytes()


def test_corr_rank_special_cases():
    Fx, lib = _fx(), _lib().load()
    g = np.random.default_rng(3)
    x = g.standard_normal(100).astype(np.float32)
    out, rx, ry = _corr_call(torch.from_numpy(x), torch.full((100,), 2.4))          # all-tied y: zero denominators
    assert np.isnan(out).all() and np.array_equal(ry, np.full(100, 50.5, dtype=np.float32)) and np.array_equal(rx, ranks_restated(x))
    v = np.asarray([0.4, -0.0, 0.4, 0.0, -3.0, 0.4, -1e-30, 1e-30, -np.inf, np.inf, -2.5, 7.0], dtype=np.float32)
    w = np.asarray([1.0, 2.0, -1.0, 2.0, -5.0, 0.5, 0.0, -0.0, -7.0, 9.0, -0.0, 3.0], dtype=np.float32)
    out, rx, ry = _corr_call(torch.from_numpy(v), torch.from_numpy(w))
    assert np.array_equal(rx, ranks_restated(v)) and np.array_equal(ry, ranks_restated(w))
    assert rx[1] == rx[3] and ry[6] == ry[7] == ry[10]                                # -0.0 == +0.0
    fin = np.isfinite(v)
    out, rx, ry = _corr_call(torch.from_numpy(v[fin]), torch.from_numpy(w[fin]))     # negative values and the zero pair, finite
    want = correlations_restated(v[fin], w[fin])
    assert np.array_equal(rx, ranks_restated(v[fin])) and abs(out[0] - want[0]) <= CORR_TOL and abs(out[1] - want[1]) <= CORR_TOL
    bad = x.copy()
    bad[17] = np.nan
    out, _, _ = _corr_call(torch.from_numpy(bad), torch.from_numpy(x))               # a NaN: both outputs NaN
    assert np.isnan(out).all()
    out, _, _ = _corr_call(torch.from_numpy(x), torch.from_numpy(bad), ranks=False)
    assert np.isnan(out).all()
    # above the cap: XFM_E_ARG from the C call, nothing launched
    big = torch.zeros(Fx.CORR_MAX_N + 1, device="cuda")
    o = torch.full((2,), 3.0, dtype=F64, device="cuda")
    rc = lib.xfm_corr_rank(big.data_ptr(), big.data_ptr(), Fx.CORR_MAX_N + 1, o.data_ptr(), None, None, None)
    assert rc == -1 and b"corr_rank" in lib.xfm_last_error()
    with pytest.raises(_lib().XfmHipError, match="corr_rank"):
        Fx.corr_rank(big, big)
    torch.cuda.synchronize()
    assert o.tolist() == [3.0, 3.0]


class _Column(torch.nn.Module):
    """A regression `model` that returns rows of a fixed prediction column (the loop's call form)."""

    def __init__(self, preds):
        super().__init__()
        self.preds, self.at = preds, 0

    def forward(self, image, text_ids, text_atts, targets, train=True):
        n = text_ids.shape[0]
        out = self.preds[self.at:self.at + n].view(n, 1)
        self.at += n
        return out


@pytest.mark.parametrize("rows,kernel", [(8192, True), (8193, False)])
def test_evaluate_uses_the_kernel_up_to_the_cap_and_the_host_form_above(rows, kernel, monkeypatch):
    Fx = _fx()
    x, y = _corr_inputs(rows, 11)
    bs = 2731   # batches of 2731 rows and a shorter last one
    loader, o = [], 0
    while o < rows:
        n = min(bs, rows - o)
        loader.append((torch.zeros(n, 1, dtype=I64), torch.ones(n, 1, dtype=I64), torch.from_numpy(y[o:o + n])))
        o += n
    calls, reads = [], []
    real_corr, real_read = Fx.corr_rank, GL._read
    monkeypatch.setattr(Fx, "corr_rank", lambda *a, **kw: (calls.append(a[0].numel()), real_corr(*a, **kw))[1])
    monkeypatch.setattr(GL, "_read", lambda t: (reads.append(tuple(t.shape)), real_read(t))[1])
    cfg = {"task_name": "stsb", "num_labels": 1, "per_device_eval_batch_size": bs}
    res = GL.evaluate(_Column(torch.from_numpy(x).cuda()), loader, torch.device("cuda"), cfg)
    assert calls == ([rows] if kernel else []) and len(reads) == 1 and res.count == rows
    want = correlations_restated(x, y)
    assert abs(res["pearson"] - want[0]) <= CORR_TOL and abs(res["spearmanr"] - want[1]) <= CORR_TOL
    assert np.array_equal(np.asarray(res.predictions, dtype=np.float32), x)


# ---------------------------------------------------------------------------------------------------------------- xfm_mse_fwd / bwd
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B", [1, 4, 33, 1000])
def test_small_mse_against_fp64_bounds(B, dtype):
    Fx = _fx()
    from xfm_amd.ops import small_mse
    g = torch.Generator().manual_seed(40 + B)
    stride = 3
    cols = (torch.rand((B, stride), generator=g) * 6.0 - 0.5).to(dtype)
    target = (torch.randint(0, 26, (B,), generator=g).float() / 5.0)
    POISON = 9.0e8
    pv, pp = _inside(cols, 1, 3, POISON)
    pred = pv.view(B, stride)[:, 1]                                  # a strided column inside the buffer, off 16 bytes
    assert pred.stride(0) == stride and pred.data_ptr() % 16 != 0
    tv, tp = _inside(target, 3, 1, POISON)
    pb, tb = pp.clone(), tp.clone()
    d = cols[:, 1].double() - target.double()
    ref = float((d * d).sum() / B)
    loss = Fx.mse_fwd(pred, tv)
    got = float(loss)
    bound = (B / 2 + 4) * U32 * ref + 2.0 ** -126
    print(f"B={B} {dtype}: loss {got!r} fp64 {ref!r} err / bound {abs(got - ref) / bound:.3f}")
    assert loss.dtype == F32 and abs(got - ref) <= bound, (got, ref, bound)
    dloss = torch.tensor([0.75], device="cuda")
    dp = Fx.mse_bwd(pred, tv, dloss)
    ref_d = 0.75 * 2.0 * d / B
    err = (dp.cpu().double() - ref_d).abs()
    assert dp.dtype == F32 and dp.shape == (B,) and bool((err <= 2 * U32 * ref_d.abs() + 2.0 ** -126).all()), float(err.max())
    assert torch.equal(pp.view(torch.int16 if dtype == BF16 else torch.int32), pb.view(torch.int16 if dtype == BF16 else torch.int32))
    assert torch.equal(tp, tb)
    # the autograd node: [B, 1] predictions as the head emits them, the upstream gradient stays on the device (no host read: a
    # synchronising call inside the region raises)
    head = cols[:, 1:2].clone().cuda().requires_grad_(True)
    tgt = target.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = small_mse(head, tgt)
        (out * 0.75).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out.shape == () and abs(float(out.detach()) - ref) <= bound
    assert head.grad.dtype == dtype and head.grad.shape == (B, 1)
    gerr = (head.grad.cpu().double().view(-1) - ref_d).abs()
    gbound = 2 * U32 * ref_d.abs() + 2.0 ** -126
    if dtype == BF16:
        gbound = gbound + 2.0 ** -8 * (ref_d.abs() + gbound)        # one bf16 rounding of a value within the fp32 bound
    assert bool((gerr <= gbound).all()), float((gerr / gbound).max())


# ---------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    z, meta = fixture()
    d = tmp_path_factory.mktemp("beit")
    vis = {k[len("vision_encoder."):]: v for k, v in state_from_spec({k: v for k, v in meta["spec"].items()
                                                                       if k.startswith("vision_encoder.")}).items()}
    vis["head.weight"], vis["head.bias"] = torch.zeros(1000, 768), torch.zeros(1000)
    torch.save({"model": vis}, os.path.join(d, "beit.pth"))
    vcfg = os.path.join(d, "config_beit2_base.json")
    with open(vcfg, "w") as f:
        json.dump({"ckpt": os.path.join(d, "beit.pth"), "vision_width": 768, "patch_size": 16}, f)
    shared = state_from_spec({k: v for k, v in meta["spec"].items() if not k.startswith("cls_head.3.")})   # one reference, left unchanged
    return z, meta, vcfg, shared


def _build(gold, task, train=True):
    """The fixture model of one run on the GPU, behind RCCLDDPAccelerator with the loop's optimizer and schedule.  Dropout and drop-path
    are off, as in the fixture (the reference model stayed in eval mode)."""
    from xfm_amd.accelerators import RCCLDDPAccelerator
    from xfm_amd.model_classification import XFMForClassification
    z, meta, vcfg, shared = gold
    cfg = loop_config(meta, task, vision_config=vcfg, text_config={"hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0})
    m = XFMForClassification(cfg)
    spec = run_spec(meta, task)
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()} == spec
    sd = dict(shared)
    sd.update(state_from_spec({k: v for k, v in spec.items() if k.startswith("cls_head.3.")}))
    m.load_state_dict(sd, strict=True)
    m.cuda()
    for blk in m.vision_encoder.blocks:
        blk.drop_path_prob = 0.0
    if not train:
        return cfg, m.finalize().eval(), None, None, None
    opt = GL.create_optimizer(cfg, m)
    names = {id(p): n for n, p in m.named_parameters()}
    assert [[names[id(p)] for p in g["params"]] for g in opt.param_groups] == meta["groups"]   # name for name, the whole model
    sch = GL.create_scheduler(cfg, opt, len(meta["runs"][task]["train_seeds"]))
    rec = {"loss": [], "sync": [], "lr_at": []}

    class Recording(RCCLDDPAccelerator):
        def backward_step(self, loss, optimizer, sync=None):
            rec["loss"].append(loss.detach())
            rec["sync"].append(sync)
            return super().backward_step(loss, optimizer, sync=sync)

        def optimizer_step(self, optimizer, model, grad_norm=0.0):
            rec["lr_at"].append([g["lr"] for g in optimizer.param_groups])
            return super().optimizer_step(optimizer, model, grad_norm)

    acc = Recording({"RNG_SEED": 3, "CLIP_GRAD_NORM": 0.0, "GRAD_ACCUMULATE_STEPS": 1})
    wrapped, opt, sch = acc.set_up(m, opt, sch, 0, 1, 0)
    return cfg, wrapped, opt, sch, (acc, rec)


def test_regression_branch_on_the_gpu_against_the_fixture(gold, monkeypatch):
    """model_classification.py:89-93 with num_labels == 1: the loss of the first training batch at the formula weights against the
    reference's, through xfm_mse_fwd; its backward through xfm_mse_bwd reaches the head (the output bias's gradient is mean 2 (p - t))."""
    import xfm_amd.model_classification as MC
    from xfm_amd.arena import grad_of
    z, meta = gold[0], gold[1]
    cfg, m, _, _, _ = _build(gold, "stsb", train=False)
    ids, atts, labels = (t.cuda() for t in train_batches(meta, "stsb")[0])
    calls = []
    real = MC.small_mse
    monkeypatch.setattr(MC, "small_mse", lambda p, t: (calls.append(tuple(p.shape)), real(p, t))[1])
    loss = m(None, ids, atts, labels, train=True)
    assert calls == [(meta["B"], 1)], "the regression loss did not go through small_mse"
    ref = float(z["stsb/loss"][0])
    print("stsb loss", float(loss), "reference", ref)
    assert abs(float(loss) - ref) <= LOSS_TOL * abs(ref), (float(loss), ref)
    loss.backward()
    with torch.no_grad():
        pred = m(None, ids, atts, labels, train=False)
    assert pred.shape == (meta["B"], 1)
    want = float((2.0 * (pred.float().view(-1) - labels)).mean())
    got = float(grad_of(getattr(m.cls_head, "3").bias).view(-1)[0])
    assert abs(got - want) <= 2e-2 * abs(want), (got, want)   # (the head's dgrad / wgrad GEMMs take the gradient in bf16: OUT_TOL)


@pytest.mark.parametrize("task", ["mrpc", "mnli", "stsb"])
def test_loop_on_the_gpu_against_the_reference(gold, task, monkeypatch):
    z, meta = gold[0], gold[1]
    R = meta["runs"][task]
    cfg, wrapped, opt, sch, (acc, rec) = _build(gold, task)
    dev = torch.device("cuda")
    reads = []
    real_read = GL._read
    monkeypatch.setattr(GL, "_read", lambda t: (reads.append(tuple(t.shape)), real_read(t))[1])
    stats, completed = GL.train_one_epoch(wrapped, train_batches(meta, task), opt, sch, 0, dev, cfg, acc, print_freq=1000)
    assert reads == []                                                    # train_one_epoch reads through the meters only, at log lines
    gas = R["gradient_accumulation_steps"]
    losses = [float(l) * gas for l in rec["loss"]]
    ref = z[f"{task}/loss"].tolist()
    print(task, "losses", losses, "reference", ref)
    assert completed == R["updates"] == 3 == len(rec["lr_at"])
    assert [i for i, s in enumerate(rec["sync"]) if s] == R["update_steps"]
    assert np.array_equal(np.asarray(rec["lr_at"]), z[f"{task}/lr_at"])
    assert [g["lr"] for g in opt.param_groups] == z[f"{task}/lr_after"][-1].tolist()
    for got, want in zip(losses, ref):
        assert abs(got - want) <= LOSS_TOL * abs(want), (losses, ref)
    assert abs(stats["loss"] - np.mean(ref)) <= LOSS_TOL * np.mean(ref)
    for tag in ["eval"] + (["eval_mm"] if task == "mnli" else []):
        seen = []
        hook = wrapped.module.register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().clone()))
        res = GL.evaluate(wrapped, eval_batches(meta, task, tag), dev, cfg)
        hook.remove()
        assert len(reads) == 1 and res.count == 12                         # ONE device read per pass
        reads.clear()
        logits = torch.cat(seen)
        _check_out(z, f"{task}/{tag}_logits", logits)
        ref_metric = R[tag]["metric"]
        if task == "stsb":
            labels = z[f"{task}/{tag}_labels"]
            preds = np.asarray(res.predictions)
            assert np.array_equal(preds.astype(np.float32), logits.view(-1).cpu().numpy())
            own = correlations_restated(preds, labels)                     # the kernel against fp64 on the GPU's own predictions
            assert abs(res["pearson"] - own[0]) <= CORR_TOL and abs(res["spearmanr"] - own[1]) <= CORR_TOL
            # no tolerance is set on GPU-versus-reference correlations: how a bf16 step moves a 12-row correlation is not measured
            print(task, tag, "pearson", res["pearson"], "reference", ref_metric["pearson"], "spearmanr", res["spearmanr"], "reference",
                  ref_metric["spearmanr"])
        else:
            assert R[tag]["margin"] > R[tag]["bound"] > 0
            assert list(res.predictions) == z[f"{task}/{tag}_preds"].tolist()
            assert dict(res) == ref_metric, (dict(res), ref_metric)
            assert list(res.predictions) == logits.argmax(dim=-1).tolist()


def test_run_glue_script_main_trains_evaluates_and_checkpoints(gold, tmp_path, capsys):
    """run_glue.py's main() as `run.py --task glue` starts it, at the fixture's shallow shape with synthetic loaders and no `vision_config`:
    one epoch of three iterations with accumulation, the evaluation, log.txt and the checkpoint; then the `--evaluate` form."""
    from types import SimpleNamespace as NS

    import run_glue as script
    meta = gold[1]

    def config(task):
        return loop_config(meta, task, synthetic=True, train_dataset_size=12, val_dataset_size=8, print_freq=1, gradient_accumulation_steps=2,
                           text_config={"vocab_size": 2048})

    out = tmp_path / "glue"
    out.mkdir()
    args = NS(checkpoint="", seed=42, evaluate=False, output_dir=str(out))
    script.main(args, config("stsb"))
    capsys.readouterr()
    line = json.loads((out / "log.txt").read_text())
    assert line["epoch"] == 0 and line["completed_steps"] == 2 and set(line) >= {"train_loss", "eval_pearson", "eval_spearmanr"}
    ckpt = torch.load(out / "model_state_epoch_0.th", weights_only=False)
    assert sorted(ckpt) == ["config", "model"] and ckpt["config"]["num_labels"] == 1 and isinstance(ckpt["model"], dict)
    args.evaluate = True
    script.main(args, config("mrpc"))
    records = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(records) == 1 and set(records[0]) == {"accuracy", "f1", "count"} and records[0]["count"] == 8
    assert 0.0 <= records[0]["accuracy"] <= 1.0 and math.isfinite(records[0]["f1"])
