"""The ImageNet fine-tune / linear-probe loop on a real MI355X: xfm_adamw_torch against torch.optim.AdamW, xfm_ce_topk_eval against
torch, the accelerator's rule selection (fine-tune and linear probe), and xfm_amd.imagenet_loop against the reference's loop
(tests/golden/imagenet_loop_small.npz).  Tolerances are taken from the existing tests of the neighbouring kernels:
  AdamW   max err / max|ref| <= 1e-4  (tests/test_hip_kernels.py::test_adamw_and_sumsq_flat_arena)
  CE rows max err / max|ref| <= 1e-5  (tests/test_hip_kernels.py, xfm_ce_fwd's `loss rows`)
  losses of the bf16 model against the fp32 reference: 2e-3 relative (tests/test_hip_modules.py on classification_imagenet.npz)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from imagenet_loop_util import eval_batch, fixture, loop_config, train_batches, used_state  # noqa: E402
from xfm_amd import imagenet_loop as IL  # noqa: E402

F32 = torch.float32
ADAMW_TOL, CE_TOL, LOSS_TOL = 1e-4, 1e-5, 2e-3


def _fx():
    from xfm_amd import functional as Fx
    return Fx


def _close(got, ref, tol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    denom = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max()) / denom
    assert err <= tol, f"{what}: max err / max|ref| = {err:.3e} > {tol}"


def _rand(shape, scale, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------- AdamW
def _groups(n):
    """Two groups with a boundary in the middle of the arena (group ids are per 256-element block)."""
    blocks = n // 256
    gid = torch.zeros(blocks, dtype=torch.uint8)
    gid[blocks // 2:] = 1
    return gid


def _torch_adamw(p0, grads, steps, lrs, wds, betas, eps, gid, clip):
    """torch.optim.AdamW itself on the CPU, fp32, `grads[i]` at step number `steps[i]` (the step count is injected into its state)."""
    mask = gid.repeat_interleave(256) == 0
    parts = [(p0[s].clone().requires_grad_(True), s, gi) for gi, s in enumerate((mask, ~mask)) if int(s.sum())]
    opt = torch.optim.AdamW([{"params": [q], "lr": lrs[gi], "weight_decay": wds[gi]} for q, _, gi in parts], betas=betas, eps=eps)
    for g, step in zip(grads, steps):
        for q, s, _ in parts:
            q.grad = (g[s] * (clip if clip is not None else 1.0)).clone()
            st = opt.state[q]
            if not st:
                st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(q), torch.zeros_like(q)
            st["step"] = torch.tensor(float(step - 1))
        opt.step()
    out_p, out_m, out_v = torch.empty_like(p0), torch.empty_like(p0), torch.empty_like(p0)
    for q, s, _ in parts:
        out_p[s], out_m[s], out_v[s] = q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    return out_p, out_m, out_v


def _transformers_adamw(p0, g, step, lrs, wds, betas, eps, gid):
    """The rule xfm_adamw runs (transformers.optimization.AdamW, as replayed in tests/test_hip_accelerator.py), one step from zero moments."""
    b1, b2 = betas
    lr = torch.tensor(lrs)[gid.long()].repeat_interleave(256)
    wd = torch.tensor(wds)[gid.long()].repeat_interleave(256)
    m = (1 - b1) * g
    v = (1 - b2) * g * g
    p = p0 - lr * (1 - b2 ** step) ** 0.5 / (1 - b1 ** step) * m / (v.sqrt() + eps)
    return p - lr * wd * p, m, v


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("n", [256, 1280, 256 * 4097])   # one block; a group boundary inside a few blocks; past the 4096-workgroup grid cap
def test_adamw_torch_matches_torch_optim_adamw(n, clip, zero_grad):
    Fx = _fx()
    lrs, wds, betas, eps = [1e-3, 3e-3], [0.01, 0.2], (0.9, 0.999), 1e-8
    gid = _groups(n)
    p0 = _rand((n,), 1.0, 1)
    steps = (1, 2, 1000)   # bc1 / bc2 near 0 and near 1
    grads = [_rand((n,), 0.1, 10 + i) for i in range(3)]
    p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    clip_t = None if clip is None else torch.tensor([clip], device="cuda")
    for g, step in zip(grads, steps):
        gd = g.clone().cuda()
        Fx.adamw(p, gd, m, v, gid.cuda(), lrs, wds, *betas, eps, step, clip_t, zero_grad=bool(zero_grad), rule="torch")
        assert float(gd.abs().max()) == 0.0 if zero_grad else torch.equal(gd.cpu(), g)
    rp, rm, rv = _torch_adamw(p0, grads, steps, lrs, wds, betas, eps, gid, clip)
    _close(p, rp, ADAMW_TOL, "p")
    _close(m, rm, ADAMW_TOL, "exp_avg")
    _close(v, rv, ADAMW_TOL, "exp_avg_sq")


def test_adamw_torch_is_not_the_transformers_rule():
    """Inputs on which the two rules are far apart (eps comparable to |g|, large lr and decay, step 1): the CPU results of the two rules
    differ by more than 100 x the tolerance, so a fall back to xfm_adamw cannot pass; xfm_adamw itself still equals ITS rule."""
    Fx = _fx()
    n = 1280
    lrs, wds, betas, eps = [0.1, 0.05], [0.1, 0.0], (0.9, 0.999), 1e-3
    gid = _groups(n)
    p0, g = _rand((n,), 1.0, 21), _rand((n,), 1e-3, 22)
    tp, tm, tv = _torch_adamw(p0, [g], (1,), lrs, wds, betas, eps, gid, None)
    hp, hm, hv = _transformers_adamw(p0, g, 1, lrs, wds, betas, eps, gid)
    apart = float((tp - hp).abs().max()) / float(tp.abs().max())
    assert apart > 100 * ADAMW_TOL, apart
    for rule, (rp, rm, rv) in (("torch", (tp, tm, tv)), ("transformers", (hp, hm, hv))):
        p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        Fx.adamw(p, g.clone().cuda(), m, v, gid.cuda(), lrs, wds, *betas, eps, 1, None, rule=rule)
        _close(p, rp, ADAMW_TOL, rule + " p")
        _close(m, rm, ADAMW_TOL, rule + " m")
        _close(v, rv, ADAMW_TOL, rule + " v")


# ---------------------------------------------------------------------------------------------------------------- evaluation kernel
TOPK_SHAPES = [(1, 2, 2), (3, 10, 10), (5, 37, 37), (7, 1000, 1000), (130, 1000, 1024), (2, 397, 400)]


def _topk_case(R, V, ld, unaligned=False):
    """Logits over +-30 with the padding columns poisoned; labels by row: column 0, column V - 1, the row maximum, an exact tie with a
    LOWER column, an exact tie with a HIGHER column, then repeating."""
    g = torch.Generator().manual_seed(1000 * R + V)
    x = (torch.rand((R, V), generator=g) * 60.0 - 30.0)
    labels = torch.zeros(R, dtype=torch.int64)
    for r in range(R):
        kind = r % 5
        if kind == 0:
            labels[r] = 0
        elif kind == 1:
            labels[r] = V - 1
        elif kind == 2:
            labels[r] = int(x[r].argmax())
        elif kind == 3:   # the tied lower column is ahead of the label
            labels[r] = V - 1 - (r % max(V - 1, 1)) if V > 1 else 0
            if labels[r] > 0:
                x[r, int(labels[r]) // 2] = x[r, labels[r]]
        else:             # the tied higher column is behind it
            labels[r] = (r % max(V - 1, 1)) if V > 1 else 0
            if labels[r] < V - 1:
                x[r, (int(labels[r]) + V) // 2] = x[r, labels[r]]
    rows = R + 1 if unaligned else R
    buf = torch.full((rows, ld), 1e9)
    dev = buf.cuda()
    view = dev[1:] if unaligned else dev
    view[:, :V] = x.cuda()
    return x, labels, view


def _topk_reference(x, labels):
    rows = torch.nn.functional.cross_entropy(x, labels, reduction="none")
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    rank = (order == labels.view(-1, 1)).int().argmax(dim=1).int()
    return rows, rank


def _check_topk(R, V, ld, k1, k2, unaligned=False):
    Fx = _fx()
    x, labels, dev = _topk_case(R, V, ld, unaligned)
    if unaligned:
        assert dev.data_ptr() % 16 != 0 and ld % 2 == 1
    ref_rows, ref_rank = _topk_reference(x, labels)
    acc = torch.zeros(3, device="cuda")
    rows, rank = Fx.ce_topk_eval(dev, V, labels.cuda(), k1, k2, acc)
    _close(rows, ref_rows, CE_TOL, "row_loss")
    assert torch.equal(rank.cpu(), ref_rank), (rank.cpu().tolist(), ref_rank.tolist())
    once = acc.clone()
    assert once[1].item() == float((ref_rank < k1).sum()) and once[2].item() == float((ref_rank < k2).sum())
    assert abs(once[0].item() - float(ref_rows.double().sum())) <= CE_TOL * max(float(ref_rows.abs().max()), 1e-6) * R
    Fx.ce_topk_eval(dev, V, labels.cuda(), k1, k2, acc)            # acc accumulates: a second call doubles it exactly
    assert torch.equal(acc, once * 2)
    again = torch.zeros(3, device="cuda")                          # two runs are bit-identical
    rows2, rank2 = Fx.ce_topk_eval(dev, V, labels.cuda(), k1, k2, again)
    assert torch.equal(again, once) and torch.equal(rows2, rows) and torch.equal(rank2, rank)
    solo = torch.zeros(3, device="cuda")                           # row_loss = row_rank = NULL: same sums, same bits
    assert Fx.ce_topk_eval(dev, V, labels.cuda(), k1, k2, solo, rows=False) is None
    assert torch.equal(solo, once)
    assert float(dev[:, V:].min()) == 1e9 if ld > V else True      # the padding was only ever skipped


@pytest.mark.parametrize("k1,k2", [(1, 2), (1, 5)])
@pytest.mark.parametrize("R,V,ld", TOPK_SHAPES)
def test_ce_topk_eval_matches_torch(R, V, ld, k1, k2):
    if k2 > V:   # (1, 2, 2) with k2 = 5: an argument error, reported and not launched
        from xfm_amd._lib import XfmHipError
        acc = torch.zeros(3, device="cuda")
        with pytest.raises(XfmHipError, match="ce_topk_eval"):
            _fx().ce_topk_eval(torch.zeros((R, ld), device="cuda"), V, torch.zeros(R, dtype=torch.int64, device="cuda"), k1, k2, acc)
        assert acc.tolist() == [0.0, 0.0, 0.0]
        return
    _check_topk(R, V, ld, k1, k2)


def test_ce_topk_eval_unaligned_base_and_odd_stride():
    _check_topk(4, 37, 37, 1, 2, unaligned=True)
    _check_topk(6, 1000, 1001, 1, 5, unaligned=True)


def test_ce_topk_eval_tie_rule_and_foreign_labels():
    Fx = _fx()
    x = torch.tensor([[1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 0.0], [0.0, 2.0, 2.0, 2.0], [5.0, 1.0, 1.0, 1.0]]).cuda()
    labels = torch.tensor([0, 2, 1, 7]).cuda()   # the last one is outside [0, V): rank V, loss 0, nothing added
    acc = torch.zeros(3, device="cuda")
    rows, rank = Fx.ce_topk_eval(x, 4, labels, 1, 2, acc)
    assert rank.tolist() == [0, 2, 0, 4] and rows[3].item() == 0.0
    assert acc[1:].tolist() == [2.0, 2.0]
    assert acc[0].item() == pytest.approx(float(rows[:3].sum()), rel=1e-6)
    with pytest.raises(ValueError):   # host labels are checked by the wrapper
        Fx.ce_topk_eval(x, 4, torch.tensor([0, 2, 1, 7]), 1, 2, acc)


def test_ce_topk_eval_argument_errors_launch_nothing():
    from xfm_amd import _lib
    lib = _lib.load()
    x = torch.zeros((2, 10), device="cuda")
    labels = torch.zeros(2, dtype=torch.int64, device="cuda")
    acc = torch.full((3,), 7.0, device="cuda")
    for bad in (dict(k1=0), dict(k1=3, k2=2), dict(k2=11), dict(ld=9), dict(R=0)):
        kw = dict(ld=10, R=2, V=10, k1=1, k2=2)
        kw.update(bad)
        rc = lib.xfm_ce_topk_eval(x.data_ptr(), kw["ld"], kw["R"], kw["V"], labels.data_ptr(), kw["k1"], kw["k2"], None, None, acc.data_ptr(),
                                  None)
        assert rc == -1, bad
    torch.cuda.synchronize()
    assert acc.tolist() == [7.0, 7.0, 7.0]


# ---------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    z, meta = fixture()
    sd = used_state(meta["spec"])
    d = tmp_path_factory.mktemp("beit")
    vis = {k[len("vision_encoder."):]: v for k, v in sd.items() if k.startswith("vision_encoder.")}
    vis["head.weight"], vis["head.bias"] = torch.zeros(1000, 768), torch.zeros(1000)
    torch.save({"model": vis}, os.path.join(d, "beit.pth"))
    vcfg = os.path.join(d, "config_beit2_base.json")
    with open(vcfg, "w") as f:
        json.dump({"ckpt": os.path.join(d, "beit.pth"), "vision_width": 768, "patch_size": 16}, f)
    return z, meta, sd, vcfg


def _build(gold, is_lp, record=None):
    """The fixture model on the GPU behind RCCLDDPAccelerator with the marked optimizer.  The text towers (unused by this branch, never
    live) are built at zero depth with a small vocabulary; drop-path is off, as in the fixture."""
    from xfm_amd.accelerators import RCCLDDPAccelerator
    from xfm_amd.model_classification import XFMForClassification
    z, meta, sd, vcfg = gold

    class Recording(RCCLDDPAccelerator):
        def backward_step(self, loss, optimizer, sync=None):
            if record is not None:
                record["loss"].append(loss.detach())
            return super().backward_step(loss, optimizer, sync=sync)

        def optimizer_step(self, optimizer, model, grad_norm=0.0):
            if record is not None:
                self.arena.reattach()
                self.grads_ready()
                record["step"].append((self.arena.grad.clone(), list(self.arena.live), optimizer.param_groups[0]["lr"]))
            return super().optimizer_step(optimizer, model, grad_norm)

    cfg = loop_config(meta, is_lp, vision_config=vcfg, text_num_hidden_layers=0, text_fusion_start_at=0, fusion_num_hidden_layers=0,
                      text_config={"vocab_size": 2048})
    m = XFMForClassification(cfg)
    missing = m.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.startswith(("text_encoder.", "fusion_encoder.")) for k in missing.missing_keys)
    m.cuda()
    opt = IL.create_optimizer(cfg, m)
    acc = Recording({"RNG_SEED": 3, "CLIP_GRAD_NORM": 0.0, "GRAD_ACCUMULATE_STEPS": 1})
    wrapped, opt, _ = acc.set_up(m, opt, None, 0, 1, 0)
    for blk in m.vision_encoder.blocks:
        blk.drop_path_prob = 0.0
    return cfg, m, wrapped, opt, acc


def _step(cfg, wrapped, m, opt, acc, criterion, batch, epoch):
    IL.adjust_learning_rate(opt, epoch, cfg)
    images, target = (t.cuda() for t in batch)
    loss = criterion(wrapped(images, None, None, None, False), target)
    opt.zero_grad()
    acc.backward_step(loss, opt)
    acc.optimizer_step(opt, m)


def _replay(named, arena, ref_params, ref_opt, grad, live, lr):
    for g in ref_opt.param_groups:
        g["lr"] = lr
    for (n, p), q in zip(named, ref_params):
        o, n_el = arena.offsets[id(p)]
        q.grad = grad[o:o + n_el].view(p.shape).cpu().clone() if live[arena._unit_of[id(p)]] else None
    ref_opt.step()


def test_accelerator_fine_tune_steps_with_the_torch_rule(gold):
    z, meta = gold[0], gold[1]
    rec = {"loss": [], "step": []}
    cfg, m, wrapped, opt, acc = _build(gold, False, rec)
    m.train()
    criterion = IL.create_criterion(cfg, None)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert [id(p) for _, p in named] == [id(p) for p in opt.param_groups[0]["params"]]
    ref_params = [p.detach().cpu().clone().requires_grad_(True) for _, p in named]
    ref_opt = torch.optim.AdamW(ref_params, lr=1.0)
    batches = train_batches(meta)
    arena = m._arena

    def compare(what):
        torch.cuda.synchronize()
        bad = []
        for (n, p), q in zip(named, ref_params):
            st = ref_opt.state.get(q)
            if not st:
                assert not arena.is_live(p), n
                assert torch.equal(p.detach().cpu(), q.detach()), f"{n}: a parameter without a gradient moved"
                continue
            mm, vv = acc._views(p)
            for got, ref, tag in ((p.detach(), q.detach(), "p"), (mm, st["exp_avg"], "m"), (vv, st["exp_avg_sq"], "v")):
                err = float((got.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
                if err > ADAMW_TOL:
                    bad.append((n, tag, f"{err:.2e}"))
        assert not bad, f"{what}: {bad[:8]}"

    for k, epoch in enumerate((0.5, 1.0)):
        _step(cfg, wrapped, m, opt, acc, criterion, batches[k], epoch)
        _replay(named, arena, ref_params, ref_opt, *rec["step"][-1])
        compare(f"step {k + 1}")
    live = [n for n, p in named if arena.is_live(p)]
    assert len(live) == meta["stepped_ft"] and any(n.startswith("vision_encoder.") for n in live)
    # optimizer.state_dict() (published in torch's format) -> a fresh torch.optim.AdamW -> one more step
    sd = opt.state_dict()
    assert len(sd["state"]) == meta["stepped_ft"] and sd["param_groups"][0]["adamw_rule"] == "torch"
    fresh_params = [p.detach().cpu().clone().requires_grad_(True) for _, p in named]
    fresh = torch.optim.AdamW(fresh_params, lr=1.0)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["weight_decay"] == 0.01 and tuple(fresh.param_groups[0]["betas"]) == (0.9, 0.999)
    _step(cfg, wrapped, m, opt, acc, criterion, batches[0], 1.5)
    _replay(named, arena, fresh_params, fresh, *rec["step"][-1])
    ref_params[:], ref_opt = fresh_params, fresh
    compare("step 3 from the loaded state")
    assert all(int(fresh.state[q]["step"]) == 3 for q in fresh_params if fresh.state.get(q))


def test_accelerator_linear_probe_leaves_the_tower_alone(gold):
    z, meta = gold[0], gold[1]
    cfg, m, wrapped, opt, acc = _build(gold, True)
    m.train()
    criterion = IL.create_criterion(cfg, None)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    batches = train_batches(meta)
    for k, epoch in enumerate((0.5, 1.0)):
        _step(cfg, wrapped, m, opt, acc, criterion, batches[k], epoch)
    torch.cuda.synchronize()
    arena = m._arena
    tower = [(n, p) for n, p in m.named_parameters() if n.startswith("vision_encoder.")]
    assert len(tower) > 20 and all(any(p is q for q in opt.param_groups[0]["params"]) for _, p in tower if p.requires_grad)
    for n, p in tower:   # in the optimizer, never a gradient: untouched, weight decay included, and no moments
        assert torch.equal(p.detach(), before[n]), f"{n} moved in a linear probe"
        assert not arena.is_live(p)
        mm, vv = acc._views(p)
        assert float(mm.abs().max()) == 0.0 and float(vv.abs().max()) == 0.0
    head = [(n, p) for n, p in m.named_parameters() if n.startswith("cls_head.")]
    assert all(float((p.detach() - before[n]).abs().max()) > 0 for n, p in head)
    sd = opt.state_dict()
    names = {id(p): n for n, p in m.named_parameters()}
    stepped = {names[id(p)] for p in opt.param_groups[0]["params"] if p in opt.state}
    assert stepped == set(meta["stepped_lp"]) and len(sd["state"]) == len(stepped)


@pytest.mark.parametrize("is_lp", [False, True])
def test_loop_on_the_gpu_against_the_reference(gold, is_lp):
    z, meta = gold[0], gold[1]
    pre = "lp" if is_lp else "ft"
    rec = {"loss": [], "step": []}
    cfg, m, wrapped, opt, acc = _build(gold, is_lp, rec)
    criterion = IL.create_criterion(cfg, IL.create_mixup(cfg))
    loader = train_batches(meta)
    for epoch in range(cfg["schedular"]["epochs"]):
        IL.train_one_epoch(wrapped, loader, opt, criterion, epoch, None, torch.device("cuda"), cfg, acc)
    assert [s[2] for s in rec["step"]] == z[f"{pre}/lr"].tolist()
    losses = [float(l) for l in rec["loss"]]
    ref = z[f"{pre}/loss"].tolist()
    print(pre, "losses", losses, "reference", ref)
    images, target = eval_batch(meta)
    res = IL.evaluate(wrapped, [(images[:4], target[:4]), (images[4:], target[4:])], torch.device("cuda"), log=lambda s: None)
    print(pre, "eval", res.loss_avg, res.acc1, res.acc2, "reference", float(z[f"{pre}/eval_loss"]), z[f"{pre}/acc"].tolist())
    for got, want in zip(losses, ref):
        assert abs(got - want) <= LOSS_TOL * abs(want), (losses, ref)
    assert abs(res.loss_avg - float(z[f"{pre}/eval_loss"])) <= LOSS_TOL * float(z[f"{pre}/eval_loss"])
    n = meta["eval_B"]
    assert round(res.acc1 * n / 100) == round(float(z[f"{pre}/acc"][0]) * n / 100)
    assert round(res.acc2 * n / 100) == round(float(z[f"{pre}/acc"][1]) * n / 100)


def test_evaluate_reads_the_device_once(gold, monkeypatch):
    z, meta = gold[0], gold[1]
    cfg, m, wrapped, opt, acc = _build(gold, True)
    images, target = eval_batch(meta)
    loader = [(images[0:2], target[0:2]), (images[2:4], target[2:4]), (images[4:6], target[4:6])]
    reads, seen = [], []
    real = IL._read
    monkeypatch.setattr(IL, "_read", lambda t: (reads.append(tuple(t.shape)), real(t))[1])
    hook = m.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
    res = IL.evaluate(wrapped, loader, torch.device("cuda"), log=lambda s: None)
    hook.remove()
    assert reads == [(3,)] and len(seen) == 3
    loss_sum, n1, n2 = 0.0, 0, 0
    for logits, (_, t) in zip(seen, loader):   # the per-batch torch form of Imagenet.py:517-523 on the same logits
        lg = logits.float().cpu()
        loss_sum += float(torch.nn.functional.cross_entropy(lg, t)) * t.numel()
        top = lg.topk(2, 1, True, True).indices
        n1 += int((top[:, 0] == t).sum())
        n2 += int((top == t.view(-1, 1)).any(1).sum())
    assert res.count == 6 and res.acc1 == 100.0 * n1 / 6 and res.acc2 == 100.0 * n2 / 6 and float(res) == res.acc1
    assert abs(res.loss_avg - loss_sum / 6) <= 1e-5 * abs(loss_sum / 6)
    a1, a2 = IL.accuracy(torch.cat(seen).float(), target.cuda(), topk=(1, 2))   # the kernel path of accuracy(): percent, one element each
    assert a1.shape == (1,) and float(a1) == pytest.approx(res.acc1) and float(a2) == pytest.approx(res.acc2)


# ------------------------------------------------------------------------------------------------------------- script
@pytest.mark.parametrize("is_lp", [False, True])
def test_imagenet_script_main_trains_saves_the_best_checkpoint_and_evaluates(gold, is_lp, tmp_path, capsys):
    """Imagenet.py's main() as `run.py --task imagenet` starts it, at the fixture's shallow shape with synthetic loaders and no
    `vision_config` (a random-init tower written next to the outputs): one epoch of two iterations, the validation pass,
    checkpoint_best.pth and log.txt; then the `--evaluate` form on a fresh model."""
    from types import SimpleNamespace as NS

    import Imagenet as script
    from xfm_amd import synthetic as syn
    meta = gold[1]

    def config():
        cfg = loop_config(meta, is_lp, synthetic=True, batch_size_train=4, batch_size_test=8, train_dataset_size=8, val_dataset_size=32,
                          print_freq=1, text_num_hidden_layers=0, text_fusion_start_at=0, fusion_num_hidden_layers=0,
                          text_config={"vocab_size": 2048})
        cfg["schedular"]["epochs"] = 1
        return cfg

    # the reference saves when acc1 > best_acc1 with best_acc1 = 0 (Imagenet.py:614-625): take the first seed whose validation labels cover
    # every class, so that even a constant prediction scores (tests/test_imagenet_loop_host.py does the same)
    seed = next(s for s in range(42, 400) if len({int(v) for k in range(4) for v in
                                                  syn.imagenet_batch(8, seed=s + 104729 + 7919 * k, image_res=16, num_labels=meta["num_labels"])[1]})
                == meta["num_labels"])
    out = tmp_path / "imagenet"
    out.mkdir()
    args = NS(checkpoint="", seed=seed, evaluate=False, output_dir=str(out))
    script.main(args, config())
    capsys.readouterr()
    ckpt = torch.load(out / "checkpoint_best.pth", weights_only=False)
    assert sorted(ckpt) == ["config", "epoch", "model", "optimizer"]
    assert ckpt["optimizer"]["param_groups"][0]["adamw_rule"] == "torch" and bool(ckpt["config"]["is_lp"]) == is_lp
    assert (out / "log.txt").read_text().endswith("best epoch: %d" % ckpt["epoch"])
    args.evaluate = True
    script.main(args, config())
    records = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(records) == 1 and sorted(records[0]) == ["acc1", "acc2", "loss"]
    assert all(np.isfinite(records[0][k]) for k in ("acc1", "acc2", "loss")), records
    assert 0.0 <= records[0]["acc1"] <= records[0]["acc2"] <= 100.0
