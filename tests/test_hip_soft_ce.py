"""Soft-target / label-smoothed cross-entropy and the device Mixup on a real MI355X: the C-ABI entry points xfm_ce_smooth_*, xfm_ce_soft_*,
xfm_mixup, xfm_mixup_target, the modules over them (losses.SoftTargetCrossEntropy / LabelSmoothingCrossEntropy, mixup.Mixup) and the
ImageNet fine-tune step they stand for (Imagenet.py:468-469, 592-609).  References: torch.nn.functional.cross_entropy / log_softmax
in fp32.  Bounds, those of the existing CE kernel tests: loss within 1e-5 relative, dlogits by _close(..., 1e-2) (bf16 output), padding
columns and ignored rows exactly 0."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_kernels import _close, _fx, _rand

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(37, 50265, 50304), (23, 1000, 1024), (5, 1001, 1004), (3, 2, 2), (1, 7, 8)]
S = 0.1


@functools.lru_cache(maxsize=None)
def _case(R, V, ld):
    """Shared per shape and left unchanged: logits with 1e9 in the padding columns, labels with -100 on a stride, second labels (some
    rows equal to the first), per-row lam in {0, 0.3, 1}, per-row upstream gradients."""
    logits = torch.full((R, ld), 1e9, dtype=F32, device="cuda")
    logits[:, :V] = _rand((R, V), 2.0, F32, seed=200 + R)
    g = torch.Generator().manual_seed(R)
    labels = torch.randint(0, V, (R,), generator=g).cuda()
    labels[2::3] = -100
    labels_b = torch.randint(0, V, (R,), generator=g).cuda()
    labels_b[1::4] = labels[1::4].clamp(min=0)   # a == b
    lam = torch.tensor([0.0, 0.3, 1.0], dtype=F32)[torch.randint(0, 3, (R,), generator=g)].cuda().contiguous()
    w = _rand((R,), 1.0, F32, seed=300 + R).contiguous()
    return logits, labels, labels_b, lam, w


def _scales(labels, w):
    nvalid = (labels != -100).sum().clamp(min=1).float()
    return [("scale[0]", (1.0 / nvalid).reshape(1)), ("scale[row]", w)]


def _check_rows(got_rows, ref_rows, what):
    print(f"{what}: loss rows max err / max|ref| = {float((got_rows - ref_rows).abs().max()) / max(float(ref_rows.abs().max()), 1e-6):.3e}")
    _close(got_rows, ref_rows, 1e-5, what + " loss rows")
    got, ref = float(got_rows.sum()), float(ref_rows.sum())
    assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (what, got, ref)


def _check_dlogits(d, ref_grad, V, ignored, what):
    _close(d[:, :V], ref_grad, 1e-2, what + " dlogits")
    if d.shape[1] > V:
        assert float(d[:, V:].float().abs().max()) == 0.0, what + ": padding columns"
    if bool(ignored.any()):
        assert float(d[ignored].float().abs().max()) == 0.0, what + ": ignored rows"


def _dense_target(labels_a, labels_b, lam, V, on, off):
    """t = off + (on - off) (lam onehot(a) + (1 - lam) onehot(b)); rows of ignored labels are zero."""
    a, b = labels_a.clamp(min=0), labels_b.clamp(min=0)
    t = torch.full((labels_a.numel(), V), off, dtype=F32, device="cuda")
    t.scatter_add_(1, a[:, None], ((on - off) * lam)[:, None])
    t.scatter_add_(1, b[:, None], ((on - off) * (1 - lam))[:, None])
    return t * (labels_a != -100)[:, None]


def _v1_rows(x, label, s):
    """LabelSmoothSoftmaxCEV1.forward (xbert.py:1210-1223) with reduction 'none', written out."""
    ignore = label.eq(-100)
    label = label.clone()
    label[ignore] = 0
    lb_pos, lb_neg = 1. - s, s / x.size(1)
    lb_one_hot = torch.empty_like(x.detach()).fill_(lb_neg).scatter_(1, label.unsqueeze(1), lb_pos)
    loss = -torch.sum(torch.log_softmax(x, dim=1) * lb_one_hot, dim=1)
    return loss.masked_fill(ignore, 0.0)


def _label_case(shape, on, off, ref_rows_fn, what, two_labels=False):
    Fx = _fx()
    R, V, ld = shape
    logits, labels, labels_b, lam, w = _case(*shape)
    kw = dict(labels_b=labels_b, lam=lam) if two_labels else {}
    ldd = (ld + 7) // 8 * 8
    lse, rows = Fx.ce_smooth_fwd(logits, V, labels, on, off, **kw)
    xr = logits[:, :V].clone().requires_grad_(True)
    ref_rows = ref_rows_fn(xr)
    _check_rows(rows, ref_rows.detach(), what)
    _close(lse, torch.logsumexp(xr.detach(), 1), 1e-5, what + " lse")
    for name, scale in _scales(labels, w):
        d = Fx.ce_smooth_bwd(logits, V, labels, on, off, lse, scale.contiguous(), ldd, **kw)
        ref_grad, = torch.autograd.grad((ref_rows * scale).sum(), xr, retain_graph=True)
        _check_dlogits(d, ref_grad, V, labels == -100, f"{what} {name}")


@pytest.mark.parametrize("shape", SHAPES)
def test_label_form_one_hot_reproduces_the_plain_ce_kernels(shape):
    """on = 1, off = 0, lam = NULL against xfm_ce_fwd/bwd on the same inputs; lam in {0, 1} with two labels likewise."""
    Fx = _fx()
    R, V, ld = shape
    logits, labels, labels_b, lam, w = _case(*shape)
    ldd = (ld + 7) // 8 * 8
    lse0, rows0 = Fx.ce_fwd(logits, V, labels)
    lse, rows = Fx.ce_smooth_fwd(logits, V, labels, 1.0, 0.0)
    _check_rows(rows, rows0, "one-hot")
    _close(lse, lse0, 1e-5, "lse")
    ones = torch.ones(R, dtype=F32, device="cuda")
    other = labels_b.masked_fill(labels == -100, 0)
    # lam = 1 puts everything on a (b is any other valid label), lam = 0 everything on b (= the plain kernel's label, a is any valid one)
    lse1, rows1 = Fx.ce_smooth_fwd(logits, V, labels, 1.0, 0.0, labels_b=other, lam=ones)
    valid_a = labels_b.masked_fill(labels == -100, -100)
    lse2, rows2 = Fx.ce_smooth_fwd(logits, V, valid_a, 1.0, 0.0, labels_b=labels.clamp(min=0), lam=1 - ones)
    _check_rows(rows1, rows0, "lam = 1")
    _check_rows(rows2, rows0, "lam = 0")
    for name, scale in _scales(labels, w):
        scale = scale.contiguous()
        d0 = Fx.ce_bwd(logits, V, labels, lse0, scale, ldd)
        for what, d in (("NULL", Fx.ce_smooth_bwd(logits, V, labels, 1.0, 0.0, lse, scale, ldd)),
                        ("lam = 1", Fx.ce_smooth_bwd(logits, V, labels, 1.0, 0.0, lse1, scale, ldd, labels_b=other, lam=ones)),
                        ("lam = 0", Fx.ce_smooth_bwd(logits, V, valid_a, 1.0, 0.0, lse2, scale, ldd, labels_b=labels.clamp(min=0), lam=1 - ones))):
            _check_dlogits(d, d0.float()[:, :V], V, labels == -100, f"{what} {name}")


@pytest.mark.parametrize("shape", SHAPES)
def test_label_form_torch_convention(shape):
    V = shape[1]
    labels = _case(*shape)[1]
    _label_case(shape, 1.0 - S + S / V, S / V,
                lambda x: F.cross_entropy(x, labels, ignore_index=-100, reduction="none", label_smoothing=S), "torch smoothing")


@pytest.mark.parametrize("shape", SHAPES)
def test_label_form_v1_convention(shape):
    V = shape[1]
    labels = _case(*shape)[1]
    _label_case(shape, 1.0 - S, S / V, lambda x: _v1_rows(x, labels, S), "V1 smoothing")


@pytest.mark.parametrize("shape", SHAPES)
def test_label_form_two_labels_with_per_row_lam(shape):
    """lam in {0, 0.3, 1} per row, some rows with a == b, against the dense torch soft-target CE of the materialised rows; a == b must
    give what lam = 1 gives."""
    Fx = _fx()
    R, V, ld = shape
    logits, labels, labels_b, lam, w = _case(*shape)
    on, off = 1.0 - S + S / V, S / V
    t = _dense_target(labels, labels_b, lam, V, on, off)
    _label_case(shape, on, off, lambda x: F.cross_entropy(x, t, reduction="none"), "two labels", two_labels=True)
    same = labels.clamp(min=0)
    _, rows_same = Fx.ce_smooth_fwd(logits, V, labels, on, off, labels_b=same, lam=lam)
    _, rows_one = Fx.ce_smooth_fwd(logits, V, labels, on, off)
    _close(rows_same, rows_one, 1e-6, "a == b against lam = 1")


@pytest.mark.parametrize("shape", SHAPES)
def test_dense_form(shape):
    """Targets: rows of xfm_mixup_target (normalised: F.cross_entropy with probabilities), random non-negative rows that do not sum to 1
    and an all-zero row (-sum t log_softmax written out; the zero row has loss 0 and gradient exactly 0).  The target's padding
    columns hold 1e9 as the logits' do."""
    Fx = _fx()
    R, V, ld = shape
    logits, labels, labels_b, lam, w = _case(*shape)
    ldd = (ld + 7) // 8 * 8
    y = labels.clamp(min=0)
    mixed = Fx.mixup_target(y, lam, V, S)
    on, off = 1.0 - S + S / V, S / V
    formula = _dense_target(y, y.flip(0), lam, V, on, off)
    assert mixed.shape == (R, V) and float((mixed - formula).abs().max()) <= 1e-6
    assert float((mixed.sum(1) - 1).abs().max()) <= 1e-5
    g = torch.Generator().manual_seed(7 * R)
    loose = (torch.rand((R, V), generator=g) * 3 * (torch.rand((R, V), generator=g) > 0.5)).cuda()
    loose[0] = 0.0
    for what, t, ref_fn in (("mixup rows", mixed, lambda x, t: F.cross_entropy(x, t, reduction="none")),
                            ("loose rows", loose, lambda x, t: -(t * torch.log_softmax(x, 1)).sum(1))):
        tbuf = torch.full((R, ld), 1e9, dtype=F32, device="cuda")
        tbuf[:, :V] = t
        lse, tsum, rows = Fx.ce_soft_fwd(logits, V, tbuf)
        xr = logits[:, :V].clone().requires_grad_(True)
        ref_rows = ref_fn(xr, t)
        _check_rows(rows, ref_rows.detach(), what)
        _close(tsum, t.sum(1), 1e-5, what + " target sums")
        for name, scale in _scales(labels.clamp(min=0), w):
            d = Fx.ce_soft_bwd(logits, V, tbuf, lse, tsum, scale.contiguous(), ldd)
            ref_grad, = torch.autograd.grad((ref_rows * scale).sum(), xr, retain_graph=True)
            _check_dlogits(d, ref_grad, V, torch.zeros(R, dtype=torch.bool, device="cuda"), f"{what} {name}")
            if what == "loose rows":
                assert float(rows[0]) == 0.0 and float(d[0].float().abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- xfm_mixup
def _check_mixed(out, x0, lam, box):
    """Row i of `out` against timm's _mix_batch / _mix_elem on the original batch x0 with the host parameters lam [B], box [B, 4]."""
    xf = x0.flip(0)
    tol = 4 * 2.0 ** -24 * float(x0.abs().max())   # two rounded products and a sum in fp32
    for i in range(x0.shape[0]):
        l, (yl, yh, xl, xh) = float(lam[i]), (int(v) for v in box[i])
        if l == 1.0:
            assert torch.equal(out[i], x0[i]), f"row {i}: lam = 1 must leave the row bit-identical"
        elif yh <= yl or xh <= xl:
            ref = l * x0[i] + (1 - l) * xf[i]
            assert float((out[i] - ref).abs().max()) <= tol, (i, float((out[i] - ref).abs().max()), tol)
        else:
            ref = x0[i].clone()
            ref[:, yl:yh, xl:xh] = xf[i][:, yl:yh, xl:xh]
            assert torch.equal(out[i], ref), f"row {i}: CutMix pixels must be bit-equal (inside: the source, outside: the input)"


def _mix_params(name, B, H, W):
    lam, box = np.full(B, 0.25, dtype=np.float32), np.zeros((B, 4), dtype=np.int32)
    interior, edges = (H // 4, H // 4 + H // 2, W // 4, W // 4 + W // 2 + 1), (0, H // 3, W - W // 3, W)   # the second touches two edges
    if name == "identity":
        lam[:] = 1.0
    elif name == "cut_interior":
        box[:] = interior
    elif name == "cut_edges":
        box[:] = edges
    elif name == "elem":   # per-row different parameters
        lam[:] = [0.25, 0.5, 1.0, 0.75, 0.6, 0.9][:B]
        box[1], box[3] = interior, edges
        if B > 4:
            box[5] = (H - 3, H, 0, 5)
    return lam, box


@pytest.mark.parametrize("params", ["mixup", "identity", "cut_interior", "cut_edges", "elem"])
@pytest.mark.parametrize("H,W", [(32, 32), (30, 34), (15, 7)])   # (30, 34): 16-byte groups that straddle image lines; (15, 7): the scalar kernel
@pytest.mark.parametrize("B", [4, 6])
def test_mixup_kernel(B, H, W, params):
    Fx = _fx()
    x0 = _rand((B, 3, H, W), 1.0, F32, seed=B * H + W)
    lam, box = _mix_params(params, B, H, W)
    x = x0.clone()
    out = Fx.mixup_(x, torch.from_numpy(lam).cuda(), torch.from_numpy(box).cuda())
    assert out.data_ptr() == x.data_ptr()
    _check_mixed(x, x0, lam, box)


def test_mixup_entry_points_report_argument_errors():
    Fx = _fx()
    from xfm_amd._lib import XfmHipError
    x = torch.zeros((3, 3, 8, 8), dtype=F32, device="cuda")
    with pytest.raises(XfmHipError, match="even batch"):
        Fx.mixup_(x, torch.ones(3, device="cuda"), torch.zeros((3, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(XfmHipError, match="bad shape"):   # 1001 % 4 != 0
        Fx.ce_smooth_fwd(torch.zeros((2, 1001), device="cuda"), 1001, torch.zeros(2, dtype=torch.int64, device="cuda"), 1.0, 0.0)


# --------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("C", [1000, 1001, 3])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_criteria_modules_against_torch(dtype, C):
    from xfm_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    x = _rand((6, C), 2.0, dtype, seed=400 + C)
    labels = torch.randint(0, C, (6,), generator=torch.Generator().manual_seed(C)).cuda()
    lam = torch.tensor([0.3] * 6, dtype=F32, device="cuda")
    target = _dense_target(labels, labels.flip(0), lam, C, 1.0 - S + S / C, S / C)
    for what, crit, arg, ref_fn in (("soft", SoftTargetCrossEntropy(), target, lambda xf: F.cross_entropy(xf, target)),
                                    ("smooth", LabelSmoothingCrossEntropy(S), labels, lambda xf: F.cross_entropy(xf, labels, label_smoothing=S))):
        xg = x.clone().requires_grad_(True)
        loss = crit(xg, arg)
        loss.backward()
        xf = x.detach().float().clone().requires_grad_(True)   # (a copy: x.float() of fp32 logits is x itself)
        ref = ref_fn(xf)
        ref.backward()
        assert loss.dim() == 0 and abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (what, float(loss), float(ref))
        assert xg.grad.dtype == dtype and xg.grad.shape == x.shape
        _close(xg.grad, xf.grad, 1e-2, what + " grad")


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_mixup_module(mode):
    from xfm_amd.mixup import Mixup
    np.random.seed(1)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=10, mode=mode)
    drawn, draw = [], mix.draw
    mix.draw = lambda B, H, W: drawn.append(draw(B, H, W)) or drawn[-1]
    kinds = set()
    for call in range(4):
        x0 = _rand((6, 3, 32, 32), 1.0, F32, seed=500 + call)
        y = torch.randint(0, 10, (6,), generator=torch.Generator().manual_seed(call)).cuda()
        x = x0.clone()
        out, soft = mix(x, y)
        lam, box = drawn[-1]
        assert out.data_ptr() == x.data_ptr() and lam.shape == (6,) and box.shape == (6, 4)
        _check_mixed(x, x0, lam, box)
        ref = _dense_target(y, y.flip(0), torch.from_numpy(lam).cuda(), 10, 1.0 - 0.1 + 0.01, 0.01)
        assert soft.shape == (6, 10) and soft.dtype == F32 and float((soft - ref).abs().max()) <= 1e-6
        assert float((soft.sum(1) - 1).abs().max()) <= 1e-5
        kinds |= {bool(b[1] > b[0] and b[3] > b[2]) for b in box}
    assert kinds == {True, False}   # the seeded draws reached both CutMix and mixup
    with pytest.raises(AssertionError):
        mix(torch.zeros((5, 3, 32, 32), device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"))
    with pytest.raises(NotImplementedError, match="pair"):
        Mixup(mode="pair")
    with pytest.raises(NotImplementedError, match="cutmix_minmax"):
        Mixup(cutmix_minmax=(0.2, 0.8))


def test_imagenet_step_with_mixup_and_soft_target_ce(tmp_path, monkeypatch):
    """The step of Imagenet.py:468-492 on the ImageNet branch of XFMForClassification (2-block tower, B = 4, 224 px, 1000 classes):
    Mixup -> model(images, None, None, None, False) -> SoftTargetCrossEntropy -> backward.  The loss against torch's fp32 soft-target CE
    of the returned logits; the last head weight's gradient against dlogits^T . features in fp32 torch, by the module tests' rule."""
    from test_hip_configs import _cfg, _formula, _vision_checkpoint
    from test_hip_modules import COS_TOL, GRAD_TOL
    from xfm_amd import synthetic as syn, xfm as xfm_mod
    from xfm_amd.losses import SoftTargetCrossEntropy
    from xfm_amd.mixup import Mixup
    from xfm_amd.model_classification import XFMForClassification
    m = XFMForClassification(_cfg(224, 1, 1, 2, vision_config=_vision_checkpoint(tmp_path, 2, 224), task_name="imagenet", num_labels=1000))
    _formula(m)
    m.cuda().finalize().eval()
    seen, linear_slot = [], xfm_mod.linear_slot

    def spy(x, slot, *a, **kw):
        if slot is m.cls_head._slots[4]:
            seen.append(x.detach().float())
        return linear_slot(x, slot, *a, **kw)
    monkeypatch.setattr(xfm_mod, "linear_slot", spy)
    images = syn.gaussian("softce.image", (4, 3, 224, 224)).cuda()
    targets = torch.tensor([3, 999, 0, 500]).cuda()
    np.random.seed(1)
    images, soft = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=1000)(images, targets)
    logits = m(images, None, None, None, False)
    assert logits.shape == (4, 1000) and len(seen) == 1
    loss = SoftTargetCrossEntropy()(logits, soft)
    loss.backward()
    lf = logits.detach().float().requires_grad_(True)
    ref = F.cross_entropy(lf, soft)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (float(loss), float(ref))
    got = dict(m.named_parameters())["cls_head.12.weight"].grad.float()
    want = lf.grad.t() @ seen[0].reshape(4, -1)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    err = float((got - want).norm() / want.norm())
    cos = float((got * want).sum() / (got.norm() * want.norm()))
    print(f"cls_head.12.weight.grad: rel-L2 {err:.4f}, cosine {cos:.5f}")
    assert err <= GRAD_TOL and cos >= COS_TOL, (err, cos)
