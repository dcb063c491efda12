"""What the two encoder routes share (xfm_amd.roberta_encoder), on CPU tensors and without a kernel launch: the gradient edges of a
tower output / input bit for bit against the expressions written out here, the decision table of the image-state-gradient plan, and
the argument checks."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from xfm_amd import roberta_encoder as RE

BF16, F32 = torch.bfloat16, torch.float32
D, ENC_ROWS = 64, 6


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- _grad_pair
def test_grad_pair_five_cases():
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(5, D, generator=g).to(BF16)
    dy32 = torch.randn(5, D, generator=g) * 1e-2
    # dy only (either switch): the bf16 edge alone
    for f32 in (True, False):
        a, b = RE._grad_pair(dy, None, f32)
        assert _same(a, dy.contiguous()) and b is None
    # dy32 only: a zero bf16 edge is made up; the twin's gradient stays fp32 with the stream on, is folded in and rounded with it off
    a, b = RE._grad_pair(None, dy32, True)
    assert _same(a, torch.zeros(dy32.shape, dtype=BF16)) and _same(b, dy32.contiguous())
    a, b = RE._grad_pair(None, dy32, False)
    assert _same(a, (torch.zeros(dy32.shape, dtype=BF16).float() + dy32).to(BF16)) and b is None
    # both, fp32 stream on: two edges, nothing rounded
    a, b = RE._grad_pair(dy, dy32, True)
    assert _same(a, dy.contiguous()) and _same(b, dy32.contiguous())
    # both, fp32 stream off: summed in fp32, rounded once
    a, b = RE._grad_pair(dy, dy32, False)
    assert _same(a, (dy.contiguous().float() + dy32).to(BF16)) and b is None
    # neither
    with pytest.raises(RuntimeError, match="encoder backward without a gradient"):
        RE._grad_pair(None, None, True)


def test_grad_pair_casts_and_makes_contiguous():
    dy = torch.randn(4, 2 * D)[:, ::2]           # fp32, strided
    dy32 = torch.randn(4, 2 * D)[:, ::2]
    a, b = RE._grad_pair(dy, dy32, True)
    assert a.is_contiguous() and b.is_contiguous() and _same(a, dy.contiguous().to(BF16)) and _same(b, dy32.contiguous())


# -------------------------------------------------------------------------------------------------------------- _input_grads
@pytest.mark.parametrize("pad", [0, 3])
def test_input_grads_with_and_without_twin(pad):
    g = torch.Generator().manual_seed(11)
    rows = 5
    dy_a = torch.randn(rows, D, generator=g).to(BF16)
    b32 = torch.randn(rows, D, generator=g) * 1e-2
    zeros = lambda dt: torch.zeros((pad, D), dtype=dt)   # noqa: E731
    padded = lambda t: torch.cat([t, zeros(t.dtype)], dim=0) if pad > 0 else t   # noqa: E731
    assert RE._input_grads(dy_a, b32, False, True, rows + pad) == (None, None)
    # a twin on the input and an fp32 residual-branch gradient: two edges, un-rounded
    dx, dx32 = RE._input_grads(dy_a, b32, True, True, rows + pad)
    assert _same(dx, padded(dy_a)) and _same(dx32, padded(b32))
    # no twin: summed in fp32 and rounded once
    dx, dx32 = RE._input_grads(dy_a, b32, True, False, rows + pad)
    assert _same(dx, padded((dy_a.float() + b32.float()).to(BF16))) and dx32 is None
    # a twin, but the bf16 stream's residual gradient: summed as well
    b16 = b32.to(BF16)
    dx, dx32 = RE._input_grads(dy_a, b16, True, True, rows + pad)
    assert _same(dx, padded((dy_a.float() + b16.float()).to(BF16))) and dx32 is None


# ------------------------------------------------------------------------------------------------------------------ EncGrad
class _Layer:
    """Stands in for a RobertaLayer (compared by identity, like an nn.Module): kv2.wt is the transposed K|V weight [D_enc, 2D] plus
    padding columns the plan must cut off."""

    def __init__(self, g):
        self._s = {"kv2": SimpleNamespace(wt=torch.randn(D, 2 * D + 8, generator=g).to(BF16))}


def _cross_layers(n):
    g = torch.Generator().manual_seed(3)
    return [_Layer(g) for _ in range(n)]


@pytest.mark.parametrize("need_denc,per_image,n", list(itertools.product([False, True], [False, True], [0, 1, 3])))
def test_enc_grad_decision_table(need_denc, per_image, n):
    enc = torch.randn(ENC_ROWS, D).to(BF16)
    layers = _cross_layers(n)
    eg = RE.EncGrad(enc, layers, D, need_denc, per_image)
    concat = need_denc and per_image and n > 1
    assert eg.concat_k is concat
    if concat:
        assert eg.denc32 is None and eg.dkv_all.shape == (ENC_ROWS, n * 2 * D) and eg.dkv_all.dtype == BF16
    elif need_denc:
        assert eg.dkv_all is None and eg.denc32.shape == (ENC_ROWS, D) and eg.denc32.dtype == F32
        assert torch.count_nonzero(eg.denc32) == 0
    else:
        assert eg.dkv_all is None and eg.denc32 is None
    for j, layer in enumerate(layers):
        dkv = eg.dkv_of(layer)
        assert dkv.shape == (ENC_ROWS, 2 * D) and dkv.dtype == BF16
        if concat:   # columns [j * 2D, (j + 1) * 2D) of the one buffer
            assert dkv.data_ptr() == eg.dkv_all.data_ptr() + j * 2 * D * 2 and dkv.stride(0) == eg.dkv_all.stride(0) == n * 2 * D
            dkv.fill_(j + 1)
            assert torch.equal(eg.dkv_all[:, j * 2 * D:(j + 1) * 2 * D], torch.full((ENC_ROWS, 2 * D), j + 1, dtype=BF16))
        else:        # a buffer of its own every time
            assert dkv.is_contiguous() and dkv.data_ptr() != eg.dkv_of(layer).data_ptr()


def test_enc_grad_without_image_states():
    eg = RE.EncGrad(None, [], D, False, True)
    assert not eg.concat_k and eg.dkv_all is None and eg.denc32 is None
    assert eg.finish(lambda: pytest.fail("nothing to wait for")) is None


def test_enc_grad_finish(monkeypatch):
    enc = torch.randn(ENC_ROWS, D).to(BF16)
    order = []
    # accumulated route: wait, then round denc32 once
    eg = RE.EncGrad(enc, _cross_layers(1), D, True, True)
    eg.denc32.copy_(torch.randn(ENC_ROWS, D))
    denc = eg.finish(lambda: order.append("wait"))
    assert order == ["wait"] and _same(denc, eg.denc32.to(BF16))
    # column-block route: ONE GEMM of dkv_all against the column-concatenated kv2.wt[:, :2D], behind the wait
    layers = _cross_layers(3)
    eg = RE.EncGrad(enc, layers, D, True, True)
    calls = []

    def gemm_nt(a, b, *args, **kw):
        order.append("gemm")
        calls.append((a, b, args, kw))
        return "denc"
    monkeypatch.setattr(RE.Fx, "gemm_nt", gemm_nt)
    del order[:]
    assert eg.finish(lambda: order.append("wait")) == "denc" and order == ["wait", "gemm"]
    (a, b, args, kw), = calls
    assert a is eg.dkv_all and not args and not kw
    assert _same(b, torch.cat([layer._s["kv2"].wt[:, :2 * D] for layer in layers], dim=1)) and b.shape == (D, 3 * 2 * D)
    # nobody reads the gradient: no wait, no launch
    del order[:]
    assert RE.EncGrad(enc, layers, D, False, True).finish(lambda: order.append("wait")) is None and order == []


# ------------------------------------------------------------------------------------------------------- checks, row prefix
def test_check_pass_args():
    pack, keep, enc = object(), torch.ones(2, 4, dtype=torch.int32), torch.zeros(2, D)
    msg_pack = "packed rows take neither a key mask (lengths say it all) nor the causal mask"
    msg_gb = "grad_batch is for self-attention-only passes: 0 < grad_batch <= batch"
    for key_keep, causal in ((keep, False), (None, True), (keep, True)):
        with pytest.raises(ValueError) as e:
            RE.check_pass_args(pack, key_keep, causal, None, None, 4)
        assert str(e.value) == msg_pack and type(e.value) is ValueError
    for grad_batch, e_states in ((0, None), (5, None), (-1, None), (2, enc)):
        with pytest.raises(ValueError) as e:
            RE.check_pass_args(None, None, False, grad_batch, e_states, 4)
        assert str(e.value) == msg_gb and type(e.value) is ValueError
    # what passes: no pack with a mask / causal, a pack without them, grad_batch in 1 .. B without image states
    RE.check_pass_args(None, keep, True, None, enc, 4)
    RE.check_pass_args(pack, None, False, None, enc, 4)
    for grad_batch in (1, 4):
        RE.check_pass_args(pack, None, False, grad_batch, None, 4)


def test_both_routes_use_the_shared_pieces():
    from xfm_amd import roberta_native as RN
    for name in ("check_pass_args", "pass_needs", "head_rows", "EncGrad", "_grad_pair", "_input_grads"):
        assert getattr(RN, name) is getattr(RE, name)


def test_head_rows():
    assert RE.head_rows(3, 30, None) == 90
    pack = SimpleNamespace(rows_of_head=lambda b: {3: 41}[b])
    assert RE.head_rows(3, 30, pack) == 41


def test_switches_and_seed_counter_stay_on_xroberta():
    from xfm_amd import roberta_layer as RL, roberta_native as RN, xroberta as XR
    assert XR._seed_counter is RL._seed_counter and XR._next_seed is RL._next_seed
    assert XR._EncoderFn is RE._EncoderFn and XR._EncoderFnNative is RN._EncoderFnNative
    assert isinstance(XR._F32_STREAM, bool) and isinstance(XR._NATIVE_LAYERS, bool)
    assert not hasattr(RE, "_F32_STREAM") and not hasattr(RN, "_F32_STREAM")   # no copy of the switch frozen at import
    before = RL._seed_counter[0]
    XR._next_seed()
    assert XR._seed_counter[0] == before + 1
    XR._seed_counter[0] = before
