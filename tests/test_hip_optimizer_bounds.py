"""The optimizer family (optimizer.hip) under elementwise fp64 bounds: adamw_kernel in both rules, sumsq.

The existing kernel tests hold p to 1e-4 of max |p| -- 40 % of one update and five times the two steps' whole decay -- with group ids 0
and 1 and, for the transformers rule, without a second grid-stride trip.  Here p', m' and v' of every element are held to
step_tail_util.adamw_ref's bound, which is relative to the element's own update, its own decay and one rounding of its own magnitude, for
both rules at n = 256, 1280 and 4096 * 1024 + 512 (a second trip whose two 256-blocks lie in different groups), steps 1, 2 and 1000 with m
and v carried on the device (the reference restarts every step from the device's p, m and v), both beta pairs, with and without clip and
zero_grad, group ids 0, 1 and 2 inside a uint8 parent filled with 3, whose slot holds lr = 1e3.  Planted 256-blocks: g = 0 on m = v = 0 (pure
decay; m' and v' stay +0), |g| about eps (where the two rules part), and beta1 m about -(1 - beta1) g.  p, g, m and v are views of 7.0
parents at a 16-byte offset; a rejected call must not write at all.  sumsq runs n around one block's 1024 elements and one past the
1024-partial grid cap, onto 0 and onto 3.0, through a NaN-filled workspace, twice for equal bits.

Every check prints `step-ratio gpu <kernel> <case> <quantity> <worst err / bound>` (pytest -s)."""
import ctypes

import pytest
import torch

import step_tail_util as S
from step_tail_util import F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_ARG = -1       # XFM_E_ARG


def _L():
    from xfm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(kernel, case, what, ratio):
    S.report("gpu", kernel, case, what, ratio)


def _adamw_call(lib, rule, o, group, n, betas, step, clip, zero_grad):
    bc1, bc2 = S.bias_corrections(*betas, step)
    a = _L().AdamWArgs(p=o["p"].data_ptr(), g=o["g"].data_ptr(), m=o["m"].data_ptr(), v=o["v"].data_ptr(), group=group.data_ptr(),
                       beta1=betas[0], beta2=betas[1], eps=S.ADAMW_EPS, bc1=bc1, bc2=bc2,
                       clip_coef=None if clip is None else clip.data_ptr(), n=n, zero_grad=zero_grad)
    for i in range(4):
        a.lr[i], a.wd[i] = S.ADAMW_LR[i], S.ADAMW_WD[i]
    rc = (lib.xfm_adamw_torch if rule == "torch" else lib.xfm_adamw)(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, bc1, bc2


def _arena(n, p, m, v):
    o = S.TailOuts(DEV)
    for name, t in (("p", p), ("m", m), ("v", v), ("g", torch.zeros(n))):
        ptr = o.add(name, (n,), F32, init=t)
        assert ptr % 16 == 0
    return o


@pytest.mark.parametrize("rule", ["transformers", "torch"])
@pytest.mark.parametrize("n", S.ADAMW_SIZES)
def test_adamw_within_bounds(rule, n):
    lib = _L().load()
    blocks, gid = S.adamw_groups(n)
    gid = gid.to(DEV)
    group = S.poisoned_ids(blocks, DEV, 3)
    state = S.adamw_state(n)
    zero_blk = slice(S.BLK_ZERO * 256, (S.BLK_ZERO + 1) * 256)
    for betas, clip_value, zero_grad in S.ADAMW_OPTIONS:
        clip = None if clip_value is None else S.poisoned_in(torch.tensor([clip_value], dtype=F32), DEV)
        o = _arena(n, *state)
        case = f"{rule}:{n}:{betas[1]}:{clip_value}"
        for step in S.ADAMW_STEPS:
            g = S.adamw_grad(n, step, o["m"], betas[0]).to(DEV)
            o["g"].copy_(g)
            p0, m0, v0 = o["p"].clone(), o["m"].clone(), o["v"].clone()
            rc, bc1, bc2 = _adamw_call(lib, rule, o, group, n, betas, step, clip, zero_grad)
            _L().check(rc, "adamw")
            o.check_outside()
            ref = S.adamw_ref(rule, p0, g, m0, v0, gid, S.ADAMW_LR, S.ADAMW_WD, betas[0], betas[1], S.ADAMW_EPS, bc1, bc2,
                              None if clip is None else clip[0])
            for name in ("p", "m", "v"):
                _report("adamw", case, f"{name}:step{step}", S.check_f32(o[name], *ref[name], f"{name}, step {step}"))
            if n >= 5 * 256:
                assert not bool(o["m"][zero_blk].view(torch.int32).any()) and not bool(o["v"][zero_blk].view(torch.int32).any()), "0 / eps"
            if zero_grad:
                assert not bool(o["g"].view(torch.int32).any()), "zero_grad left g other than +0.0"
            else:
                assert S.bits_equal(o["g"], g), "g changed without zero_grad"


@pytest.mark.parametrize("rule", ["transformers", "torch"])
def test_adamw_rejection_writes_nothing(rule):
    lib = _L().load()
    n = 300
    o = _arena(n, S.randn((n,), 1.0, 1), S.randn((n,), 0.03, 2), S.randn((n,), 0.1, 3) ** 2)
    group = S.poisoned_ids(torch.zeros(2, dtype=torch.uint8), DEV, 3)
    rc, _, _ = _adamw_call(lib, rule, o, group, n, (0.9, 0.999), 1, None, 1)
    assert rc == E_ARG, rc
    o.check_unchanged()


# --------------------------------------------------------------------------------------------------------------------------- sumsq
def _sumsq(lib, x, n, out0):
    o = S.TailOuts(DEV)
    op = o.add("out", (1,), F32, init=torch.tensor([out0]))
    wp = o.add("workspace", (_L().SUMSQ_WORKSPACE_FLOATS,), F32, init=torch.full((_L().SUMSQ_WORKSPACE_FLOATS,), S.NAN))
    rc = lib.xfm_sumsq(x.data_ptr(), n, op, wp, _stream())
    torch.cuda.synchronize()
    return rc, o


@pytest.mark.parametrize("n", S.SUMSQ_SIZES)
def test_sumsq_within_bounds(n):
    lib = _L().load()
    x = S.poisoned_in(S.randn((n,), 1.0, 350), DEV)
    for out0 in (0.0, 3.0):
        rc, o = _sumsq(lib, x, n, out0)
        _L().check(rc, "sumsq")
        o.check_outside()
        _report("sumsq", str(n), f"out0={out0}", S.check_f32(o["out"], *S.sumsq_ref(x, out0), "sumsq"))
        rc, o2 = _sumsq(lib, x, n, out0)
        assert rc == 0 and S.bits_equal(o["out"], o2["out"]), "two launches differ"


def test_sumsq_rejection_writes_nothing():
    lib = _L().load()
    x = S.poisoned_in(S.randn((8,), 1.0, 350), DEV)
    rc, o = _sumsq(lib, x, 6, 3.0)
    assert rc == E_ARG, rc
    o.check_unchanged()
