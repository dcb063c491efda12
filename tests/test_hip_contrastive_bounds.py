"""The contrastive family (contrastive.hip) under elementwise fp64 bounds: rownorm, itc_fwd / itc_bwd / itc_dtemp, hard_neg.

The existing tests run itc at E = 128 and 256 and hard_neg at (8, 256) only, hold the gradients to a fraction of their largest entry and
never look at lse, cnt, the accumulation of dtemp, the bits of a second launch or the memory around a buffer.  Here every width of
XFM_EPL_DISPATCH is launched for every kernel; every element of y, inv, dx, lse (rows, then columns), dI, dT and the scalars loss and
dtemp is held to step_tail_util's bound (the backward from the lse and cnt handed to it, so it is checked on its own); cnt is exact; N sits
below the wave count, one past the 256-thread stride and at the limit 16000 (64,016 bytes of dynamic LDS); one row's maximum is planted at
columns 0, 3, 255, 256 and N - 1 in turn, so a lost column moves lse by O(1).  hard_neg's logits are exact in fp32 by construction, so
every row of every call has one right answer up to the widening of check_draw: B = 257 and 300 take every strided loop round twice and
make the scan walk past 256 entries.  Inputs are views of NaN parents (idx: of a parent filled with idx[0]'s id), outputs views of
7.0 parents that must keep their bits outside the view; a rejected call must not write at all.

Every check prints `step-ratio gpu <kernel> <case> <quantity> <worst err / bound>` (pytest -s)."""
import functools

import pytest
import torch

import step_tail_util as S
from step_tail_util import F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_ARG, E_UNSUPPORTED = -1, -3       # XFM_E_ARG, XFM_E_UNSUPPORTED


def _L():
    from xfm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(kernel, case, what, ratio):
    S.report("gpu", kernel, case, what, ratio)


def _in(t):
    return S.poisoned_in(t, DEV)


def _scalar(x):
    return _in(torch.tensor([x], dtype=F32))


def _ids(idx):
    return None if idx is None else S.poisoned_ids(idx, DEV, int(idx[0]))


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------- rownorm
@pytest.mark.parametrize("R,E", S.ROWNORM_SHAPES)
def test_rownorm_within_bounds(R, E):
    lib = _L().load()
    c = S.rownorm_case(R, E)
    case = f"{R}x{E}"
    x = _in(c["x"])
    o = S.TailOuts(DEV)
    yp, ip = o.add("y", (R, E), F32), o.add("inv", (R,), F32)
    _L().check(lib.xfm_rownorm_fwd(x.data_ptr(), R, E, yp, ip, _stream()), "rownorm_fwd")
    torch.cuda.synchronize()
    o.check_outside()
    ref = S.rownorm_fwd_ref(x)
    _report("rownorm_fwd", case, "y", S.check_f32(o["y"], *ref["y"], "y"))
    _report("rownorm_fwd", case, "inv", S.check_f32(o["inv"], *ref["inv"], "inv"))
    if R > 1:   # the all-zero row
        assert float(o["y"][R - 1].abs().max()) == 0.0 and abs(float(o["inv"][R - 1]) - 1e12) <= 1e12 * 2 * S.U32
    yg, ig = S.rownorm_given(c["x"])
    y, iv, dy = _in(yg), _in(ig), _in(c["dy"])
    o = S.TailOuts(DEV)
    dp = o.add("dx", (R, E), F32)
    _L().check(lib.xfm_rownorm_bwd(dy.data_ptr(), y.data_ptr(), iv.data_ptr(), R, E, dp, _stream()), "rownorm_bwd")
    torch.cuda.synchronize()
    o.check_outside()
    assert bool(torch.isfinite(o["dx"]).all())
    _report("rownorm_bwd", case, "dx", S.check_f32(o["dx"], *S.rownorm_bwd_ref(dy, y, iv), "dx"))


# ----------------------------------------------------------------------------------------------------------------------------- itc
def _itc_fwd(lib, I, T, tv, N, E, idx, expect=0, with_cnt=True):
    o = S.TailOuts(DEV)
    lp = o.add("lse", (4 * N,), F32)
    sp = o.add("loss_sum", (2,), F32, init=torch.zeros(2))          # zeroed by the caller, as the header requires
    cp = o.add("cnt", (N,), F32) if idx is not None and with_cnt else None
    rc = lib.xfm_itc_fwd(I.data_ptr(), T.data_ptr(), tv.data_ptr(), N, E, lp, sp, _ptr(idx), cp, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.xfm_last_error())
    if expect:
        o.check_unchanged()
    else:
        o.check_outside()
        assert int(o["loss_sum"].view(torch.int32)[1]) == 2 * N, "the ticket counter"
    return o


def _itc_bwd(lib, I, T, tv, lse_g, gv, N, E, idx, cnt, expect=0):
    o = S.TailOuts(DEV)
    lp = o.add("lse", (4 * N,), F32, init=torch.cat([lse_g, torch.full((2 * N,), S.SENTINEL, device=lse_g.device)]))
    ip, tp = o.add("dI", (N, E), F32), o.add("dT", (N, E), F32)
    dp = o.add("dtemp", (1,), F32, init=torch.tensor([S.ITC_DTEMP0]))
    rc = lib.xfm_itc_bwd(I.data_ptr(), T.data_ptr(), tv.data_ptr(), lp, gv.data_ptr(), N, E, ip, tp, dp, _ptr(idx), _ptr(cnt), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.xfm_last_error())
    if expect:
        o.check_unchanged()
    else:
        o.check_outside()       # nothing past the documented 4N floats
        assert S.bits_equal(o["lse"][:2 * N], lse_g.to(DEV)), "the backward changed the statistics lse[0, 2N)"
    return o


@functools.lru_cache(maxsize=2)
def _itc_case(N, E, with_idx):
    return S.itc_case(N, E, with_idx)


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("N,E", S.ITC_SHAPES)
def test_itc_within_bounds(N, E, with_idx):
    lib = _L().load()
    c = _itc_case(N, E, with_idx)
    I, idx, gv = _in(c["I"]), _ids(c["idx"]), _scalar(S.ITC_G)
    cols, r = S.itc_plants(N)
    for temp in S.ITC_TEMPS:
        tv = _scalar(temp)
        case = f"{N}x{E}:{'idx' if with_idx else 'eye'}:{temp}"
        for j in cols:
            T = _in(S.itc_planted(c, j, r))
            o = _itc_fwd(lib, I, T, tv, N, E, idx)
            ref = S.itc_fwd_ref(I, T, tv[0], idx)
            _report("itc_fwd", case, f"lse:{j}", S.check_f32(o["lse"][:2 * N], *ref["lse"], f"lse, T_{j} = I_{r}"))
            _report("itc_fwd", case, f"loss:{j}", S.check_f32(o["loss_sum"][:1], *ref["loss"], f"loss, T_{j} = I_{r}"))
            if with_idx:
                assert torch.equal(o["cnt"].double(), ref["cnt"]), "cnt"
            if j is None:
                o2 = _itc_fwd(lib, I, T, tv, N, E, idx)
                assert S.bits_equal(o["loss_sum"][:1], o2["loss_sum"][:1]) and S.bits_equal(o["lse"], o2["lse"]), "two forward launches differ"
        # the backward, from statistics of its own: the fp64 lse rounded once, the exact counts
        T = _in(c["T"])
        ref = S.itc_fwd_ref(I, T, tv[0], idx)
        lse_g = ref["lse"][0].float()
        cnt = _in(ref["cnt"].float()) if with_idx else None
        o = _itc_bwd(lib, I, T, tv, lse_g, gv, N, E, idx, cnt)
        bref = S.itc_bwd_ref(I, T, tv[0], lse_g, gv[0], S.ITC_DTEMP0, idx, cnt)
        for k in ("dI", "dT", "dtemp"):
            _report("itc_bwd", case, k, S.check_f32(o[k], *bref[k], k))
        o2 = _itc_bwd(lib, I, T, tv, lse_g, gv, N, E, idx, cnt)
        assert all(S.bits_equal(o[k], o2[k]) for k in ("dI", "dT", "dtemp")), "two backward launches differ"


def test_itc_limit_shape():
    """N = XFM_LOSS_MAXN: both kernels launch with 64,016 bytes of dynamic LDS.  The references work a block of rows at a time."""
    lib = _L().load()
    N, E, temp = S.LOSS_MAXN, 64, S.ITC_TEMPS[0]
    c = S.itc_case(N, E, False)
    I, T, tv, gv = _in(c["I"]), _in(c["T"]), _scalar(temp), _scalar(S.ITC_G)
    o = _itc_fwd(lib, I, T, tv, N, E, None)
    ref = S.itc_fwd_ref(I, T, tv[0], None, chunk=2000)
    _report("itc_fwd", f"{N}x{E}", "lse", S.check_f32(o["lse"][:2 * N], *ref["lse"], "lse"))
    _report("itc_fwd", f"{N}x{E}", "loss", S.check_f32(o["loss_sum"][:1], *ref["loss"], "loss"))
    lse_g = ref["lse"][0].float()
    o = _itc_bwd(lib, I, T, tv, lse_g, gv, N, E, None, None)
    g = torch.Generator(device="cpu").manual_seed(7)
    rows = torch.cat([torch.tensor([0, N - 1]), 1 + torch.randperm(N - 2, generator=g)[:62]]).to(DEV)
    bref = S.itc_bwd_ref(I, T, tv[0], lse_g, gv[0], S.ITC_DTEMP0, None, None, rows=rows, chunk=2000)
    _report("itc_bwd", f"{N}x{E}", "dI", S.check_f32(o["dI"][rows], *bref["dI"], "dI rows"))
    _report("itc_bwd", f"{N}x{E}", "dT", S.check_f32(o["dT"][rows], *bref["dT"], "dT rows"))
    _report("itc_bwd", f"{N}x{E}", "dtemp", S.check_f32(o["dtemp"], *bref["dtemp"], "dtemp"))


@pytest.mark.parametrize("N,E,code,idx_no_cnt", [(S.LOSS_MAXN + 1, 64, E_ARG, False), (4, 192, E_UNSUPPORTED, False), (4, 100, E_ARG, False),
                                                 (4, 64, E_ARG, True)])
def test_itc_rejections_write_nothing(N, E, code, idx_no_cnt):
    lib = _L().load()
    I, T = _in(S.randn((N, E), 0.1, 1)), _in(S.randn((N, E), 0.1, 2))
    tv, gv = _scalar(0.07), _scalar(S.ITC_G)
    idx = _ids(S.shared_ids(N, 3)) if idx_no_cnt else None
    _itc_fwd(lib, I, T, tv, N, E, idx, expect=code, with_cnt=False)
    _itc_bwd(lib, I, T, tv, torch.zeros(2 * N, device=DEV), gv, N, E, idx, None, expect=code)


# ------------------------------------------------------------------------------------------------------------------------ hard_neg
def _hard_neg(lib, I, T, tv, B, E, seed, idx, expect=0):
    o = S.TailOuts(DEV)
    ip, tp = o.add_ids("image_neg", B), o.add_ids("text_neg", B)
    rc = lib.xfm_hard_negatives(I.data_ptr(), T.data_ptr(), tv.data_ptr(), B, E, seed, ip, tp, _ptr(idx), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.xfm_last_error())
    if expect:
        o.check_unchanged()
    else:
        o.check_outside()
    return o


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("B,E", S.HARD_NEG_SHAPES)
def test_hard_neg_every_draw(B, E, with_idx):
    lib = _L().load()
    c = S.hard_neg_case(B, E, with_idx)
    I, T, tv, idx = _in(c["I"]), _in(c["T"]), _scalar(S.HARD_NEG_TEMP), _ids(c["idx"])
    weights = dict(zip(("text_neg", "image_neg"), S.hard_neg_weights(I, T, tv[0], idx)))     # image rows draw text_neg
    worst = 0.0
    for seed in S.HARD_NEG_SEEDS:
        o = _hard_neg(lib, I, T, tv, B, E, seed, idx)
        for name, first in (("text_neg", 0), ("image_neg", B)):
            pick, w = o[name], weights[name]
            assert bool(((pick >= 0) & (pick < B)).all()), f"{name}: a pick outside [0, {B})"
            ok = w.sum(1) > 0              # B = 2 with idx: both rows share the id and no row has any weight
            if bool(ok.any()):
                u = S.hard_neg_u(seed, first, B).to(DEV)
                worst = max(worst, S.check_draw(pick[ok], u[ok], w[ok], f"{name}, seed {seed}"))
        o2 = _hard_neg(lib, I, T, tv, B, E, seed, idx)
        assert torch.equal(o["image_neg"], o2["image_neg"]) and torch.equal(o["text_neg"], o2["text_neg"]), "two launches differ"
    _report("hard_neg", f"{B}x{E}:{'idx' if with_idx else 'eye'}", "draw", worst)


def test_hard_neg_no_weight_and_batch_of_one():
    lib = _L().load()
    B, E = 64, 128
    c = S.hard_neg_case(B, E, False)
    I, T, tv = _in(c["I"]), _in(c["T"]), _scalar(S.HARD_NEG_TEMP)
    idx = _ids(torch.full((B,), 1234, dtype=torch.int64))       # every row shares one id: every weight is 0
    o = _hard_neg(lib, I, T, tv, B, E, 5, idx)
    for name in ("image_neg", "text_neg"):
        assert bool(((o[name] >= 0) & (o[name] < B)).all()), name
    _hard_neg(lib, I, T, tv, 1, E, 5, None, expect=E_ARG)
