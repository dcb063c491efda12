"""The step-tail bounds (step_tail_util) are neither vacuous nor too tight, shown on the CPU.  For every case builder of
tests/test_hip_contrastive_bounds.py and tests/test_hip_optimizer_bounds.py a plain fp32 torch evaluation of each formula (the dot
products as 64 lane partials and a halving tree, the CDF as a serial fp32 scan) stays within 0.75 of its bound, and every planted fault on
such an emulated output lands past the bound.  The hard-negative design is checked for every shape: the fp32 logits equal the fp64 ones
bit for bit, every emulated pick lies inside the widened interval, delta / W <= 1e-4.  The worst ratios are printed (pytest -s) as
`step-ratio cpu <kernel> <case> <quantity> <ratio>` lines; profiles/tests_step_tail_bounds.md sets them next to the MI355X's."""
import os

import pytest
import torch

import step_tail_util as S
from step_tail_util import F32, U32

CPU_MAX = 0.75


def _report(kernel, case, what, ratio):
    S.report("cpu", kernel, case, what, ratio)
    assert ratio <= CPU_MAX, f"{kernel} {case} {what}: emulation at {ratio:.3g} of the bound (limit {CPU_MAX})"


def _fails(fn, match="past the bound"):
    with pytest.raises(AssertionError, match=match):
        fn()


def t32(x):
    return torch.tensor(x, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------ fp32 emulations
def lane_sum(t):
    """[..., E] -> [...]: lane l adds its elements of every 64-wide slice in turn, then a halving tree across the 64 lanes"""
    lanes = t.reshape(*t.shape[:-1], t.shape[-1] // 64, 64)
    acc = lanes[..., 0, :].clone()
    for i in range(1, lanes.shape[-2]):
        acc = acc + lanes[..., i, :]
    n = 64
    while n > 1:
        n //= 2
        acc = acc[..., :n] + acc[..., n:2 * n]
    return acc[..., 0]


def emul_rownorm_fwd(x):
    n = torch.sqrt(lane_sum(x * x)).clamp_min(t32(1e-12))
    iv = 1.0 / n
    return x * iv.unsqueeze(1), iv


def emul_rownorm_bwd(dy, y, inv):
    s = lane_sum(dy * y)
    return (dy - y * s.unsqueeze(1)) * inv.unsqueeze(1)


def emul_logits(own, oth, temp):
    return lane_sum(own.unsqueeze(1) * oth.unsqueeze(0)) * (1.0 / t32(temp))


def emul_lse(L):
    mx = L.max(1).values
    return mx + torch.log(torch.exp(L - mx.unsqueeze(1)).sum(1))


def emul_itc_fwd(I, T, temp, idx, keep=None, rows=None):
    """(lse [2N], loss [1]) in fp32; keep: a bool [N] column mask (a planted fault), rows: the number of row terms summed"""
    N = I.shape[0]
    lse, terms = [], []
    for own, oth in ((I, T), (T, I)):
        L = emul_logits(own, oth, temp)
        Lk = L if keep is None else L[:, keep]
        l = emul_lse(Lk)
        if idx is None:
            pos = L.diagonal()
        else:
            same = (idx.unsqueeze(1) == idx.unsqueeze(0)).float()
            pos = (L * same).sum(1) / same.sum(1)
        lse.append(l)
        terms.append((l - pos) / (2.0 * N))
    t = torch.cat(terms)
    return torch.cat(lse), (t if rows is None else t[:rows]).sum().reshape(1)


def emul_itc_bwd(I, T, temp, lse, g, d0, idx, cnt, keep=None):
    N = I.shape[0]
    inv_temp, gs = 1.0 / t32(temp), t32(g) / (2.0 * N)
    out = []
    for own, oth, lo, lt in ((I, T, lse[:N], lse[N:]), (T, I, lse[N:], lse[:N])):
        L = emul_logits(own, oth, temp)
        if idx is None:
            lab = 2.0 * torch.eye(N)
        else:
            lab = (idx.unsqueeze(1) == idx.unsqueeze(0)).float() * (1.0 / cnt.unsqueeze(1) + 1.0 / cnt.unsqueeze(0))
        G = torch.exp(L - lo.unsqueeze(1)) + torch.exp(L - lt.unsqueeze(0)) - lab
        if keep is not None:
            G = G * keep.float().unsqueeze(0)
        out.append(((G * gs) @ oth) * inv_temp)
        if own is I:
            share = -(G * L).sum(1) * gs * inv_temp
    return out[0], out[1], (t32(d0) + share.sum()).reshape(1), (t32(d0) + share[:-1].sum()).reshape(1)


def emul_scan(I, T, temp, idx, side, keep=None):
    """(w fp32 [B, B], c: its serial fp32 running sum along the row, wsum: the kernel's tree-free stand-in, the plain fp32 sum)"""
    L = (I @ T.t()) * (1.0 / t32(temp))
    if side == "txt":
        L = L.t()
    B = L.shape[0]
    mx = L.max(1, keepdim=True).values
    e = torch.exp(L - mx)
    inv = 1.0 / e.sum(1, keepdim=True)
    same = torch.eye(B, dtype=torch.bool) if idx is None else idx.unsqueeze(1) == idx.unsqueeze(0)
    w = torch.where(same, torch.zeros(()), e * inv + t32(1e-5))
    if keep is not None:
        w = w * keep.float().unsqueeze(0)
    c = torch.zeros_like(w)
    run = torch.zeros(B)
    for j in range(B):
        run = run + w[:, j]
        c[:, j] = run
    return w, c, w.sum(1)


def emul_pick(w, c, wsum, u):
    B = w.shape[1]
    x = (u.float() * wsum).unsqueeze(1)
    ar = torch.arange(B).expand_as(w)
    first = torch.where((w > 0) & (x < c), ar, torch.full_like(ar, B)).min(1).values
    last = torch.where(w > 0, ar, torch.full_like(ar, -1)).max(1).values
    return torch.where(first < B, first, last)


def emul_adamw(rule, p, g, m, v, blocks, lrs, wds, beta1, beta2, eps, bc1, bc2, clip=None, fault=None):
    """one fp32 step; blocks: the uint8 group id per 256-block.  fault: None or a planted one (see the tests)"""
    ids = torch.cat([blocks.long(), torch.tensor([3])])              # what lies behind the last id in the tests' parent: 3
    ids = ids[1:] if fault == "neighbour_group" else ids[:-1]
    gid = ids.repeat_interleave(256)
    lr, wd = t32(list(lrs))[gid], t32(list(wds))[gid]
    b1, b2, ep, c1, c2 = t32(beta1), t32(beta2), t32(eps), t32(bc1), t32(bc2)
    gj = g * (t32(clip) if clip is not None and fault != "no_clip" else t32(1.0))
    m1 = b1 * m + (1.0 - b1) * gj
    v1 = b2 * v + (1.0 - b2) * gj * gj
    tf = (rule == "transformers") != (fault == "eps_side")
    if tf:
        u = (lr * torch.sqrt(c2) / c1) * m1 / (torch.sqrt(v1) + ep)
    else:
        u = (lr / c1) * m1 / (torch.sqrt(v1) / torch.sqrt(c2) + ep)
    decay = torch.zeros_like(lr) if fault == "no_decay" else lr * wd
    if (rule == "transformers") != (fault == "decay_first"):
        p1 = p - u
        pn = p1 - decay * p1
    else:
        pn = p * (1.0 - decay) - u
    return pn, m1, v1


# ------------------------------------------------------------------------------------------------------------------------- rownorm
@pytest.mark.parametrize("R,E", S.ROWNORM_SHAPES)
def test_rownorm_emulation_and_faults(R, E):
    c = S.rownorm_case(R, E)
    case = f"{R}x{E}"
    ref = S.rownorm_fwd_ref(c["x"])
    y, iv = emul_rownorm_fwd(c["x"])
    _report("rownorm_fwd", case, "y", S.check_f32(y, *ref["y"], "y"))
    _report("rownorm_fwd", case, "inv", S.check_f32(iv, *ref["inv"], "inv"))
    if R > 1:
        assert float(y[R - 1].abs().max()) == 0.0 and abs(float(iv[R - 1]) - 1e12) <= 1e12 * 2 * U32
    yg, ig = S.rownorm_given(c["x"])
    dref, db = S.rownorm_bwd_ref(c["dy"], yg, ig)
    dx = emul_rownorm_bwd(c["dy"], yg, ig)
    assert bool(torch.isfinite(dx).all())
    _report("rownorm_bwd", case, "dx", S.check_f32(dx, dref, db, "dx"))
    # planted: the last column dropped from the norm / from the dot product; y's last column left unscaled
    xs = c["x"].clone()
    xs[:, E - 1] = 0
    _fails(lambda: S.check_f32(emul_rownorm_fwd(xs)[1], *ref["inv"], "inv without the last column"))
    bad = y.clone()
    bad[:, E - 1] = 0
    _fails(lambda: S.check_f32(bad, *ref["y"], "y, last column zero"))
    ys = yg.clone()
    ys[:, E - 1] = 0
    _fails(lambda: S.check_f32((c["dy"] - yg * lane_sum(c["dy"] * ys).unsqueeze(1)) * ig.unsqueeze(1), dref, db, "dx, dot without the last column"))
    if E >= 256:   # entries k = 3 (mod 4) of the lane's elements dropped: every fourth 64-wide slice
        xs = c["x"].clone()
        xs.reshape(R, E // 64, 64)[:, 3::4] = 0
        _fails(lambda: S.check_f32(emul_rownorm_fwd(xs)[1], *ref["inv"], "inv without slices 3 mod 4"))


# ----------------------------------------------------------------------------------------------------------------------------- itc
def _keeps(N):
    """the planted column faults that exist at N: name -> bool [N] of the columns kept"""
    ar = torch.arange(N)
    out = {}
    if N > 1:
        out["last column"] = ar < N - 1
    if N > 256:
        out["columns >= 256"] = ar < 256
    if N > 3:
        out["columns 3 mod 4"] = ar % 4 != 3
    return out


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("N,E", S.ITC_SHAPES)
def test_itc_emulation_and_faults(N, E, with_idx):
    c = S.itc_case(N, E, with_idx)
    I, idx = c["I"], c["idx"]
    cols, r = S.itc_plants(N)
    for temp in S.ITC_TEMPS:
        tf = S.f32(temp)
        case = f"{N}x{E}:{'idx' if with_idx else 'eye'}:{temp}"
        for j in cols:
            T = S.itc_planted(c, j, r)
            ref = S.itc_fwd_ref(I, T, tf, idx)
            lse, loss = emul_itc_fwd(I, T, temp, idx)
            _report("itc_fwd", case, f"lse:{j}", S.check_f32(lse, *ref["lse"], "lse"))
            _report("itc_fwd", case, f"loss:{j}", S.check_f32(loss, *ref["loss"], "loss"))
            if j is not None and N > 1:   # the planted column lost: row r's lse is off by O(1)
                keep = torch.arange(N) != j
                _fails(lambda: S.check_f32(emul_itc_fwd(I, T, temp, idx, keep)[0], *ref["lse"], f"lse without column {j}"))
        T = c["T"]
        ref = S.itc_fwd_ref(I, T, tf, idx)
        for name, keep in _keeps(N).items():
            _fails(lambda: S.check_f32(emul_itc_fwd(I, T, temp, idx, keep)[0], *ref["lse"], "lse without " + name))
        if N > 1 and temp == 0.5:   # (at temp 0.07 a row's lse - pos is about N exp(-13): the term itself is below the loss's bound)
            _fails(lambda: S.check_f32(emul_itc_fwd(I, T, temp, idx, None, 2 * N - 1)[1], *ref["loss"], "loss without the last row term"))
        # backward from the given statistics
        lse_g = ref["lse"][0].float()
        cnt = ref["cnt"].float() if with_idx else None
        bref = S.itc_bwd_ref(I, T, tf, lse_g, S.f32(S.ITC_G), S.ITC_DTEMP0, idx, cnt)
        dI, dT, dtemp, dtemp_short = emul_itc_bwd(I, T, temp, lse_g, S.ITC_G, S.ITC_DTEMP0, idx, cnt)
        _report("itc_bwd", case, "dI", S.check_f32(dI, *bref["dI"], "dI"))
        _report("itc_bwd", case, "dT", S.check_f32(dT, *bref["dT"], "dT"))
        _report("itc_bwd", case, "dtemp", S.check_f32(dtemp, *bref["dtemp"], "dtemp"))
        if N > 1 and temp == 0.5:
            # (at temp 0.07 the softmax of these rows sits on the positives: G is 1e-5 of its terms, so is every gradient, and a
            # dropped column or row changes them by less than the logits' own E U32 / temp)
            for name, keep in _keeps(N).items():
                bad = emul_itc_bwd(I, T, temp, lse_g, S.ITC_G, S.ITC_DTEMP0, idx, cnt, keep)
                _fails(lambda: S.check_f32(bad[0], *bref["dI"], "dI without " + name))
                _fails(lambda: S.check_f32(bad[1], *bref["dT"], "dT without " + name))
            _fails(lambda: S.check_f32(dtemp_short, *bref["dtemp"], "dtemp without the last row"))
            _fails(lambda: S.check_f32(dtemp - S.ITC_DTEMP0, *bref["dtemp"], "dtemp overwritten, not accumulated"))
        if N > 1:   # rows restricted and chunked: the same numbers as the full reference (the limit shape's path)
            rows = torch.tensor([0, N - 1])
            part = S.itc_bwd_ref(I, T, tf, lse_g, S.f32(S.ITC_G), S.ITC_DTEMP0, idx, cnt, rows=rows, chunk=7)
            for k in ("dI", "dT"):
                assert bool(((part[k][0] - bref[k][0][rows]).abs() <= 1e-6 * bref[k][1][rows]).all()) and torch.allclose(part[k][1], bref[k][1][rows], rtol=1e-9)
            assert abs(float(part["dtemp"][0] - bref["dtemp"][0])) <= 1e-6 * float(bref["dtemp"][1]) and torch.allclose(part["dtemp"][1], bref["dtemp"][1], rtol=1e-9)


# ------------------------------------------------------------------------------------------------------------------------ hard_neg
def test_rng_replica_known_values():
    """the integer replica against values worked out by hand from common.h's definition (32-bit wrap-around at every multiply)"""
    assert S.mix32(0) == 0
    x = 1
    x ^= x >> 16
    x = (x * 0x7feb352d) % (1 << 32)
    x ^= x >> 15
    x = (x * 0x846ca68b) % (1 << 32)
    x ^= x >> 16
    assert S.mix32(1) == x
    assert S.rng_row_key(0, 0, 0) == S.mix32(0x85EBCA6B)
    assert S.rng_row_key(5, 77, 3) == S.mix32((S.mix32(6) + 0x9E3779B9 * 77 + 0x85EBCA6B) % (1 << 32))
    u = S.hard_neg_u((77 << 32) | 5, 3, 2)
    assert float(u[0]) == (S.mix32(S.rng_row_key(5, 77, 3)) >> 8) / 2.0 ** 24 and 0.0 <= float(u.min()) and float(u.max()) < 1.0


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("B,E", S.HARD_NEG_SHAPES)
def test_hard_neg_design_and_faults(B, E, with_idx):
    c = S.hard_neg_case(B, E, with_idx)
    I, T, idx = c["I"], c["T"], c["idx"]
    temp = S.HARD_NEG_TEMP
    case = f"{B}x{E}:{'idx' if with_idx else 'eye'}"
    # 1. the logits are exact in fp32
    assert torch.equal(((I @ T.t()) * (1.0 / t32(temp))).double(), I.double() @ T.double().t() / temp)
    assert torch.equal(emul_logits(I, T, temp).double(), I.double() @ T.double().t() / temp)
    ws = dict(zip(("img", "txt"), S.hard_neg_weights(I, T, temp, idx)))
    seeds = list(S.HARD_NEG_SEEDS) + list(range(2, 17))
    rows = agree = 0
    worst = 0.0
    for side, first in (("img", 0), ("txt", B)):
        w64 = ws[side]
        drawable = w64.sum(1) > 0          # B = 2 with idx: both rows share the id, no row has any weight
        if not bool(drawable.any()):
            continue
        w, cs, wsum = emul_scan(I, T, temp, idx, side)
        for seed in seeds:
            u = S.hard_neg_u(seed, first, B)
            pick = emul_pick(w, cs, wsum, u)
            # 2. every emulated pick lies inside the widened interval (check_draw asserts 3., delta / W <= 1e-4)
            worst = max(worst, S.check_draw(pick[drawable], u[drawable], w64[drawable], f"{side} seed {seed}"))
            rows += int(drawable.sum())
            agree += int((pick == S.draw_exact(u, w64))[drawable].sum())
        if not bool(drawable.all()):
            continue
        # planted faults, first seed with a non-zero low word
        seed = S.HARD_NEG_SEEDS[3]
        u = S.hard_neg_u(seed, first, B)
        if B > 2:
            _fails(lambda: S.check_draw(emul_pick(w, cs, wsum, S.hard_neg_u(seed, first + 1, B)), u, w64, "row r with block r + 1's key"))
        if side == "txt" and B > 2:
            _fails(lambda: S.check_draw(emul_pick(w, cs, wsum, S.hard_neg_u(seed, 0, B)), u, w64, "text rows with blocks [0, B)"))
        for name, keep in _keeps(B).items() if B >= 64 else ():   # (a handful of rows with a handful of choices each proves little)
            fw, fc, fs = emul_scan(I, T, temp, idx, side, keep)
            _fails(lambda: S.check_draw(emul_pick(fw, fc, fs, u), u, w64, "weights without " + name))
    S.report("cpu", "hard_neg", case, "draw", worst)
    print(f"step-ratio cpu hard_neg {case} agree {agree}/{rows}")
    assert worst <= 1.0
    # a serial fp32 scan can part from the fp64 pick only where u W lies within its own error, B U32 W / 2, of one of B edges: 1e-2 of draws
    assert agree >= rows * (1.0 - 2 * B * B * U32 / 2) - 1, f"{agree} of {rows} emulated picks agree with the fp64 pick"


# --------------------------------------------------------------------------------------------------------------------------- adamw
def _adamw_run(rule, n, betas, clip, check, faults=()):
    blocks, gid = S.adamw_groups(n)
    p, m, v = S.adamw_state(n)
    case = f"{rule}:{n}:{betas[1]}:{clip}"
    for step in S.ADAMW_STEPS:
        g = S.adamw_grad(n, step, m, betas[0])
        bc1, bc2 = S.bias_corrections(*betas, step)
        args = (blocks, S.ADAMW_LR, S.ADAMW_WD, betas[0], betas[1], S.ADAMW_EPS, bc1, bc2, clip)
        ref = S.adamw_ref(rule, p, g, m, v, gid, S.ADAMW_LR, S.ADAMW_WD, betas[0], betas[1], S.ADAMW_EPS, bc1, bc2,
                          None if clip is None else S.f32(clip))
        pn, m1, v1 = emul_adamw(rule, p, g, m, v, *args)
        if check:
            for name, got in (("p", pn), ("m", m1), ("v", v1)):
                _report("adamw", case, f"{name}:step{step}", S.check_f32(got, *ref[name], name))
            if n >= 5 * 256:
                z = slice(S.BLK_ZERO * 256, (S.BLK_ZERO + 1) * 256)
                assert float(m1[z].abs().max()) == 0.0 and float(v1[z].abs().max()) == 0.0
        for fault in faults:
            if fault == "eps_side" and 1.0 - S.f32(bc2) ** 0.5 < 0.01:
                continue     # sqrt(bc2) = 1 (beta2 = 0.98 at step 1000): the two sides of the bias correction are the same place
            bad = emul_adamw(rule, p, g, m, v, *args, fault=fault)
            if fault == "no_clip":   # seen in m and v at once, in p one step later
                _fails(lambda: S.check_f32(bad[1], *ref["m"], f"m, {fault}, step {step}"))
            else:
                _fails(lambda: S.check_f32(bad[0], *ref["p"], f"p, {fault}, step {step}"))
        p, m, v = pn, m1, v1


@pytest.mark.parametrize("rule", ["transformers", "torch"])
@pytest.mark.parametrize("n", S.ADAMW_SIZES)
def test_adamw_emulation_within_bounds(rule, n):
    for betas, clip, _ in (S.ADAMW_OPTIONS if n < 1 << 20 else S.ADAMW_OPTIONS[:1]):
        _adamw_run(rule, n, betas, clip, True)


@pytest.mark.parametrize("rule", ["transformers", "torch"])
@pytest.mark.parametrize("n", S.ADAMW_SIZES[:2])
def test_adamw_planted_faults_are_caught(rule, n):
    # n = 256 is one block of group 0 without planted gradients: lr wd = 1e-5 makes the order of decay and update a 1e-8 matter, and no
    # gradient is near eps; those two faults are planted at n = 1280 (group 1: lr wd = 6e-4; the |g| = 1e-8 block)
    faults = ["no_decay", "neighbour_group"]
    if n >= 5 * 256:
        faults += ["eps_side"] + (["decay_first"] if rule == "transformers" else [])
    _adamw_run(rule, n, (0.9, 0.999), None, False, faults)
    _adamw_run(rule, n, (0.9, 0.98), 0.5, False, faults + ["no_clip"])


def test_max_norm_check_misses_the_decay_the_bound_catches():
    """why these bounds exist, kept as a test: the transformers-rule output WITHOUT its decay is within 1e-4 of max |p| of the reference
    (the existing kernel test's tolerance) after each of two steps, and past the elementwise bound"""
    n = 1280
    blocks, gid = S.adamw_groups(n)
    p, m, v = S.adamw_state(n)
    for step in (1, 2):
        g = S.adamw_grad(n, step, m, 0.9)
        bc1, bc2 = S.bias_corrections(0.9, 0.999, step)
        args = (blocks, (1e-3,) * 4, (0.01,) * 4, 0.9, 0.999, S.ADAMW_EPS, bc1, bc2)     # that test's lr and decay, in every group
        ref, b32 = S.adamw_ref("transformers", p, g, m, v, gid, *args[1:])["p"]
        bad, m1, v1 = emul_adamw("transformers", p, g, m, v, *args, fault="no_decay")
        assert float((bad.double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())
        _fails(lambda: S.check_f32(bad, ref, b32, "decay omitted"))
        p, m, v = emul_adamw("transformers", p, g, m, v, *args)


# --------------------------------------------------------------------------------------------------------------------------- sumsq
@pytest.mark.parametrize("n", S.SUMSQ_SIZES)
def test_sumsq_emulation_and_faults(n):
    x = S.randn((n,), 1.0, 350)
    for out0 in (0.0, 3.0):
        ref, b = S.sumsq_ref(x, out0)
        q = x * x
        part = q.reshape(-1, 4).sum(1)                      # one thread's four elements
        got = (t32(out0) + part.sum()).reshape(1)
        _report("sumsq", str(n), f"out0={out0}", S.check_f32(got, ref, b, "sumsq"))
        if n < 2048:   # (four squares of a million are below the million roundings granted)
            _fails(lambda: S.check_f32((t32(out0) + part[:-1].sum()).reshape(1), ref, b, "sumsq without the last four elements"))
        if out0 and n < 2048:
            _fails(lambda: S.check_f32(part.sum().reshape(1), ref, b, "sumsq overwritten, not accumulated"))
        if n > 1024:
            _fails(lambda: S.check_f32((t32(out0) + q[:1024].sum()).reshape(1), ref, b, "sumsq without a second grid-stride trip"))


def test_limits_mirror_the_sources():
    """the constants the tests size their buffers and limit shapes by are the library's"""
    from xfm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "xfm_hip.h")) as f:
        assert f"#define XFM_SUMSQ_WORKSPACE_FLOATS {_lib.SUMSQ_WORKSPACE_FLOATS}\n" in f.read()
    with open(os.path.join(root, "xfm_amd", "csrc", "contrastive.hip")) as f:
        src = f.read()
    assert f"#define XFM_LOSS_MAXN {S.LOSS_MAXN}\n" in src
    assert all(f"case {E // 64}: {{ constexpr int EPL = {E // 64};" in src for E in S.WIDTHS) and src.count("constexpr int EPL") == len(S.WIDTHS)
