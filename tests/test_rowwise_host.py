"""The row-kernel bounds (rowwise_util) are neither vacuous nor too tight, shown on the CPU.  For every input generator and shape of
tests/test_hip_layernorm_bounds.py and tests/test_hip_ce_bounds.py a straightforward fp32 evaluation of each formula (LayerNorm sums: 64
lane partials, then across them; the GELU with common.h's polynomial) stays within 0.75 of its fp32 bound and, rounded to bf16, within 1.0
of the bf16 bound; every planted fault on such an output lands past the bound.  The worst ratios are printed (pytest -s) as
`rowwise-ratio cpu <kernel> <mode> <width> <quantity> <ratio>` lines; profiles/tests_rowwise_bounds.md sets them next to the MI355X's."""
import math

import pytest
import torch

import rowwise_util as R
from rowwise_util import BF16, F32, U32, gelu_parts32

CPU_F32_MAX, CPU_BF16_MAX = 0.75, 1.0


def _report(kernel, mode, width, what, ratio, limit):
    print(f"rowwise-ratio cpu {kernel} {mode} {width} {what} {ratio:.3g}")
    assert ratio <= limit, f"{kernel} {mode} {width} {what}: emulation at {ratio:.3g} of the bound (limit {limit})"


# ------------------------------------------------------------------------------------------------------------------ fp32 emulations
def lane_sum(t):
    """[rows, D] -> [rows]: lane l adds its elements of every 64-wide slice in turn, then a halving tree across the 64 lanes"""
    rows, D = t.shape
    lanes = t.reshape(rows, D // 64, 64)
    acc = lanes[:, 0].clone()
    for i in range(1, D // 64):
        acc = acc + lanes[:, i]
    n = 64
    while n > 1:
        n //= 2
        acc = acc[:, :n] + acc[:, n:2 * n]
    return acc[:, 0]


def emul_ln_fwd(v, w, b, eps, gelu=False):
    D = v.shape[1]
    inv = torch.tensor(1.0 / D, dtype=F32)
    mu = lane_sum(v) * inv
    d = v - mu.unsqueeze(1)
    rstd = torch.rsqrt(lane_sum(d * d) * inv + eps)
    y = d * rstd.unsqueeze(1) * w + b
    if gelu:
        y = y * gelu_parts32(y)[0]
    return mu, rstd, y


def emul_ln_bwd(dy_parts, xs, mean, rstd, w, gelu_b=None):
    D = xs.shape[1]
    dy = dy_parts[0].float()
    for p in dy_parts[1:]:
        if p is not None:
            dy = dy + p.float()
    xh = (xs.float() - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    if gelu_b is not None:
        u = xh * w + gelu_b
        cdf, pdf = gelu_parts32(u)
        dy = dy * (u * pdf + cdf)
    g = dy * w
    inv = torch.tensor(1.0 / D, dtype=F32)
    c1, c2 = lane_sum(g) * inv, lane_sum(g * xh) * inv
    dz = rstd.unsqueeze(1) * (g - c1.unsqueeze(1) - xh * c2.unsqueeze(1))
    return dz, dy, xh


def emul_ce_bwd(x, lse32, t, tsum, scale):
    p = torch.exp(x - lse32.unsqueeze(1))
    return (tsum.float().unsqueeze(1) * p - t.float()) * scale.reshape(-1, 1)


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_cases():
    out = [(D, m, rows) for D in R.LN_NARROW for m in R.LN_MODES for rows in (R.small_rows(D, m), R.ROWS_BIG)]
    out += [(D, m, rows) for D in R.LN_WIDE for m in ("plain32", "plain16") for rows in (R.small_rows(D, m), R.ROWS_BIG)]
    return out + [(256, "plain32", R.ROWS_GRID), (256, "ls", R.ROWS_GRID)]


@pytest.mark.parametrize("D,mode,rows", _ln_cases())
def test_ln_forward_emulation_within_bounds(D, mode, rows):
    c = R.ln_case(D, mode, rows)
    X, x_err = R.ln_row(c)
    v = R.ln_row_f32(c)
    if x_err is not None:
        _report("ln_fwd", mode, D, "row32", R.check_f32(v, X, x_err, "row"), CPU_F32_MAX)
        _report("ln_fwd", mode, D, "row16", R.check_bf16(v.to(BF16), X, x_err, "row bf16"), CPU_BF16_MAX)
    for gelu in (False, True):
        ref = R.ln_fwd_ref(X, c["w"], c["b"], R.EPS, x_err, gelu)
        mu, rstd, y = emul_ln_fwd(v, c["w"], c["b"], R.EPS, gelu)
        assert bool(torch.isfinite(y).all())
        tag = "gelu" if gelu else "y"
        _report("ln_fwd", mode, D, "mean", R.check_f32(mu, *ref["mean"], "mean"), CPU_F32_MAX)
        _report("ln_fwd", mode, D, "rstd", R.check_f32(rstd, *ref["rstd"], "rstd"), CPU_F32_MAX)
        _report("ln_fwd", mode, D, tag + "32", R.check_f32(y, *ref["y"], tag), CPU_F32_MAX)
        _report("ln_fwd", mode, D, tag + "16", R.check_bf16(y.to(BF16), *ref["y"], tag + " bf16"), CPU_BF16_MAX)


@pytest.mark.parametrize("D,mode,rows", _ln_cases())
def test_ln_backward_emulation_within_bounds(D, mode, rows):
    c = R.ln_case(D, mode, rows)
    xs = R.ln_stored(c)
    mean, rstd = R.ln_stats(xs)
    variants = [("dx", [c["dy1"]], None), ("dx_sum", [c["dy1"], c["dy2"], c["dy32"]], None)]
    if mode.startswith("plain"):
        variants.append(("dx_gelu", [c["dy1"]], c["b"]))
    for tag, parts, gb in variants:
        ref = R.ln_bwd_ref(parts, xs, mean, rstd, c["w"], gb)
        dz, dy, xh = emul_ln_bwd(parts, xs, mean, rstd, c["w"], gb)
        _report("ln_bwd", mode, D, tag + "32", R.check_f32(dz, *ref["dx"], tag), CPU_F32_MAX)
        _report("ln_bwd", mode, D, tag + "16", R.check_bf16(dz.to(BF16), *ref["dx"], tag + " bf16"), CPU_BF16_MAX)
        DY, e_dy = ref["dy"]
        dg_ref, dg_b = R.colsum_bound(DY * ref["xh"], e_dy * ref["xh"].abs(), 0.5)
        db_ref, db_b = R.colsum_bound(DY, e_dy, 0.25)
        _report("ln_bwd", mode, D, tag + ":dgamma", R.check_f32(0.5 + (dy * xh).sum(0), dg_ref, dg_b, "dgamma"), CPU_F32_MAX)
        _report("ln_bwd", mode, D, tag + ":dbeta", R.check_f32(0.25 + dy.sum(0), db_ref, db_b, "dbeta"), CPU_F32_MAX)
    if mode == "plain32":   # dx_accum
        dx, bdx = ref["dx"]
        _report("ln_bwd", mode, D, "dx_accum", R.check_f32(c["dx0"] + dz, dx + c["dx0"].double(), bdx + U32 * c["dx0"].double().abs(), "accum"),
                CPU_F32_MAX)
    if mode == "ls":        # the stream add, dh = s gamma o, dls = sum_r s h o
        ref = R.ln_bwd_ref([c["dy1"]], xs, mean, rstd, c["w"])
        dz, _, _ = emul_ln_bwd([c["dy1"]], xs, mean, rstd, c["w"])
        dx, bdx = ref["dx"]
        o = c["dx0"] + dz
        o_ref = dx + c["dx0"].double()
        b_o = bdx + U32 * o_ref.abs()
        _report("ln_bwd", mode, D, "dstream", R.check_f32(o, o_ref, b_o, "dstream"), CPU_F32_MAX)
        s = R.row_scale_of(c["row_scale"], rows, c["rps"], "cpu")
        sg = s * c["ls_gamma"].double()
        dh = (s.float() * c["ls_gamma"] * o).to(BF16)
        _report("ln_bwd", mode, D, "dh16", R.check_bf16(dh, sg * o_ref, sg.abs() * b_o + 3 * U32 * (sg * o_ref).abs(), "dh"), CPU_BF16_MAX)
        dls = 0.5 + (s.float() * c["h"].float() * o).sum(0)
        _report("ln_bwd", mode, D, "dls", R.check_f32(dls, *R.colsum_bound(s * c["h"].double() * o.double(), None, 0.5), "dls"), CPU_F32_MAX)
    if mode.startswith("post"):
        dh = dz.to(BF16)
        _report("ln_bwd", mode, D, "dbias", R.check_f32(0.5 + dh.float().sum(0), *R.colsum_bound(dh, None, 0.5), "dbias"), CPU_F32_MAX)


def _fails(fn, match="past the bound"):
    with pytest.raises(AssertionError, match=match):
        fn()


@pytest.mark.parametrize("D,mode", [(256, "plain32"), (768, "post16"), (1536, "ls"), (8192, "plain16")])
def test_ln_planted_faults_are_caught(D, mode):
    rows = R.ROWS_BIG
    c = R.ln_case(D, mode, rows)
    X, x_err = R.ln_row(c)
    ref = R.ln_fwd_ref(X, c["w"], c["b"], R.EPS, x_err)
    mu, rstd, y = emul_ln_fwd(R.ln_row_f32(c), c["w"], c["b"], R.EPS)
    y16 = y.to(BF16)
    R.check_bf16(y16, *ref["y"], "sound")
    # one element off by 2 bf16 ulps (row 0 is a randn * 2 row; the element of largest |y| there)
    col = int(y[0].abs().argmax())
    bad = y16.clone()
    bits = bad.view(torch.int16)
    bits[0, col] += 2
    _fails(lambda: R.check_bf16(bad, *ref["y"], "2 ulps"))
    # the last 4-column granule zeroed; one 256-column chunk taken from its neighbour
    bad = y16.clone()
    bad[:, D - 4:] = 0
    _fails(lambda: R.check_bf16(bad, *ref["y"], "last granule"))
    if D >= 512:
        for t, chk in ((y, R.check_f32), (y16, R.check_bf16)):
            bad = t.clone()
            bad[:, 256:512] = t[:, 0:256]
            _fails(lambda: chk(bad, *ref["y"], "chunk 1 from chunk 0"))
    # last column zeroed, fp32 twin
    bad = y.clone()
    bad[:, D - 1] = 0
    _fails(lambda: R.check_f32(bad, *ref["y"], "last column"))
    # mean off by 4 em
    _fails(lambda: R.check_f32((ref["mean"][0] + 4 * ref["mean"][1]).float(), *ref["mean"], "mean + 4 em"))
    # dgamma missing one row
    xs = R.ln_stored(c)
    mean, rs = R.ln_stats(xs)
    bref = R.ln_bwd_ref([c["dy1"]], xs, mean, rs, c["w"])
    dz, dy, xh = emul_ln_bwd([c["dy1"]], xs, mean, rs, c["w"])
    dg_ref, dg_b = R.colsum_bound(bref["dy"][0] * bref["xh"], None, 0.5)
    R.check_f32(0.5 + (dy * xh).sum(0), dg_ref, dg_b, "sound dgamma")
    _fails(lambda: R.check_f32(0.5 + (dy * xh)[:-1].sum(0), dg_ref, dg_b, "dgamma without the last row"))
    _fails(lambda: R.check_f32(0.25 + dy[1:].sum(0), *R.colsum_bound(bref["dy"][0], None, 0.25), "dbeta without the first row"))
    if mode == "ls":   # sample 1 normalised with sample 0's row_scale
        wrong = dict(c)
        wrong["row_scale"] = c["row_scale"].clone()
        wrong["row_scale"][1] = c["row_scale"][0]
        v = R.ln_row_f32(wrong)
        _fails(lambda: R.check_f32(v, X, x_err, "x' with the neighbour's row_scale"))
        _fails(lambda: R.check_f32(emul_ln_fwd(v, c["w"], c["b"], R.EPS)[2], *ref["y"], "y with the neighbour's row_scale"))


def test_outside_rows_one_bit():
    """one changed bit in the row before and in the row after an output's rows"""
    for dtype in (F32, BF16):
        v, p = R.embed(torch.zeros((5, 256), dtype=dtype), 256, 0, 4, 4, R.SENTINEL)
        R.assert_outside_untouched(p, v, R.SENTINEL)
        it = torch.int32 if dtype == F32 else torch.int16
        for r in (3, 9):
            q = p.clone()
            q.view(it)[r, 100] ^= 1
            _fails(lambda: R.assert_outside_untouched(q, q[4:9], R.SENTINEL, "row"), "outside the view")


# --------------------------------------------------------------------------------------------------------------------- cross-entropy
def _ce_lse32(x):
    mx = x.max(1).values
    return mx + torch.log(torch.exp(x - mx.unsqueeze(1)).sum(1))


@pytest.mark.parametrize("Rr,V,ld", R.CE_SHAPES)
def test_ce_emulation_within_bounds_and_faults_caught(Rr, V, ld):
    c = R.ce_case(Rr, V)
    x = c["x"]
    for form in R.CE_FORMS:
        t, tsum, valid = R.ce_target(c, form, V)
        lse, b_lse, loss, b_loss = R.ce_fwd_ref(x, t, tsum, valid)
        l32 = _ce_lse32(x)
        _report("ce_fwd", form, V, "lse", R.check_f32(l32, lse, b_lse, "lse"), CPU_F32_MAX)
        loss32 = l32 * tsum.float() - (t.float() * x).sum(1)
        if valid is not None:
            loss32 = torch.where(valid, loss32, torch.zeros_like(loss32))
        _report("ce_fwd", form, V, "loss", R.check_f32(loss32, loss, b_loss, "loss"), CPU_F32_MAX)
        for sname in ("scale1", "scaleR"):
            ref, b32 = R.ce_bwd_ref(x, l32, t, tsum, c[sname], valid)
            d = emul_ce_bwd(x, l32, t, tsum, c[sname])
            if valid is not None:
                d = torch.where(valid.unsqueeze(1), d, torch.zeros_like(d))
            _report("ce_bwd", form, V, sname + ":d32", R.check_f32(d, ref, b32, "dlogits"), CPU_F32_MAX)
            d16 = d.to(BF16)
            _report("ce_bwd", form, V, sname + ":d16", R.check_bf16(d16, ref, b32, "dlogits bf16"), CPU_BF16_MAX)
            if valid is not None and Rr <= 3:
                continue   # rows 0 and 1 are the times-30 and the 100-above rows, whose small entries flush, row 2 is ignored: no plain row
            # planted faults
            bad = d16.clone()
            bad[:, V - 1] = 0
            _fails(lambda: R.check_bf16(bad, ref, b32, "last column zeroed"))
            bad = d16.clone()
            bad[:, max(V - 4, 0):] = 0
            _fails(lambda: R.check_bf16(bad, ref, b32, "last granule zeroed"))
            if V >= 512:
                bad = d16.clone()
                bad[:, 256:512] = d16[:, 0:256]
                _fails(lambda: R.check_bf16(bad, ref, b32, "chunk 1 from chunk 0"))
            if form == "onehot":
                lab = t > 0
                bad = torch.where(lab, d, d * 1.02).to(BF16)
                _fails(lambda: R.check_bf16(bad, ref, b32, "non-label entries times 1.02"))
    # the planted maximum: a forward that loses its column is off by O(1), far past the lse bound
    lab0 = int(c["labels"][0])
    for col in R.plant_columns(V, lab0):
        xp = x.clone()
        xp[:, col] = xp.max(1).values + 20.0
        t, tsum, valid = R.ce_target(c, "onehot", V)
        lse, b_lse, loss, b_loss = R.ce_fwd_ref(xp, t, tsum, valid)
        R.check_f32(_ce_lse32(xp), lse, b_lse, "lse, planted")
        if V > 1:
            lost = xp.clone()
            lost[:, col] = -1e30
            _fails(lambda: R.check_f32(_ce_lse32(lost), lse, b_lse, f"lse without column {col}"))


def test_max_norm_check_misses_what_the_bound_catches():
    """why these bounds exist, kept as a test: a zeroed last column of dlogits at V = 50265 is invisible to max-error / max|ref| <= 1e-2"""
    Rr, V, _ = R.CE_SHAPES[0]
    c = R.ce_case(Rr, V)
    t, tsum, valid = R.ce_target(c, "onehot", V)
    l32 = _ce_lse32(c["x"])
    ref, b32 = R.ce_bwd_ref(c["x"], l32, t, tsum, c["scale1"], valid)
    d = torch.where(valid.unsqueeze(1), emul_ce_bwd(c["x"], l32, t, tsum, c["scale1"]), torch.zeros(())).to(BF16)
    d[:, V - 1] = 0
    assert float((d.double() - ref).abs().max() / ref.abs().max()) < 1e-2
    _fails(lambda: R.check_bf16(d, ref, b32, "last column zeroed"))
    assert math.isfinite(float(b32.max()))
