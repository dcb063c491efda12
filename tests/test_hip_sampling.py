"""xfm_sample_token (csrc/decode.hip) on a real MI355X against the fp64 restatement of sample_util, inside poisoned buffers: NaN in the
logit columns past V and in the rows around the logits, sentinels around every output.  Checked per launch: `filtered` (the
restatement's z where kept, within the rounding of the penalty and of the temperature divide; -inf elsewhere), the kept set (equal on
sharp rows, a prefix of the tie-ruled order with a length inside the DELTA band otherwise), the token against the fp64 running sum over
the kernel's own kept set, the log-probability within its derived bound, next_token_ref's bookkeeping, untouched inputs and
surroundings, and equal bits from two launches.  The device generator is checked by chi-squared tests over rows and over steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from decode_util import next_token_ref  # noqa: E402
from gemm_strided_util import NAN, SENTINEL, check_f32  # noqa: E402
from sample_util import draw_ref, filter_ref, lp_bound, row_is_bad, tempered64, token_accepted  # noqa: E402

F32, I32, I64 = torch.float32, torch.int32, torch.int64
NEG = -float("inf")
SHAPES = (1, 2, 63, 64, 65, 257, 4099, 50265, 131072)
MAXLEN, STEPS, STEP = 9, 4, 2


def combos(V):
    """(top_k, top_p, temperature, penalty, B, cur_len): every top_k of {0, 1, 5, V, V + 7}, top_p of {1, 0.9, 0.5, 1e-6}, temperature
    of {1, 0.7, 2.5}, penalty of {1, 1.3} and B of {1, 5} occurs; the no-filter path, each select alone and both together; cur_len 0."""
    return ((0, 1.0, 1.0, 1.0, 5, 6), (1, 1.0, 0.7, 1.3, 5, 6), (5, 0.9, 1.0, 1.0, 5, 6), (V, 0.5, 2.5, 1.3, 5, 6), (V + 7, 1e-6, 1.0, 1.0, 1, 6),
            (0, 0.9, 0.7, 1.3, 5, 0), (0, 0.5, 1.0, 1.0, 1, 6), (5, 1.0, 2.5, 1.0, 1, 6), (50, 0.9, 0.7, 1.3, 5, 6), (1, 1e-6, 2.5, 1.0, 5, 6))


def make_case(V, B, seed):
    """-> (x fp32 [B, ld] with NaN past V, ids [B, MAXLEN], unfinished, u, eos, sharp rows).  B = 5: row 0 two equal maxima and four equal
    values one below them (equal values across a top-k cut of 1 or 5, and inside the nucleus); row 1 -inf entries, at both ends and every
    third column; row 2 ONE finite entry; row 3 already finished, flat (standard normal: many positions inside the top-p band); row 4
    plain, with duplicated ids on a positive and a negative logit.  Ids outside [0, V) sit in rows 0 and 1.  B = 1: a plain row."""
    ld = (V + 63) // 64 * 64
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = 4.0 * torch.randn((B, ld), generator=g)
    x[:, V:] = NAN
    ids = torch.randint(0, V, (B, MAXLEN), generator=g)
    ids[:, 6:] = -7
    u = torch.rand(B, generator=g).float().clamp(max=1 - 2.0 ** -24)
    eos = [min(5, V - 1), min(3, max(V - 2, 0))]
    if B == 1:
        return x, ids, torch.ones(1, dtype=I32), u, eos, []
    hi = float(x[:, :V].max()) + 12.0   # far above the rest: the planted columns carry the mass at every temperature used
    if V >= 8:
        x[0, 1] = x[0, V - 2] = hi
        x[0, 2] = x[0, 3] = x[0, V // 2] = x[0, V - 3] = hi - 1.0
    elif V == 2:
        x[0, 0] = x[0, 1] = hi
    if V >= 4:
        x[1, 0] = x[1, V - 1] = NEG
        x[1, 2:V:3] = NEG
    keep = x[2, V // 3].clone()
    x[2, :V] = NEG
    x[2, V // 3] = keep
    x[3, :V] *= 0.25
    if V > 6:
        x[4, 2], x[4, 4] = hi - 2.0, -1.0
        ids[4, :4] = torch.tensor([2, 4, 2, 4])
    ids[0, 0], ids[1, 1] = V + 3, -7
    u[0], u[3] = 1 - 2.0 ** -24, 0.0
    return x, ids, torch.tensor([1, 1, 1, 0, 1], dtype=I32), u, eos, [0, 2] if V >= 8 else [2]   # (V = 2: two halves ON a top_p of 0.5)


def run_kernel(x, V, ids, cur_len, unfinished, u, eos, pad, top_k, top_p, T, penalty, seed=0, use_uniforms=True):
    """One launch inside poisoned parents -> dict of CPU tensors (the parents whole)."""
    from xfm_amd import functional as Fx
    dev = torch.device("cuda")
    B, ld = x.shape
    xp = torch.full((B + 2, ld), NAN, dtype=F32)
    xp[1:B + 1] = x
    g_xp = xp.to(dev)
    fp = torch.full((B + 2, ld + 8), SENTINEL, dtype=F32, device=dev)
    g_ids, g_unf = ids.to(dev), unfinished.to(dev)
    hist_u = torch.full((B, STEPS), -3, dtype=I32, device=dev)
    hist_lp = torch.full((B, STEPS), SENTINEL, dtype=F32, device=dev)
    count = torch.tensor([100], dtype=I32, device=dev)
    Fx.sample_token(g_xp[1:B + 1], V, g_ids, cur_len, g_unf, hist_u, hist_lp, STEP, pad, eos, T, top_k, top_p, seed, penalty=penalty,
                    n_unfinished=count, uniforms=u.to(dev) if use_uniforms else None, filtered=fp[1:B + 1])
    torch.cuda.synchronize()
    return dict(xp=g_xp.cpu(), xp0=xp, fp=fp.cpu(), ids=g_ids.cpu(), unf=g_unf.cpu(), hist_u=hist_u.cpu(), hist_lp=hist_lp.cpu(), count=int(count))


def check_launch(V, x, ids, cur_len, unfinished, u, eos, pad, top_k, top_p, T, penalty, sharp, out, what):
    B, ld = x.shape
    z, b_z = tempered64(x, V, ids, cur_len, penalty, T)
    # nothing but the written columns changed
    assert torch.equal(out["xp"].view(I32), out["xp0"].view(I32)), f"{what}: the logits were modified"
    fp = out["fp"]
    assert bool((fp[0] == SENTINEL).all() and (fp[B + 1] == SENTINEL).all() and (fp[:, V:] == SENTINEL).all()), f"{what}: filtered written outside [0, V)"
    want_ids = ids.clone()
    want_ids[:, cur_len] = out["ids"][:, cur_len]
    assert torch.equal(out["ids"], want_ids), f"{what}: ids written outside column cur_len"
    other = [c for c in range(STEPS) if c != STEP]
    assert bool((out["hist_u"][:, other] == -3).all()) and bool((out["hist_lp"][:, other] == SENTINEL).all()), f"{what}: history outside column step"
    filt = fp[1:B + 1, :V]
    toks, lps, b_lps = [], [], []
    for b in range(B):
        assert not row_is_bad(z[b])
        f = filter_ref(z[b], top_k, top_p)
        finite = torch.isfinite(z[b])
        kept = torch.isfinite(filt[b])
        # values: z where kept (within the rounding of the penalty and the divide), -inf elsewhere
        assert bool((filt[b][~kept] == NEG).all()), f"{what} row {b}: a removed column is not -inf"
        check_f32(filt[b][kept], z[b][kept], b_z[b][kept], f"{what} row {b}: filtered values")
        # the kept set: a prefix of the tie-ruled order whose length lies in the band (sharp rows: n_lo == n_hi, so equal)
        n_fin = int(finite[f["order"]].sum())   # the -inf columns sort last and carry nothing
        n_lo, n_hi, n = min(f["n_lo"], n_fin), min(f["n_hi"], n_fin), int(kept.sum())
        if b in sharp:
            assert n_lo == n_hi, f"{what} row {b}: meant to be sharp, band [{n_lo}, {n_hi}]"
        assert n_lo <= n <= n_hi, f"{what} row {b}: {n} kept, band [{n_lo}, {n_hi}]"
        want = torch.zeros(V, dtype=torch.bool)
        want[f["order"][:n]] = True
        assert torch.equal(kept, want), f"{what} row {b}: the kept set is not the first {n} of the order"
        if top_k > 0 and not bool(f["topk"].all()):   # the cut of top-k is decided by more than the rounding of z
            below = z[b][~f["topk"]]
            t = z[b][f["topk"]].min()
            assert not below.numel() or float(t - below.max()) > 4 * float(b_z[b].max()), f"{what} row {b}: top-k cut too close to call"
        # the token: inside the fp64 running sum over the kernel's own kept set
        ub = float(u[b])
        d = draw_ref(z[b], kept, ub)
        if int(unfinished[b]):
            tok = int(out["ids"][b, cur_len])
            assert 0 <= tok < V and token_accepted(d["C"], kept, tok, ub), f"{what} row {b}: token {tok} for u = {ub} (fp64 draws {d['tok']})"
        else:   # a finished row shows a pad: its token is known through u = 0, the first kept column with weight
            assert int(out["ids"][b, cur_len]) == pad
            tok = d["tok"]
        lp, b_lp = lp_bound(z[b], b_z[b], kept, tok)
        toks.append(tok)
        lps.append(lp)
        b_lps.append(b_lp)
    ratio = check_f32(out["hist_lp"][:, STEP].contiguous(), torch.tensor(lps, dtype=torch.float64), torch.tensor(b_lps, dtype=torch.float64),
                      f"{what}: log-probability")
    r = next_token_ref(torch.zeros(B, V), V, ids, cur_len, 1.0, unfinished, pad, eos, next_token=torch.tensor(toks))
    assert out["ids"][:, cur_len].tolist() == r["add"].tolist()
    assert out["unf"].tolist() == r["unfinished"].tolist() and out["hist_u"][:, STEP].tolist() == r["flag"].tolist()
    assert out["count"] == 100 + r["count"]
    return ratio


@pytest.mark.parametrize("V", SHAPES)
def test_sample_token_against_fp64(V):
    pad = 1 if V > 2 else 0
    worst = 0.0
    for i, (top_k, top_p, T, penalty, B, cur_len) in enumerate(combos(V)):
        x, ids, unfinished, u, eos, sharp = make_case(V, B, 1000 * i + V)
        what = f"sample_token V={V} B={B} top_k={top_k} top_p={top_p} T={T} penalty={penalty} cur_len={cur_len}"
        outs = [run_kernel(x, V, ids, cur_len, unfinished, u, eos, pad, top_k, top_p, T, penalty) for _ in range(2)]
        for k in ("fp", "ids", "unf", "hist_u", "hist_lp"):
            a, b = outs[0][k], outs[1][k]
            assert torch.equal(a.view(I32) if a.dtype == F32 else a, b.view(I32) if b.dtype == F32 else b), f"{what}: {k} differs between two launches"
        worst = max(worst, check_launch(V, x, ids, cur_len, unfinished, u, eos, pad, top_k, top_p, T, penalty, sharp, outs[0], what))
    print(f"sample_token V={V}: log-prob worst err / bound {worst:.3g}")


def test_rows_without_a_distribution():
    """No finite value, a NaN, a +inf: token 0 and a NaN score, the bookkeeping as for any token; the good row beside them is unharmed."""
    V = 257
    x, ids, unfinished, u, eos, _ = make_case(V, 5, 77)
    x[0, :V] = NEG
    x[1, 100] = NAN
    x[4, 7] = float("inf")
    unfinished = torch.ones(5, dtype=I32)
    out = run_kernel(x, V, ids, 6, unfinished, u, eos, 1, 5, 0.9, 0.7, 1.0)
    assert out["ids"][[0, 1, 4], 6].tolist() == [0, 0, 0] and bool(torch.isnan(out["hist_lp"][[0, 1, 4], STEP]).all())
    assert torch.equal(out["xp"].view(I32), out["xp0"].view(I32)) and bool((out["fp"][:, V:] == SENTINEL).all())
    z, b_z = tempered64(x, V, ids, 6, 1.0, 0.7)
    f = filter_ref(z[2], 5, 0.9)
    assert torch.equal(torch.isfinite(out["fp"][3, :V]), f["kept"]) and int(out["ids"][2, 6]) == V // 3
    assert bool(torch.isfinite(out["hist_lp"][[2, 3], STEP]).all())
    r = next_token_ref(torch.zeros(5, V), V, ids, 6, 1.0, unfinished, 1, eos, next_token=out["ids"][:, 6].clone())
    assert out["unf"].tolist() == r["unfinished"].tolist() and out["count"] == 100 + r["count"]


def _chi2_ok(obs, p, what):
    """Pearson chi-squared of counts against probabilities; cells whose expected count is below 5 are merged into one."""
    from scipy.stats import chi2
    n = obs.sum()
    exp = p * n
    small = exp < 5
    o = np.concatenate([obs[~small], [obs[small].sum()]]) if small.any() else obs
    e = np.concatenate([exp[~small], [exp[small].sum()]]) if small.any() else exp
    o, e = o[e > 0], e[e > 0]
    stat, dof = float(((o - e) ** 2 / e).sum()), len(e) - 1
    limit = float(chi2.ppf(1 - 1e-6, dof))
    print(f"{what}: chi2 = {stat:.1f} over {dof} degrees of freedom (limit {limit:.1f})")
    assert stat < limit, f"{what}: chi2 = {stat:.1f} over {dof} degrees of freedom (limit {limit:.1f})"


def test_device_generator_follows_the_softmax():
    """4 096 identical rows at V = 64 in one launch, then one row over 4 096 steps: both token counts follow the restatement's softmax
    over the kept set (chi-squared at 1 - 1e-6); another seed draws other tokens."""
    from xfm_amd import functional as Fx
    V, N, T, top_k = 64, 4096, 0.7, 20
    dev = torch.device("cuda")
    row = 2.0 * torch.randn((1, V), generator=torch.Generator(device="cpu").manual_seed(3))
    z, _ = tempered64(row, V, torch.zeros(1, 1, dtype=I64), 0, 1.0, T)
    kept = filter_ref(z[0], top_k, 1.0)["kept"]
    p = torch.softmax(torch.where(kept, z[0], torch.full_like(z[0], NEG)), 0).numpy()
    draws = {}
    for seed in (11, 2 ** 40 + 5):
        ids = torch.zeros((N, 1), dtype=I64, device=dev)
        Fx.sample_token(row.expand(N, V).contiguous().to(dev), V, ids, 0, torch.ones(N, dtype=I32, device=dev), torch.zeros((N, 1), dtype=I32, device=dev),
                        torch.zeros((N, 1), dtype=F32, device=dev), 0, 1, [], T, top_k, 1.0, seed)
        draws[seed] = ids.cpu()[:, 0]
        assert bool(kept[draws[seed]].all())
        _chi2_ok(np.bincount(draws[seed].numpy(), minlength=V).astype(np.float64), p, f"rows, seed {seed}")
    assert not torch.equal(draws[11], draws[2 ** 40 + 5])
    g_row = row.to(dev)
    ids = torch.zeros((1, N), dtype=I64, device=dev)
    unf, hu, hl = torch.ones(1, dtype=I32, device=dev), torch.zeros((1, N), dtype=I32, device=dev), torch.zeros((1, N), dtype=F32, device=dev)
    for step in range(N):
        Fx.sample_token(g_row, V, ids, step, unf, hu, hl, step, 1, [], T, top_k, 1.0, 11)
    steps = ids.cpu()[0]
    _chi2_ok(np.bincount(steps.numpy(), minlength=V).astype(np.float64), p, "steps, seed 11")
    assert int(steps[0]) == int(draws[11][0]), "row 0 at step 0 is one draw, whatever the batch"
    assert not torch.equal(steps, draws[11])
