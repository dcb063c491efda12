"""The token-path bounds (token_rows_util) are neither vacuous nor too tight, shown on the CPU: for every case of
tests/test_hip_embedding_bounds.py and tests/test_hip_token_rows_bounds.py a plain fp32 evaluation of each formula (torch in float32, bf16
rounding where the kernel stores bf16; the LayerNorm sums of tests/test_rowwise_host.py) goes through the same check_* functions as the
kernels' outputs and stays within 0.75 of every fp32 bound and 1.0 of every bf16 bound; every case has the property it is there to reach
(recomputed with the host sides' launch arithmetic); planted faults land past the bounds.  The worst ratios are printed (pytest -s) as
`token-ratio cpu <kernel> <case> <width> <quantity> <ratio>` lines; profiles/tests_token_rows_bounds.md sets them next to the MI355X's."""
import pytest
import torch

import token_rows_util as T
from test_rowwise_host import CPU_BF16_MAX, CPU_F32_MAX, emul_ln_bwd, emul_ln_fwd
from token_rows_util import BF16, EPS, F32, I32, PAD, SENTINEL


rep = T.reporter("cpu", {"f32": CPU_F32_MAX, "bf16": CPU_BF16_MAX})


def _assert_reaches(c, reaches, what):
    assert c["reaches"], f"{what} names no path"
    for tag in c["reaches"]:
        assert reaches(c, tag), f"{what} does not reach: {tag}"


def _fails(fn, match="past the bound|differ"):
    with pytest.raises(AssertionError, match=match):
        fn()


# ------------------------------------------------------------------------------------------------------------------------- embedding
def emul_pos_ids(c, later_chunks_strict=False):
    """position ids the way roberta_pos counts them: 64-token ballots over j <= t (later_chunks_strict: the planted fault, j < t from the
    second ballot on)"""
    ids, T_ = c["ids"], c["T"]
    if c["pos_mode"]:
        return torch.arange(T_).unsqueeze(0).expand(c["B"], -1).contiguous()
    nz = (ids != PAD).int()
    out = torch.full_like(ids, PAD)
    for t in range(T_):
        cnt = torch.zeros(c["B"], dtype=torch.int32)
        for j0 in range(0, t + 1, 64):
            hi = t if (later_chunks_strict and j0 > 0) else t + 1
            cnt += nz[:, j0:min(j0 + 64, hi)].sum(1).int()
        out[:, t] = torch.where(ids[:, t] != PAD, cnt.long() + PAD, torch.full((c["B"],), PAD))
    return out


def emul_emb_fwd(c, keep=None, drop_scale=1.0, pid=None):
    pid = emul_pos_ids(c) if pid is None else pid
    lr, orow = T.emb_live(c)
    mu, rstd, y = emul_ln_fwd(T.emb_rows32(c, pid)[lr], c["w"], c["b"], EPS)
    if keep is not None:
        y = torch.where(keep[lr], y * torch.tensor(drop_scale, dtype=F32), torch.zeros(()))
    got = {"y32": torch.full((c["out_rows"], c["D"]), SENTINEL), "mean": torch.full((c["rows"],), SENTINEL),
           "rstd": torch.full((c["rows"],), SENTINEL), "pos_ids": torch.full((c["rows"],), SENTINEL).view(I32).clone()}
    got["y32"][orow], got["mean"][lr], got["rstd"][lr], got["pos_ids"][lr] = y, mu, rstd, pid.reshape(-1)[lr].to(I32)
    got["y"] = got["y32"].to(BF16)
    return got


def emul_emb_bwd(c, mean, rstd, pid32, use_dy32, keep=None, drop_scale=1.0, drop_from=None):
    """drop_from: the planted fault -- the rows from that (unpacked) row on are left out of dbeta"""
    lr, orow = T.emb_live(c)
    dy = c["dy"][orow].float()
    if use_dy32:
        dy = dy + c["dy32"][orow]
    if keep is not None:
        dy = torch.where(keep[lr], dy * torch.tensor(drop_scale, dtype=F32), torch.zeros(()))
    dz, dy, xh = emul_ln_bwd([dy], T.emb_rows32(c, pid32.long())[lr], mean[lr], rstd[lr], c["w"])
    ids, pl = c["ids"].reshape(-1)[lr], pid32.long()[lr]
    wv = ids != PAD
    pv = torch.ones_like(wv) if c["pos_mode"] else pl != PAD
    dyb = dy if drop_from is None else dy[lr < drop_from]
    return {"dz": dz, "dword": c["dword0"].clone().index_add_(0, ids[wv], dz[wv]), "dpos": c["dpos0"].clone().index_add_(0, pl[pv], dz[pv]),
            "dgamma": c["dgamma0"] + (dy * xh).sum(0), "dbeta": c["dbeta0"] + dyb.sum(0), "dtype": c["dtype0"] + dz.sum(0)}


@pytest.mark.parametrize("name", sorted(T.EMB_CASES))
def test_embedding_emulation_within_bounds_and_case_reaches_its_path(name):
    c = T.emb_case(name)
    for tag in c["reaches"]:
        assert T.emb_reaches(c, tag), f"{name} does not reach: {tag}"
    assert torch.equal(emul_pos_ids(c), T.emb_pos_ids(c))
    T.check_emb_fwd(c, emul_emb_fwd(c), rep)
    mean, rstd, pid32 = T.emb_stats(c)
    for use32 in (False, True):
        ref = T.emb_bwd_ref(c, mean, rstd, pid32, use32)
        T.check_emb_bwd(c, emul_emb_bwd(c, mean, rstd, pid32, use32), ref, rep, tag="dy32:" if use32 else "")
    if "hundreds of hits" in c["reaches"]:
        assert ref["hits"] >= 150


def test_embedding_dropout_emulation_and_binomial_window():
    c = T.emb_case(T.DROP_CASE)
    p = T.DROP_P
    n = int((c["row_map"] >= 0).sum()) * c["D"]
    lo, hi = T.binomial_window(p, n)
    assert 0.0 < lo < 1.0 - p < hi < 1.0 and hi - lo < 0.02, (lo, hi)      # excludes all kept and all dropped, and a p off by 0.01
    keep = torch.rand((c["rows"], c["D"]), generator=torch.Generator().manual_seed(3)) >= p
    live = c["row_map"] >= 0
    T.check_keep_fraction(keep[live], p)
    off = torch.rand(keep[live].shape, generator=torch.Generator().manual_seed(4)) >= 0.12
    for bad in (torch.ones_like(keep[live]), torch.zeros_like(keep[live]), off):
        _fails(lambda: T.check_keep_fraction(bad, p), "kept fraction")
    scale = 1.0 / (1.0 - p)
    T.check_emb_fwd(c, emul_emb_fwd(c, keep, scale), rep, keep, scale, tag="drop:")
    mean, rstd, pid32 = T.emb_stats(c)
    ref = T.emb_bwd_ref(c, mean, rstd, pid32, True, keep, scale)
    T.check_emb_bwd(c, emul_emb_bwd(c, mean, rstd, pid32, True, keep, scale), ref, rep, tag="drop:")
    # a forward that used another mask, a backward that ignored it
    other = keep.clone()
    other[live.nonzero()[0, 0], 5] ^= True
    _fails(lambda: T.check_emb_fwd(c, emul_emb_fwd(c, other, scale), rep, keep, scale))
    _fails(lambda: T.check_emb_bwd(c, emul_emb_bwd(c, mean, rstd, pid32, True), ref, rep))


def test_embedding_planted_faults_are_caught():
    c = T.emb_case("t130_1024")
    wrong = emul_pos_ids(c, later_chunks_strict=True)
    assert torch.equal(wrong[:, :64], T.emb_pos_ids(c)[:, :64]) and not torch.equal(wrong, T.emb_pos_ids(c))
    _fails(lambda: T.check_emb_fwd(c, emul_emb_fwd(c, pid=wrong), rep), "pos_ids differ")
    c = T.emb_case("bwd_stride_1024")
    mean, rstd, pid32 = T.emb_stats(c)
    ref = T.emb_bwd_ref(c, mean, rstd, pid32, False)
    got = emul_emb_bwd(c, mean, rstd, pid32, False, drop_from=4096)     # the rows of the grid-stride pass missing from dbeta
    _fails(lambda: T.check_emb_bwd(c, got, ref, rep))
    got = emul_emb_bwd(c, mean, rstd, pid32, False)
    v = int(c["ids"].reshape(-1)[T.emb_live(c)[0]][7])
    assert v != PAD
    got["dword"][v] -= got["dz"][7]                                       # one of some 200 hits missing from a table row
    _fails(lambda: T.check_emb_bwd(c, got, ref, rep))
    got = emul_emb_bwd(c, mean, rstd, pid32, False)
    got["dword"][PAD, 3] = 1e-30                                          # the pad row touched
    _fails(lambda: T.check_emb_bwd(c, got, ref, rep), "past the bound|pad row")


# -------------------------------------------------------------------------------------------------------------------------- rows.hip
@pytest.mark.parametrize("R,D,S,pattern", T.ROWS_SHAPES)
def test_rows_scatter_emulation_within_bounds(R, D, S, pattern):
    c = T.rows_case(R, D, S, pattern)
    _assert_reaches(c, T.rows_reaches, f"rows case {R, D, S, pattern}")
    idx = c["index"]
    v = idx >= 0
    got = c["dst0"].clone().index_add_(0, idx[v].long(), c["upd16"].float()[v])
    ref, bound = T.hits_sum(c["upd16"], idx, v, c["dst0"])
    rep("rows_scatter_add", pattern, D, f"R{R}", T.check_f32(got, ref, bound, "scatter"), "f32")
    untouched = torch.bincount(idx[v].long(), minlength=S) == 0
    assert T.bits_equal(got[untouched], c["dst0"][untouched])
    if R > 2:          # one update lost
        r = int(v.nonzero()[0, 0])
        bad = got.clone()
        bad[idx[r].long()] -= c["upd16"][r].float()
        _fails(lambda: T.check_f32(bad, ref, bound, "one update lost"))
    assert torch.equal(T.gather_ref(c["src16"], idx)[~v].float().abs().sum(), torch.zeros(()))


@pytest.mark.parametrize("R,D,nk,skip", T.SEG_SHAPES)
def test_rows_segment_sum_emulation_within_bounds(R, D, nk, skip):
    c = T.seg_case(R, D, nk, skip)
    _assert_reaches(c, T.seg_reaches, f"segment case {R, D, nk, skip}")
    keys = c["keys"]
    v = (keys >= 0) & (keys != skip)
    got = c["out0"].clone().index_add_(0, keys[v], c["src"][v])
    ref, bound = T.hits_sum(c["src"], keys, v, c["out0"])
    rep("rows_segment_sum", f"R{R}", D, "out", T.check_f32(got, ref, bound, "segment sum"), "f32")
    if skip < nk:
        assert T.bits_equal(got[skip], c["out0"][skip])


def test_case_lists_cover_every_launch_path_of_the_row_pool_and_mim_kernels():
    """the tags above are asserted case by case; here: every path of the lists is still named by some case, and the launch figures they
    stand for, recomputed over the case lists with the host sides' formulas, are all there"""
    assert {t for c in T.ROWS_CASES for t in c[-1]} == T.ROWS_PATHS
    assert {t for c in T.SEG_CASES for t in c[-1]} == T.SEG_PATHS
    threads = {T.rows_threads(R, D) for R, D, _, _ in T.ROWS_SHAPES}
    assert threads >= {1, 255, 256, 257}
    assert {T.rows_grid(R, D) for R, D, _, _ in T.ROWS_SHAPES if T.rows_threads(R, D) in (1, 255, 256, 257)} == {1, 2}
    assert 129 in {D >> 3 for _, D, _, _ in T.ROWS_SHAPES} and 129 in {D >> 3 for _, D, _, _ in T.SEG_SHAPES}
    assert {D for _, D, _, _ in T.ROWS_SHAPES} == {8, 64, 768, 1032, 2048} == {D for _, D, _, _ in T.SEG_SHAPES}
    assert {T.seg_passes(D) for _, D, _, _ in T.SEG_SHAPES} == {1, 2}
    assert any(p == "one" and R >= 300 for R, _, _, p in T.ROWS_SHAPES)
    # pool_rows: the smallest and the full workgroup, N = 2, both parities
    assert set(T.POOL_D) == set(T.POOL_D_TAGS) and set(T.POOL_N) == set(T.POOL_N_TAGS)
    assert {T.pool_fwd_block(D) for D in T.POOL_D} >= {2, 256} and max(T.POOL_D) == 1024
    assert 2 in T.POOL_N and {N % 2 for N in T.POOL_N if N > 2} == {0, 1}
    assert {t for D in T.POOL_D for N in T.POOL_N for t in T.pool_case(D, N)["reaches"]} == T.POOL_PATHS
    # MIM loss: lanes of the first and the second forward pass, the forward's grid, the masks
    assert set(T.MIM_D) == set(T.MIM_D_TAGS) and set(T.MIM_BN) == set(T.MIM_BN_TAGS) and set(T.MIM_MASKS) == set(T.MIM_MASK_TAGS)
    assert {(T.mim_lanes(D, 0), T.mim_lanes(D, 1)) for D in T.MIM_D} == {(1, 0), (64, 0), (64, 1), (64, 32), (64, 64)}
    assert [D for D in T.MIM_D if D > 512 and D % 512 == 8] == [520]
    assert sorted(B * N for B, N in T.MIM_BN) == [4, 185, 2109] and 2109 > 4 * T.MIM_PARTIALS
    assert {T.mim_fwd_grid(B, N) for B, N in T.MIM_BN} == {1, 47, T.MIM_PARTIALS}


# ------------------------------------------------------------------------------------------------------------------------- ViT input
def emul_vit_bwd(c, skip_last_of_chunks=False):
    Bt, Bx, P, D, reps = c["Bt"], c["Bx"], c["P"], c["D"], c["reps"]
    G = c["dx0"].view(Bx, P + 1, D)
    gp = G[:, 1:]
    m = c["mask"].bool().unsqueeze(-1) if c["mask"] is not None else torch.zeros((Bx, P, 1), dtype=torch.bool)
    kept = torch.where(m, torch.zeros(()), gp).view(reps, Bt, P, D)
    dtok = kept[0].clone()
    for r in range(1, reps):
        dtok = dtok + kept[r]
    msk = torch.where(m, gp, torch.zeros(()))
    if skip_last_of_chunks:       # the planted fault: every chunk's last patch left out
        ch = T.vit_chunks(Bt, Bx, P)
        per = T.cdiv(P, ch)
        for k in range(ch):
            i1 = min((k + 1) * per, P)
            if i1 > k * per:
                msk[:, i1 - 1] = 0
    got = {"dtok": dtok.reshape(Bt * P, D), "dcls": c["dcls0"] + G[:, 0].sum(0)}
    got["dmtok"] = c["dmtok0"] + msk.sum((0, 1)) if c["mask"] is not None else c["dmtok0"].clone()
    return got


@pytest.mark.parametrize("name", sorted(T.VIT_CASES))
def test_vit_tokens_emulation_within_bounds_and_case_reaches_its_path(name):
    c = T.vit_case(name)
    assert T.vit_reaches(c), name
    x0 = T.vit_fwd_ref(c)
    assert x0.shape == (c["Bx"] * (c["P"] + 1), c["D"]) and x0.dtype == F32
    T.check_vit_bwd(c, emul_vit_bwd(c), rep)
    if c["mask"] is not None and c["name"] != "grid_stride":
        _fails(lambda: T.check_vit_bwd(c, emul_vit_bwd(c, skip_last_of_chunks=True), rep))


def test_vit_tokens_cases_select_every_chunk_count_and_the_rejection():
    assert sorted({T.vit_chunks(c["Bt"], c["Bx"], c["P"]) for c in map(T.vit_case, T.VIT_CASES)}) == [1, 2, 4]
    assert T.vit_reaches(T.vit_case("rejected"))
    assert {T.vit_case(n)["pattern"] for n in T.VIT_CASES} >= {"none", "all", "clean_view"}
    assert {T.vit_case(n)["D"] for n in T.VIT_CASES} == {64, 768, 1024}


def test_patchify_cases_and_reference():
    assert max(T.patchify_threads(*s[:2], s[3], s[4], s[2]) for s in T.PATCH_CASES) > 4096 * 256
    assert sum(T.patchify_threads(*s[:2], s[3], s[4], s[2]) > 4096 * 256 for s in T.PATCH_CASES) == 1
    B, C, P, H, W = T.PATCH_CASES[0]
    img = T.randn((B, C, H, W), 1.0, 1)
    ref = T.patchify_ref(img, P)
    unf = torch.nn.functional.unfold(img, P, stride=P).transpose(1, 2).reshape(-1, C * P * P).to(BF16)
    assert torch.equal(ref, unf)


@pytest.mark.parametrize("N", T.POOL_N)
@pytest.mark.parametrize("D", T.POOL_D)
def test_pool_rows_emulation_within_bounds(D, N):
    c = T.pool_case(D, N)
    _assert_reaches(c, T.pool_reaches, f"pool case D = {D}, N = {N}")
    B = c["B"]
    y = c["y"].float().view(B, N, D)
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(N - 1), dtype=F32)

    def fwd(div):
        s = y[:, 1::2].sum(1) + y[:, 2::2].sum(1)       # the two row phases
        return torch.cat([(s * div).unsqueeze(1), y[:, 1:]], 1).to(BF16).reshape(B * N, D)

    g = c["dy"].float().view(B, N, D)
    bwd = g.double() + (g[:, :1].double() * inv.double())     # an fma: one rounding of the exact sum with the rounded inv
    bwd = bwd.float()
    bwd[:, 0] = 0.0
    T.check_pool(c, fwd(inv), bwd.to(BF16).reshape(B * N, D), rep)
    if N > 2:           # dividing by N
        _fails(lambda: T.check_pool(c, fwd(torch.tensor(1.0 / N)), bwd.to(BF16).reshape(B * N, D), rep))


# --------------------------------------------------------------------------------------------------------------------------- MIM loss
def emul_mim(c, cls_term, kp_on_cls=False):
    B, N, D = c["B"], c["N"], c["D"]
    d = (c["x"].float() - c["t"].float()).view(B, N, D)
    m = c["mask"].bool()
    sums = torch.stack([(d[:, 1:] ** 2 * m.unsqueeze(-1)).sum(), (d[:, 0] ** 2).sum(), m.sum().float()])
    g = c["gout"][0]
    kp = 2.0 * g / torch.clamp(sums[2] * D, min=1.0)
    kc = 2.0 * g / (torch.tensor(float(B)) * D) if cls_term else torch.zeros(())
    if kp_on_cls and cls_term:
        kc = kp
    k = torch.cat([kc.expand(B, 1), m.float() * kp], 1).unsqueeze(-1)
    return sums, (k * d).to(BF16).reshape(B * N, D)


@pytest.mark.parametrize("B,N", T.MIM_BN)
@pytest.mark.parametrize("D", T.MIM_D)
def test_mim_loss_emulation_within_bounds(D, B, N):
    for pattern in T.MIM_MASKS:
        c = T.mim_case(D, B, N, pattern)
        _assert_reaches(c, T.mim_reaches, f"MIM case {D, B, N, pattern}")
        for cls_term in (True, False):
            sums, dx = emul_mim(c, cls_term)
            T.check_mim(c, sums, dx, cls_term, rep)
        if pattern == "random" and B * (N - 1) > 4:       # count != B: kp on the cls rows is another factor
            sums, dx = emul_mim(c, True, kp_on_cls=True)
            _fails(lambda: T.check_mim(c, sums, dx, True, rep))
            sums, dx = emul_mim(c, True)
            bad = dx.clone()
            row = int(c["mask"].reshape(-1).nonzero()[0, 0])
            row = (row // (N - 1)) * N + 1 + row % (N - 1)
            bad[row, D - 8:] = 0                            # a dropped 8-column group
            _fails(lambda: T.check_mim(c, sums, bad, True, rep))
    assert B * N <= 4 or B * N == 185 or B * N > 4 * T.MIM_PARTIALS
