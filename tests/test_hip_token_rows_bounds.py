"""rows.hip, vit_input.hip and the loss half of mim.hip under exact comparisons and elementwise fp64 bounds.

tests/test_hip_kernels.py runs these kernels at one shape each (rows_scatter_add at none) and accepts the bf16 outputs at 1e-2 of the tensor's
largest value.  Here every kernel runs at the smallest shapes that reach each of its paths (token_rows_util has the cases and the arithmetic
that picks them, tests/test_token_rows_host.py asserts that each case reaches its path): 1 / 255 / 256 / 257 threads, 129 chunks a row and
the second column pass for the row moves; each chunk count of the token backward, a ragged and an empty chunk, the rejected shape, the
grouped set fold and both 8192-workgroup grid-stride loops; patchify past its 4096-workgroup cap; pool_rows at N = 2 / 3 / 50 / 197 and
D = 8 ... 1024; the MIM loss at D = 8 ... 1024, past its 512-workgroup cap, with no, every and one image's patches masked.  Copies are compared
with torch.equal, sums and bf16 results with the bounds of token_rows_util's header.  Every call goes through the C ABI: inputs are views of
NaN-filled parents, outputs of 7.0-filled ones whose outside must keep its bits.

Every check prints `token-ratio gpu <kernel> <case> <width> <quantity> <worst err / bound>` (pytest -s); profiles/tests_token_rows_bounds.md
holds the table."""
import pytest
import torch

import token_rows_util as T
from token_rows_util import BF16, F32, U8

pytestmark = pytest.mark.gpu

DEV = "cuda"
XFM_E_ARG = -1


def _L():
    from xfm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


rep = T.reporter("gpu")


def _run(fn, *args):
    rc = fn(*args, _stream())
    torch.cuda.synchronize()
    return rc


def _ok(fn, what, *args):
    _L().check(_run(fn, *args), what)


# -------------------------------------------------------------------------------------------------------------------------- rows.hip
@pytest.mark.parametrize("R,D,S,pattern", T.ROWS_SHAPES)
def test_rows_gather_is_a_copy_and_scatter_add_within_bounds(R, D, S, pattern):
    from xfm_amd import functional as Fx
    lib = _L().load()
    c = T.rows_case(R, D, S, pattern)
    g = T.dev(c, DEV)
    idx = g["index"]
    # gather, bf16 rows and the fp32-view form of functional.rows_gather
    o = T.Outs(DEV)
    src16, src32 = T.poisoned_in(c["src16"], DEV), T.poisoned_in(c["src32"], DEV)
    _ok(lib.xfm_rows_gather, "rows_gather", src16.data_ptr(), idx.data_ptr(), R, D, o.add("g16", (R, D), BF16))
    o.add("g32", (R, D), F32)
    Fx.rows_gather(src32, idx, out=o["g32"])
    torch.cuda.synchronize()
    o.check_outside()
    T.check_equal(o["g16"].contiguous(), T.gather_ref(g["src16"], idx), "rows_gather")
    T.check_equal(o["g32"].contiguous(), T.gather_ref(g["src32"], idx), "rows_gather, fp32 view")
    # scatter-add onto a non-zero destination
    o = T.Outs(DEV)
    upd = T.poisoned_in(c["upd16"], DEV)
    _ok(lib.xfm_rows_scatter_add, "rows_scatter_add", upd.data_ptr(), idx.data_ptr(), R, D, o.add("dst", (S, D), F32, c["dst0"]))
    o.check_outside()
    v = idx >= 0
    ref, bound = T.hits_sum(g["upd16"], idx, v, g["dst0"])
    rep("rows_scatter_add", pattern, D, f"R{R}", T.check_f32(o["dst"], ref, bound, "rows_scatter_add"), "f32")
    untouched = torch.bincount(idx[v].long(), minlength=S) == 0
    T.check_equal(o["dst"][untouched], g["dst0"][untouched], "destination rows without hits")


@pytest.mark.parametrize("R,D,nk,skip", T.SEG_SHAPES)
def test_rows_segment_sum_within_bounds_and_repeatable(R, D, nk, skip):
    lib = _L().load()
    c = T.seg_case(R, D, nk, skip)
    g = T.dev(c, DEV)
    skey, perm = torch.sort(g["keys"], stable=True)
    src = T.poisoned_in(c["src"], DEV)
    outs = []
    for _ in range(2):
        o = T.Outs(DEV)
        _ok(lib.xfm_rows_segment_sum, "rows_segment_sum", src.data_ptr(), perm.data_ptr(), skey.data_ptr(), R, D, skip,
            o.add("out", (nk, D), F32, c["out0"]))
        o.check_outside()
        outs.append(o["out"].contiguous())
    v = (g["keys"] >= 0) & (g["keys"] != skip)
    ref, bound = T.hits_sum(g["src"], g["keys"], v, g["out0"])
    rep("rows_segment_sum", f"R{R}", D, "out", T.check_f32(outs[0], ref, bound, "rows_segment_sum"), "f32")
    assert T.bits_equal(outs[0], outs[1])
    untouched = torch.bincount(g["keys"][v], minlength=nk) == 0
    T.check_equal(outs[0][untouched], g["out0"][untouched], "rows without a run")


# ------------------------------------------------------------------------------------------------------------------------- ViT input
def _vit_bwd(c):
    lib = _L().load()
    D, Bt, Bx, P = c["D"], c["Bt"], c["Bx"], c["P"]
    o = T.Outs(DEV)
    dx0 = T.poisoned_in(c["dx0"], DEV)
    mask = None if c["mask"] is None else c["mask"].to(DEV).contiguous()
    rc = _run(lib.xfm_vit_tokens_bwd, dx0.data_ptr(), 0 if mask is None else mask.data_ptr(), Bt, Bx, P, D, o.add("dtok", (Bt * P, D), F32),
              o.add("dcls", (D,), F32, c["dcls0"]), o.add("dmtok", (D,), F32, c["dmtok0"]))
    return rc, o


@pytest.mark.parametrize("name", sorted(T.VIT_CASES))
def test_vit_tokens_forward_is_a_copy_and_backward_within_bounds(name):
    lib = _L().load()
    c = T.vit_case(name)
    g = T.dev(c, DEV)
    D, Bt, Bx, P = c["D"], c["Bt"], c["Bx"], c["P"]
    o = T.Outs(DEV)
    tok, cls, mtok = (T.poisoned_in(c[k], DEV) for k in ("tok", "cls", "mtok"))
    mask = None if c["mask"] is None else g["mask"].contiguous()
    _ok(lib.xfm_vit_tokens_fwd, "vit_tokens_fwd", tok.data_ptr(), cls.data_ptr(), mtok.data_ptr(), 0 if mask is None else mask.data_ptr(),
        Bt, Bx, P, D, o.add("x0", (Bx * (P + 1), D), F32))
    o.check_outside()
    T.check_equal(o["x0"].contiguous(), T.vit_fwd_ref(g), "vit_tokens_fwd")
    rc, o = _vit_bwd(c)
    _L().check(rc, "vit_tokens_bwd")
    o.check_outside()
    T.check_vit_bwd(g, {q: o[q] for q in ("dtok", "dcls", "dmtok")}, rep)
    if c["pattern"] == "all":
        assert float(o["dtok"].abs().max()) == 0.0, "dtok of fully masked views is not zero"


def test_vit_tokens_backward_rejects_a_dtok_too_small_for_its_scratch():
    c = T.vit_case("rejected")
    rc, o = _vit_bwd(c)
    assert rc == XFM_E_ARG, rc
    assert b"dtok too small" in _L().load().xfm_last_error()
    o.check_unchanged()


@pytest.mark.parametrize("B,C,P,H,W", T.PATCH_CASES)
def test_patchify_is_a_rounded_gather(B, C, P, H, W):
    lib = _L().load()
    img = T.randn((B, C, H, W), 1.0, 10300 + B + H)
    flat = T.poisoned_in(img.reshape(-1), DEV)
    o = T.Outs(DEV)
    rows, cols = B * (H // P) * (W // P), C * P * P
    _ok(lib.xfm_patchify, "patchify", flat.data_ptr(), B, C, H, W, P, o.add("out", (rows, cols), BF16))
    o.check_outside()
    T.check_equal(o["out"].contiguous(), T.patchify_ref(img.to(DEV), P), "patchify")


@pytest.mark.parametrize("N", T.POOL_N)
@pytest.mark.parametrize("D", T.POOL_D)
def test_pool_rows_forward_and_backward_within_bounds(D, N):
    lib = _L().load()
    c = T.pool_case(D, N)
    B = c["B"]
    o = T.Outs(DEV)
    _ok(lib.xfm_pool_rows_fwd, "pool_rows_fwd", o.add("y", (B * N, D), BF16, c["y"]), B, N, D)
    dy = T.poisoned_in(c["dy"], DEV)
    _ok(lib.xfm_pool_rows_bwd, "pool_rows_bwd", dy.data_ptr(), B, N, D, o.add("out", (B * N, D), BF16))
    o.check_outside()
    T.check_pool(T.dev(c, DEV), o["y"].contiguous(), o["out"].contiguous(), rep)


# --------------------------------------------------------------------------------------------------------------------------- MIM loss
@pytest.mark.parametrize("B,N", T.MIM_BN)
@pytest.mark.parametrize("D", T.MIM_D)
def test_mim_loss_forward_and_backward_within_bounds(D, B, N):
    lib = _L().load()
    nf = _L().MIM_SUMS_FLOATS
    for pattern in T.MIM_MASKS:
        c = T.mim_case(D, B, N, pattern)
        g = T.dev(c, DEV)
        x, t, gout = T.poisoned_in(c["x"], DEV), T.poisoned_in(c["t"], DEV), T.poisoned_in(c["gout"], DEV)
        mask = g["mask"].contiguous()
        assert mask.dtype == U8
        o = T.Outs(DEV)
        sums = o.add("sums", (nf,), F32, torch.zeros(nf))
        _ok(lib.xfm_mim_loss_fwd, "mim_loss_fwd", x.data_ptr(), t.data_ptr(), mask.data_ptr(), B, N, D, sums)
        for cls_term in (1, 0):
            _ok(lib.xfm_mim_loss_bwd, "mim_loss_bwd", x.data_ptr(), t.data_ptr(), mask.data_ptr(), sums, gout.data_ptr(), cls_term, B, N, D,
                o.add(f"dx{cls_term}", (B * N, D), BF16))
            o.check_outside()
            T.check_mim(g, o["sums"][:3].contiguous(), o[f"dx{cls_term}"].contiguous(), bool(cls_term), rep)
