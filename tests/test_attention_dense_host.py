"""Host-side proof that attention_util's dense bounds hold for a correct fp32 evaluation and bite for a wrong one (CPU, no GPU); the twin
of tests/test_attention_host.py for the routes of tests/test_hip_attention_dense_bounds.py.

1. attention_util.dense_plan, the restatement of the library's route choice, agrees with the route every dense spec names, and the specs
   together reach every dense route.
2. A plain fp32 emulation of each family's arithmetic -- the ViT forward (accumulator from bias / scale, one row maximum, exp2 of one fma),
   the general plain kernels (test_attention_host's emulation), the short pair and the long kernels (softmax in the exponent of 2 from the
   given lse; the dK/dV side of the short pair with lse in the accumulator), dS and P rounded to bf16 before the second product, the bias
   gradient summed nb entries at a time and flushed slice by slice onto 0.5, the opt-in single pass -- stays within HOST_MAX of every bound, and prints
   `attn-ratio host <quantity> <spec> <ratio>` (pytest -s).
3. Planted faults land past the bound on the quantity named.
4. test_max_norm_check_misses_what_the_dense_bounds_catch: two of them pass the 1e-2 / 2e-2 max-norm checks of tests/test_hip_kernels.py."""
import functools

import pytest
import torch

import attention_util as A
from attention_util import BF16, SCALE
from test_attention_host import HOST_MAX, emul_fwd

SPECS = A.dense_specs()
LOG2E = torch.tensor(1.44269504088896341, dtype=torch.float32)
INV = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(SCALE, dtype=torch.float32)
C2 = torch.tensor(SCALE, dtype=torch.float32) * LOG2E


def _report(sp, what, ratio):
    print(f"attn-ratio host {what} {A.spec_id(sp)} {ratio:.3g}")
    assert ratio <= HOST_MAX, f"{A.spec_id(sp)} {what}: a correct fp32 evaluation at {ratio:.3g} of the bound: the derivation misses a rounding"


def _fails(fn, match="past the bound"):
    with pytest.raises(AssertionError, match=match):
        fn()


@functools.lru_cache(maxsize=4)
def _case(sp):
    return A.make_case(sp)


def _spec(route, shape, name=None):
    return next(s for s in SPECS if s.route == route and A.shape_of(s) == shape and (name is None or s.name == name))


# ------------------------------------------------------------------------------------------------------------------- fp32 emulation
def _h32(t):
    return t.permute(0, 2, 1, 3).float()


def _rows(t, S):
    return t.permute(0, 2, 1, 3).reshape(t.shape[0] * S, t.shape[1] * 64)


def _bias32(c, bias=None):
    b = c["bias"] if bias is None else bias
    return None if b is None else b[:, :, :c["sp"].Sk].unsqueeze(0)


def emul_vit_fwd(c, bias=None, k=None, unscaled_bias=False, drop_last_tile=False):
    """attn_fwd_vit_kernel -> (o bf16 [B*Sq, H*64], o_lo, lse fp32 [B*H, Sq]).  Faults: bias (another bias), k (other keys), unscaled_bias
    (the accumulator starts from bias, not bias / scale), drop_last_tile (the last key tile left out)."""
    sp = c["sp"]
    K = _h32(c["k"] if k is None else k)
    st = _h32(c["q"]) @ K.transpose(-1, -2)
    b = _bias32(c, bias)
    if b is not None:
        st = (b if unscaled_bias else b * INV) + st
    mx = st.max(-1, keepdim=True).values
    p = torch.exp2(st * C2 + (-mx * C2))
    if drop_last_tile:
        p[..., 16 * ((sp.Sk - 1) // 16):] = 0.0
    l = p.sum(-1, keepdim=True)
    v = (p.to(BF16).float() @ _h32(c["v"])) * (1.0 / l)
    o = v.to(BF16)
    o_lo = (v - o.float()).to(BF16)
    lse = mx.squeeze(-1) * SCALE + torch.log(l.squeeze(-1))
    return _rows(o, sp.Sq), _rows(o_lo, sp.Sq), lse.reshape(sp.B * sp.H, sp.Sq)


def emul_probs(c, fam, lse32, bias=None):
    """P fp32 [B, H, Sq, Sk] from the given lse as the family forms it"""
    sp = c["sp"]
    raw = _h32(c["q"]) @ _h32(c["k"]).transpose(-1, -2)
    b = _bias32(c, bias)
    lse = lse32.reshape(sp.B, sp.H, sp.Sq, 1)
    if fam == "general":
        s = raw * SCALE if b is None else raw * SCALE + b
        return torch.exp(s - lse)
    if fam == "short_dq":
        st = raw if b is None else b * INV + raw
        return torch.exp2(st * C2 + (-lse * LOG2E))
    if fam == "short_dkv":
        st = ((-lse) * INV + (0.0 if b is None else b * INV)) + raw
        return torch.exp2(st * C2)
    assert fam == "long"
    nl = -lse * LOG2E
    return torch.exp2(raw * C2 + (nl if b is None else b * LOG2E + nl))


def emul_dense_bwd(c, lse32, rt, out_halves=None, bias=None, store_dbias=False, drop_slice=None, drop_last_tile=False, dbias_init=A.DBIAS_INIT):
    """The backward of Route rt -> dict of delta, dq, dk, dv, dbias.  out_halves: (o, o_lo) bf16 [B*Sq, H*64] where delta = dO . (O + O_lo).
    Faults: bias (another bias), store_dbias (the bias gradient stored, not added), drop_slice (that slice's plane left out),
    drop_last_tile (the dK/dV side leaves the last key tile's P at zero)."""
    sp = c["sp"]
    B, H, Sq, Sk = sp.B, sp.H, sp.Sq, sp.Sk
    _, fam_q, fam_k = A.dense_families(rt)
    Pq, Pk = emul_probs(c, fam_q, lse32, bias), emul_probs(c, fam_k, lse32, bias)
    if drop_last_tile:
        Pk = Pk.clone()
        Pk[..., 16 * ((Sk - 1) // 16):] = 0.0
    Q, K, V, DO = _h32(c["q"]), _h32(c["k"]), _h32(c["v"]), _h32(c["do"])
    dp = DO @ V.transpose(-1, -2)
    if out_halves is None:
        delta = (Pq * dp).sum(-1)
    else:
        O, L = (t.float().reshape(B, Sq, H, 64).permute(0, 2, 1, 3) for t in out_halves)
        delta = (DO * (O + L)).sum(-1)
    ds = Pq * (dp - delta.unsqueeze(-1))
    dq = ((ds.to(BF16).float() @ K) * SCALE).to(BF16)
    ds_k = Pk * (dp - delta.unsqueeze(-1))
    dk = ((ds_k.to(BF16).float().transpose(-1, -2) @ Q) * SCALE).to(BF16)
    dv = (Pk.to(BF16).float().transpose(-1, -2) @ DO).to(BF16)
    out = {"delta": delta.reshape(B * H, Sq), "dq": _rows(dq, Sq), "dk": _rows(dk, Sk), "dv": _rows(dv, Sk)}
    if c["bias"] is not None:
        nb = max(rt.nb, 1)
        ds_b = ds      # mode 4 of the single pass: the bias-gradient kernel of the long route forms its own P
        if rt.dq == "vit3" and rt.dbias == "blocks":
            ds_b = emul_probs(c, "long", lse32, bias) * (dp - delta.unsqueeze(-1))
        acc = torch.zeros((H, Sq, Sk)) if store_dbias else torch.full((H, Sq, Sk), dbias_init)
        for sl, b0 in enumerate(range(0, B, nb)):
            part = torch.zeros((H, Sq, Sk))
            for b in range(b0, min(b0 + nb, B)):
                part = part + ds_b[b]
            if sl != drop_slice:
                acc = acc + part
        out["dbias"] = acc.reshape(H * Sq, Sk)
    return out


def _fwd_of(sp, c, **faults):
    if sp.want.fwd.startswith("vit"):
        return emul_vit_fwd(c, **faults)
    o, lse = emul_fwd(c)
    return o, None, lse


# ------------------------------------------------------------------------------------------------------------------------ the routes
def test_restatement_agrees_with_every_declared_route():
    for sp in SPECS:
        assert A.dense_plan(sp) == sp.want, (A.spec_id(sp), A.dense_plan(sp), sp.want)
        if sp.bias:      # the padding of a bias row is NaN wherever it has any
            assert sp.ld >= sp.Sk and sp.ld % 4 == 0
            assert bool(torch.isnan(_case(sp)["bias"][:, :, sp.Sk:]).all())
    for sp in (s for s in SPECS if s.route == "vit_walk"):
        c, grid, last = A.vit_map(sp.B, sp.H)
        assert sp.B * sp.H > 256 and c == 2 and last == 1 and sp.B % 2 == 1, "two items a workgroup, a last one of one, workgroups across heads"


def test_the_specs_reach_every_dense_route():
    seen = set()
    for sp in SPECS:
        seen.add(("fwd", sp.want.fwd))
        if not sp.bwd:
            continue
        plans = [A.dense_plan(sp), A.dense_plan(sp, bias_t=False, have_ws=False), A.dense_plan(sp, pre=True, o_lo=True), A.dense_plan(sp, det=True),
                 A.dense_plan(sp, tiled=True, vit_mode=3), A.dense_plan(sp, tiled=True, vit_mode=4)]
        for rt in plans:
            seen |= {("dq", rt.dq, A.attn_short_dq_np(sp.Sk) if rt.dq.startswith("short") else 0), ("dkv", rt.dkv), ("dbias", rt.dbias, rt.planes > 0)}
            if rt.dq == "sums":
                seen.add(("sums nb", rt.nb))
            if rt.dbias == "blocks":
                seen.add(("blocks entries", min(rt.nb, 2), sp.B % max(rt.nb, 1) != 0))
    want = {("fwd", "vit13"), ("fwd", "vit_rt"), ("fwd", "plain_res"), ("fwd", "plain_stream"),
            ("dq", "short", 4), ("dq", "short", 7), ("dq", "short", 8), ("dq", "short_pre", 4), ("dq", "short_pre", 7), ("dq", "short_pre", 8),
            ("dq", "sums", 0), ("dq", "long", 0), ("dq", "vit3", 0), ("dkv", "vit3"), ("dkv", "short"), ("dkv", "general"), ("dkv", "long"),
            ("dbias", "atomics", False), ("dbias", "sums", False), ("dbias", "short_planes", True), ("dbias", "blocks", True),
            ("dbias", "blocks", False), ("sums nb", 1), ("sums nb", 2), ("sums nb", 4),
            ("blocks entries", 1, False), ("blocks entries", 2, True)}
    assert want <= seen, sorted(want - seen, key=str)


# ----------------------------------------------------------------------------------------------------------------------- the bounds
@pytest.mark.parametrize("sp", SPECS, ids=A.spec_id)
def test_emulated_dense_kernels_stay_within_the_bounds(sp):
    c = _case(sp)
    fam_f = A.dense_families(sp.want)[0]
    fr = A.dense_fwd_ref(c, fam_f)
    o, o_lo, lse = _fwd_of(sp, c)
    _report(sp, "o", A.check_bf16(o, *fr["o"], "o"))
    _report(sp, "lse", A.check_f32(lse, *fr["lse"], "lse"))
    if o_lo is not None:
        _report(sp, "o+o_lo", A.check_o_lo(o, o_lo, *fr["o"]))
    if not sp.bwd:
        return
    if o_lo is None:
        v = fr["o"][0].float()
        o_lo = (v - v.to(BF16).float()).to(BF16)
    lse32 = fr["lse"][0].float()
    plans = {"": A.dense_plan(sp)}
    if sp.bias:
        plans["gather"] = A.dense_plan(sp, bias_t=False, have_ws=False)
    if sp.want.dq == "short":
        plans["pre+lo"] = A.dense_plan(sp, pre=True, o_lo=True)
    if sp.want.dq == "long":
        plans["lo"] = A.dense_plan(sp, o_lo=True)
    if sp.route == "short_slices":
        plans["det"] = A.dense_plan(sp, det=True)
    if sp.want.fwd == "vit13":
        plans["vit3"] = A.dense_plan(sp, tiled=True, vit_mode=3)
        if sp.bias:
            plans["vit4"] = A.dense_plan(sp, tiled=True, vit_mode=4)
    for tag, rt in plans.items():
        _, fam_q, fam_k = A.dense_families(rt)
        from_out = tag in ("pre+lo", "lo", "vit3", "vit4")
        assert (rt.dq == "vit3") == tag.startswith("vit")
        lo = torch.zeros_like(o_lo) if rt.dq == "vit3" else o_lo      # the single pass: dO . O with the bf16 O alone
        given = A.delta_out_ref(c, o, lo, A.C_DELTA_DOT if rt.dq == "short_pre" else A.C_DELTA_CHAIN) if from_out else None
        br = A.dense_bwd_ref(c, lse32, fam_q, fam_k, A.dense_flushes(sp, rt), given, fam_b="long" if tag == "vit4" else None,
                             delta_in_acc=rt.dq == "vit3")
        out = emul_dense_bwd(c, lse32, rt, (o, lo) if from_out else None)
        sfx = ":" + tag if tag else ""
        _report(sp, "delta" + sfx, A.check_f32(out["delta"], *br["delta"], "delta"))
        for name in ("dq", "dk", "dv"):
            _report(sp, name + sfx, A.check_bf16(out[name], *br[name], name))
        if sp.bias:
            _report(sp, "dbias" + sfx, A.check_f32(out["dbias"], *br["dbias"], "dbias"))


def test_dense_reference_is_the_masked_suites_reference():
    """dense_bwd_ref / dense_fwd_ref in the general family are bwd_ref / fwd_ref of the same case: values equal, bounds equal but for the
    bias-gradient's flush count."""
    sp = _spec("sums", "3x2x70x130")
    c = _case(sp)
    fr, fd = A.fwd_ref(c), A.dense_fwd_ref(c, "general")
    for name in ("o", "lse"):
        assert torch.equal(fr[name][0], fd[name][0]) and torch.allclose(fr[name][1], fd[name][1], rtol=1e-12, atol=0)
    lse32 = fr["lse"][0].float()
    br, bd = A.bwd_ref(c, lse32), A.dense_bwd_ref(c, lse32, "general", "general", 3)
    for name in ("delta", "dq", "dk", "dv", "dbias"):
        assert torch.allclose(br[name][0], bd[name][0], rtol=1e-13, atol=0), name
        if name != "dbias":
            assert torch.allclose(br[name][1], bd[name][1], rtol=1e-12, atol=0), name


# ------------------------------------------------------------------------------------------------------------------ planted faults
def _next_head(c):
    return torch.roll(c["bias"], -1, 0)


def test_bias_of_the_next_head_lands_past_the_bounds():
    sp = _spec("vit13", "2x2x197x197", "ld208")
    c = _case(sp)
    fr = A.dense_fwd_ref(c, "vit")
    o, _, _ = emul_vit_fwd(c, bias=_next_head(c))
    _fails(lambda: A.check_bf16(o, *fr["o"], "o"))
    lse32 = fr["lse"][0].float()
    br = A.dense_bwd_ref(c, lse32, "short_dq", "short_dkv", sp.want.slices)
    out = emul_dense_bwd(c, lse32, sp.want, bias=_next_head(c))
    _fails(lambda: A.check_bf16(out["dq"], *br["dq"], "dq"))
    _fails(lambda: A.check_bf16(out["dk"], *br["dk"], "dk"))


def test_bias_gradient_stored_or_a_plane_dropped_lands_past_the_bound():
    sp = _spec("short_slices", "9x2x40x40")
    c = _case(sp)
    rt = A.dense_plan(sp, det=True)
    assert rt.dbias == "short_planes" and rt.planes == 9
    lse32 = A.dense_fwd_ref(c, "general")["lse"][0].float()
    br = A.dense_bwd_ref(c, lse32, "short_dq", "short_dkv", rt.slices)
    A.check_f32(emul_dense_bwd(c, lse32, rt)["dbias"], *br["dbias"], "dbias")
    _fails(lambda: A.check_f32(emul_dense_bwd(c, lse32, rt, store_dbias=True)["dbias"], *br["dbias"], "dbias"))
    _fails(lambda: A.check_f32(emul_dense_bwd(c, lse32, rt, drop_slice=4)["dbias"], *br["dbias"], "dbias"))


def test_second_item_on_the_first_items_keys_lands_past_the_bound():
    sp = _spec("vit_walk", "87x3x70x70")
    c = _case(sp)
    fr = A.dense_fwd_ref(c, "vit")
    k = c["k"].clone()
    k[1, :, 0] = k[0, :, 0]          # items are head-major: (h 0, b 0), (h 0, b 1) share workgroup 0; the stale image is b 0's
    o, _, _ = emul_vit_fwd(c, k=k)
    _fails(lambda: A.check_bf16(o, *fr["o"], "o"))


def test_delta_from_the_wrong_half_lands_past_the_bound():
    sp = _spec("vit13", "2x2x197x197", "ld208")
    c = _case(sp)
    fr = A.dense_fwd_ref(c, "vit")
    o, o_lo, _ = emul_vit_fwd(c)
    lse32 = fr["lse"][0].float()
    rt = A.dense_plan(sp, pre=True, o_lo=True)
    given = A.delta_out_ref(c, o, o_lo, A.C_DELTA_DOT)
    br = A.dense_bwd_ref(c, lse32, "short_dq", "short_dkv", rt.slices, given)
    A.check_f32(emul_dense_bwd(c, lse32, rt, (o, o_lo))["delta"], *br["delta"], "delta")
    wrong = emul_dense_bwd(c, lse32, rt, (o, torch.zeros_like(o_lo)))
    _fails(lambda: A.check_f32(wrong["delta"], *br["delta"], "delta"))


@pytest.mark.parametrize("shape", ["2x2x65x65", "2x2x130x130"])
def test_last_key_tile_left_out_lands_past_the_bounds(shape):
    sp = _spec("vit_rt", shape, f"ld{A.cdiv(int(shape.split('x')[2]), 16) * 16}")
    c = _case(sp)
    fr = A.dense_fwd_ref(c, "vit")
    o, _, _ = emul_vit_fwd(c, drop_last_tile=True)
    _fails(lambda: A.check_bf16(o, *fr["o"], "o"))
    lse32 = fr["lse"][0].float()
    br = A.dense_bwd_ref(c, lse32, "short_dq", "short_dkv", sp.want.slices)
    out = emul_dense_bwd(c, lse32, sp.want, drop_last_tile=True)
    _fails(lambda: A.check_bf16(out["dv"], *br["dv"], "dv"))


def test_unscaled_bias_lands_past_the_bound():
    sp = _spec("vit_rt", "2x2x65x65", "ld80")
    c = _case(sp)
    fr = A.dense_fwd_ref(c, "vit")
    o, _, _ = emul_vit_fwd(c, unscaled_bias=True)
    _fails(lambda: A.check_bf16(o, *fr["o"], "o"))


def test_max_norm_check_misses_what_the_dense_bounds_catch():
    """tests/test_hip_kernels.py holds the dense kernels to max |err| / max |ref| <= 1e-2 (forward) and 2e-2 (backward).  Two of the faults
    above pass that: delta taken from dO . O where dO . (O + O_lo) is defined (what it does to dq and dk), and a bias gradient stored
    instead of added, which a gradient that starts at zero cannot show at all."""
    sp = _spec("vit13", "2x2x197x197", "ld208")
    c = _case(sp)
    fr = A.dense_fwd_ref(c, "vit")
    o, o_lo, _ = emul_vit_fwd(c)
    lse32 = fr["lse"][0].float()
    rt = A.dense_plan(sp, pre=True, o_lo=True)
    br = A.dense_bwd_ref(c, lse32, "short_dq", "short_dkv", rt.slices, A.delta_out_ref(c, o, o_lo, A.C_DELTA_DOT))
    wrong = emul_dense_bwd(c, lse32, rt, (o, torch.zeros_like(o_lo)))
    _fails(lambda: A.check_f32(wrong["delta"], *br["delta"], "delta"))
    for name, tol in (("dq", 2e-2), ("dk", 2e-2)):
        err = A.max_norm_err(wrong[name], br[name][0])
        print(f"attn-maxnorm host delta-from-dO.O {name} {err:.3g}")
        assert err <= tol, (name, err)

    # `=` for `+=` where one slice owns its block of dbias (the long route without a workspace): on a gradient that starts at zero, as
    # in tests/test_hip_kernels.py, the stored sum IS the added one
    sp = _spec("long", "2x2x40x300", "ld304")
    c = _case(sp)
    rt = A.dense_plan(sp, bias_t=False, have_ws=False)
    assert rt.dbias == "blocks" and rt.slices == 1 and rt.planes == 0
    lse32 = A.dense_fwd_ref(c, "general")["lse"][0].float()
    br = A.dense_bwd_ref(c, lse32, "long", "general", 1)
    stored = emul_dense_bwd(c, lse32, rt, store_dbias=True)["dbias"]
    _fails(lambda: A.check_f32(stored, *br["dbias"], "dbias"))
    from_zero = emul_dense_bwd(c, lse32, rt, dbias_init=0.0)["dbias"]
    err = A.max_norm_err(stored, from_zero.double())
    print(f"attn-maxnorm host dbias-stored-from-zero dbias {err:.3g}")
    assert err <= 2e-2, err
