"""Host-side proof that the ragged-rows section of attention_util holds for a correct fp32 evaluation and bites for a wrong one (CPU, no GPU).

1. The ragged reference agrees with torch autograd in fp64 on the truncated problem: per entry a softmax over its live keys alone (the
   additive -10000 on masked / causally hidden LOCAL keys, nothing for the keys past k_len: they are not there), grouped dk / dv summed
   over the live rows of a source's entries.
2. The fp32 emulation of tests/test_attention_host.py, run per entry on the truncated operands (grouped: per source on the concatenated
   live rows of its entries, one bf16 rounding of the summed dk / dv as the grouped kernel makes), stays within every bound of every case
   of attention_util.ragged_specs(), without o_lo and with it (delta = dO . (O + O_lo) in fp32), at no more than HOST_MAX = 0.9, and prints
   `attn-ratio host <quantity> <family> <ratio>`.
3. Planted faults land past the bound: a key past k_len admitted; -10000 in place of exclusion where every live key is masked; the causal
   test on the buffer row instead of the local index; the last live query row read from row q_len; key_keep strided by k_len; the
   dropout row counter laid out for q_len; a grouped dk that takes a row past q_len; delta from o without o_lo.
4. test_norm_relative_check_misses_what_the_bound_catches: the measure of tests/test_hip_packing.py passes some of them."""
import functools

import pytest
import torch

import attention_util as A
from attention_util import BF16, SCALE
from test_attention_host import HOST_MAX, _h32, emul_bwd, emul_fwd, emul_scores, host_mask

SPECS = A.ragged_specs()
CHECK = {"o": A.check_bf16, "lse": A.check_f32, "delta": A.check_f32, "dq": A.check_bf16, "dk": A.check_bf16, "dv": A.check_bf16}
SIDE = {"o": "q", "lse": "stat", "delta": "stat", "dq": "q", "dk": "k", "dv": "k"}


@functools.lru_cache(maxsize=8)
def _case(sp):
    return A.make_ragged_case(sp)


def _spec(route, variant, ragged=True, U=2):
    return next(s for s in SPECS if s.route == route and s.name.startswith(variant + ":") and (s.q_len is not None) == ragged and s.U in (U, s.B))


def _check(sp, name, got, pair):
    """the checker of `name` on what the kernels own (ragged_live)"""
    live = A.ragged_live(sp)[SIDE[name]]
    g = got[:, :sp.Sq] if SIDE[name] == "stat" else got
    return CHECK[name](g[live], pair[0][live], pair[1][live], name)


def _report(sp, what, ratio, limit=HOST_MAX):
    print(f"attn-ratio host {what} {A.spec_id(sp)} {ratio:.3g}")
    assert ratio <= limit, f"{A.spec_id(sp)} {what}: a correct fp32 evaluation at {ratio:.3g} of the bound: the derivation misses a rounding"


def _fault(sp, what, fn):
    with pytest.raises(AssertionError, match="past the bound") as e:
        fn()
    ratio = float(str(e.value).rsplit("=", 1)[1])
    print(f"attn-fault host {A.spec_id(sp)} {what} {ratio:.3g}")
    assert ratio > 1.0


# ------------------------------------------------------------------------------------------------------------------- fp32 emulation
def emul_o32(c, M=None):
    """fp32 o [Sq, H*64] of one entry before its bf16 rounding (a plain softmax: the halves o, o_lo the delta-from-output backward reads)"""
    sp = c["sp"]
    p = torch.softmax(emul_scores(c), -1)
    if M is not None:
        p = torch.where(M, p * A.drop_scale32(sp.p), torch.zeros(()))
    o = p.to(BF16).float() @ _h32(c["v"])
    return o.permute(0, 2, 1, 3).reshape(sp.Sq, sp.H * 64)


def emul_bwd_given(c, lse32, delta32, M=None):
    """emul_bwd with delta given (fp32 [H, Sq]) instead of sum_j P dP: the dQ kernels' fast_delta branch; dk / dv form dS from the same"""
    sp = c["sp"]
    H, Sq, Sk = sp.H, sp.Sq, sp.Sk
    Q, K, V, DO = _h32(c["q"]), _h32(c["k"]), _h32(c["v"]), _h32(c["do"])
    P = torch.exp(emul_scores(c) - lse32.reshape(1, H, Sq, 1))
    f = torch.ones(()) if M is None else torch.where(M, A.drop_scale32(sp.p) * torch.ones(()), torch.zeros(()))
    ds = P * ((DO @ V.transpose(-1, -2)) * f - delta32.reshape(1, H, Sq, 1))
    dq = ((ds.to(BF16).float() @ K) * SCALE).to(BF16)
    dk = ((ds.to(BF16).float().transpose(-1, -2) @ Q) * SCALE).to(BF16)
    dv = ((P * f).to(BF16).float().transpose(-1, -2) @ DO).to(BF16)
    rows = lambda t, S: t.permute(0, 2, 1, 3).reshape(S, H * 64)   # noqa: E731
    return {"delta": delta32.reshape(H, Sq), "dq": rows(dq, Sq), "dk": rows(dk, Sk), "dv": rows(dv, Sk)}


def emul_halves(c, M=None):
    """(o, o_lo) bf16 [q_rows, H*64] in the buffer's layout, zeros in the slack rows"""
    sp = c["sp"]
    lay = A.ragged_layout(sp)
    o, lo = (torch.zeros((lay.q_rows, sp.H * 64), dtype=BF16) for _ in range(2))
    for b in range(sp.B):
        cb, Mb = A.entry_case(c, b, M)
        v = emul_o32(cb, Mb)
        s, n = lay.q_start[b], lay.q_len[b]
        o[s:s + n] = v.to(BF16)
        lo[s:s + n] = (v - v.to(BF16).float()).to(BF16)
    return o, lo


def emul_ragged_fwd(c, M=None, plant=None):
    """-> (o bf16 [q_rows, H*64], lse fp32 [B*H, Sq]).  plant(b, cb, Mb) -> (cb, Mb, emul_fwd's fault arguments) or None"""
    sp = c["sp"]
    lay = A.ragged_layout(sp)
    o = torch.zeros((lay.q_rows, sp.H * 64), dtype=BF16)
    lse = torch.zeros((sp.B * sp.H, sp.Sq))
    for b in range(sp.B):
        cb, Mb = A.entry_case(c, b, M)
        kw = {}
        if plant is not None and plant(b, cb, Mb) is not None:
            cb, Mb, kw = plant(b, cb, Mb)
        ob, lb = emul_fwd(cb, Mb, **kw)
        s, n = lay.q_start[b], lay.q_len[b]
        o[s:s + n] = ob
        A._stat_rows(lse, sp, b, n).copy_(lb)
    return o, lse


def _group_case(c, u, lse32, M, halves, extra):
    """the entries of source u as ONE entry: their live query rows one after the other (attention rows are independent, and dk / dv are
    then summed over all of them in fp32 and rounded once, as xattn_dkv_kernel does).  extra: {b: rows past q_len taken along}"""
    sp = c["sp"]
    lay = A.ragged_layout(sp)
    bs = [b for b in range(sp.B) if int(c["idx"][b]) == u]
    n = {b: lay.q_len[b] + extra.get(b, 0) for b in bs}
    cat = lambda t: torch.cat([t[b:b + 1, :n[b]] for b in bs], 1)   # noqa: E731
    spg = A.Spec(sp.route, 1, sp.H, sum(n.values()), sp.Sk, 1, None, True, sp.mask, False, sp.p, sp.score, False, sp.name)
    cg = {"sp": spg, "q": cat(c["q"]), "do": cat(c["do"]), "k": c["k"][u:u + 1], "v": c["v"][u:u + 1], "bias": None,
          "keep": None if c["keep"] is None else c["keep"][u:u + 1], "idx": torch.zeros(1, dtype=torch.int64)}
    Mg = None if M is None else torch.cat([M[b:b + 1, :, :n[b]] for b in bs], 2)
    lse = []
    for b in bs:      # a row past q_len has no statistic of its own: the one a forward over it would have left
        full = A.fwd_ref(*A.entry_case(c, b, M, q_len=n[b]))["lse"][0].float()
        full[:, :lay.q_len[b]] = A._stat_rows(lse32, sp, b, lay.q_len[b])
        lse.append(full)
    dl = None
    if halves is not None:
        rows = torch.cat([torch.arange(lay.q_start[b], lay.q_start[b] + n[b]) for b in bs])
        dl = (cg["do"].float().reshape(-1, sp.H, 64) * (halves[0][rows].float() + halves[1][rows].float()).reshape(-1, sp.H, 64)).sum(-1).t()
    return cg, Mg, torch.cat(lse, 1), dl, bs, n


def emul_ragged_bwd(c, lse32, M=None, halves=None, plant=None, extra=None):
    """-> delta [B*H, Sq], dq [q_rows, .], dk / dv [k_rows, .].  halves: (o, o_lo) -> delta from the output.  plant as in emul_ragged_fwd
    (self-attention and range mode); extra: rows past q_len a grouped dk / dv takes along (a fault)"""
    sp = c["sp"]
    lay = A.ragged_layout(sp)
    D = sp.H * 64
    out = {"delta": torch.zeros((sp.B * sp.H, sp.Sq)), "dq": torch.zeros((lay.q_rows, D), dtype=BF16),
           "dk": torch.zeros((lay.k_rows, D), dtype=BF16), "dv": torch.zeros((lay.k_rows, D), dtype=BF16)}
    if sp.grouped:
        for u in range(sp.U):
            if not bool((c["idx"] == u).any()):
                continue
            cg, Mg, lse, dl, bs, n = _group_case(c, u, lse32, M, halves, extra or {})
            got = emul_bwd(cg, lse, Mg) if dl is None else emul_bwd_given(cg, lse, dl, Mg)
            at = 0
            for b in bs:
                s, ql = lay.q_start[b], lay.q_len[b]
                A._stat_rows(out["delta"], sp, b, ql).copy_(got["delta"][:, at:at + ql])
                out["dq"][s:s + ql] = got["dq"][at:at + ql]
                at += n[b]
            out["dk"][u * sp.Sk:(u + 1) * sp.Sk], out["dv"][u * sp.Sk:(u + 1) * sp.Sk] = got["dk"], got["dv"]
        return out
    for b in range(sp.B):
        cb, Mb = A.entry_case(c, b, M)
        kw = {}
        if plant is not None and plant(b, cb, Mb) is not None:
            cb, Mb, kw = plant(b, cb, Mb)
        s, n = lay.q_start[b], lay.q_len[b]
        lse = A._stat_rows(lse32, sp, b, n).reshape(sp.H, n)
        if halves is None:
            got = emul_bwd(cb, lse, Mb, **kw)
        else:
            dl = (cb["do"].float().reshape(n, sp.H, 64) * (halves[0][s:s + n].float() + halves[1][s:s + n].float()).reshape(n, sp.H, 64)).sum(-1).t()
            got = emul_bwd_given(cb, lse, dl, Mb)
        ks, kn = lay.k_start[b], lay.k_len[b]
        A._stat_rows(out["delta"], sp, b, n).copy_(got["delta"])
        out["dq"][s:s + n], out["dk"][ks:ks + kn], out["dv"][ks:ks + kn] = got["dq"], got["dk"][:kn], got["dv"][:kn]
    return out


# ----------------------------------------------------------------------------------------------------------------------- 1. autograd
@pytest.mark.parametrize("sp", [s for s in SPECS if s.p == 0.0], ids=A.spec_id)
def test_ragged_reference_agrees_with_autograd(sp):
    c = _case(sp)
    lay = A.ragged_layout(sp)
    fr = A.ragged_fwd_ref(c)
    br = A.ragged_bwd_ref(c, fr["lse"][0])      # the exact lse: the backward is then the gradient of the forward
    D = sp.H * 64
    want = {"dk": torch.zeros((lay.k_rows, D), dtype=torch.float64), "dv": torch.zeros((lay.k_rows, D), dtype=torch.float64)}

    def rel(got, ref):
        return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))

    for b in range(sp.B):
        cb, _ = A.entry_case(c, b)
        src = int(c["idx"][b])
        n, kn = lay.q_len[b], lay.k_len[src]
        leaf = lambda t: t.double().clone().requires_grad_(True)   # noqa: E731
        q, k, v = leaf(cb["q"]), leaf(cb["k"]), leaf(cb["v"])
        s = SCALE * (q.permute(0, 2, 1, 3) @ k.permute(0, 2, 3, 1)) + A.MASK_NEG * A.masked_of(cb).double()
        o = (s.softmax(-1) @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(n, D)
        o.backward(cb["do"].double().reshape(n, D))
        rows = slice(lay.q_start[b], lay.q_start[b] + n)
        assert rel(fr["o"][0][rows], o.detach()) <= 1e-12
        assert rel(br["dq"][0][rows], q.grad.reshape(n, D)) <= 1e-12
        want["dk"][lay.k_start[src]:lay.k_start[src] + kn] += k.grad.reshape(kn, D)
        want["dv"][lay.k_start[src]:lay.k_start[src] + kn] += v.grad.reshape(kn, D)
    for name in ("dk", "dv"):
        assert rel(br[name][0], want[name]) <= 1e-12, name
        assert bool((br[name][0][~A.ragged_live(sp)["k"]] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------- 2. emulation
@pytest.mark.parametrize("sp", SPECS, ids=A.spec_id)
def test_ragged_emulation_within_bounds(sp):
    c = _case(sp)
    M = host_mask(sp)
    fr = A.ragged_fwd_ref(c, M)
    o, lse = emul_ragged_fwd(c, M)
    _report(sp, "o", _check(sp, "o", o, fr["o"]))
    _report(sp, "lse", _check(sp, "lse", lse, fr["lse"]))
    halves = emul_halves(c, M)
    live = A.ragged_live(sp)["q"]
    # (not emul_fwd's output: the halves of emul_o32, held to the bound itself.  With no bf16 rounding of the output to absorb it, the one
    # bf16 rounding of P IS the error of an entry of two or three live keys, and u16 = 2^-8 is exactly bf16's unit roundoff: 0.906 at k_len 3)
    _report(sp, "o+o_lo", A.check_o_lo(halves[0][live], halves[1][live], fr["o"][0][live], fr["o"][1][live]), 1.0)
    lse32 = A.ragged_lse32(fr, sp)
    for tag, hv in (("", None), (":lo", halves)):
        br = A.ragged_bwd_ref(c, lse32, M, *(hv or ()))
        got = emul_ragged_bwd(c, lse32, M, hv)
        for name, t in got.items():
            _report(sp, name + tag, _check(sp, name, t, br[name]))


# -------------------------------------------------------------------------------------------------------------------------- 3. faults
def _only(entry, fn):
    return lambda b, cb, Mb: fn(cb, Mb) if b == entry else None


def test_fault_one_key_past_k_len_admitted():
    sp = _spec("streamed", "holes")      # entry 1: 257 of 300 keys; key 257 is one the holes keep
    c = _case(sp)
    fr = A.ragged_fwd_ref(c)
    plant = _only(1, lambda cb, Mb: A.entry_case(c, 1, k_len=258) + ({},))
    o, lse = emul_ragged_fwd(c, plant=plant)
    _fault(sp, "key k_len admitted:lse", lambda: _check(sp, "lse", lse, fr["lse"]))
    _fault(sp, "key k_len admitted:o", lambda: _check(sp, "o", o, fr["o"]))


def test_fault_minus_10000_in_place_of_exclusion():
    """every live key of entry 0 masked: exclusion leaves a softmax over its 64 live keys, the additive form one over all 130"""
    sp = A.ragged_spec("resident", 2, 70, 130, 2, None, False, "holes", (33, 70), (64, 130))._replace(mask="all", name="all:q33.70:k64.130")
    c = A.make_ragged_case(sp)
    fr = A.ragged_fwd_ref(c)
    o, lse = emul_ragged_fwd(c)
    _check(sp, "o", o, fr["o"]), _check(sp, "lse", lse, fr["lse"])
    o, lse = emul_ragged_fwd(c, plant=_only(0, lambda cb, Mb: A.entry_case(c, 0, k_len=130) + ({},)))
    _fault(sp, "-10000 past k_len:lse", lambda: _check(sp, "lse", lse, fr["lse"]))
    _fault(sp, "-10000 past k_len:o", lambda: _check(sp, "o", o, fr["o"]))


def test_fault_causal_on_buffer_rows():
    sp = _spec("causal", "causal+holes+p0.1")      # 3 x 65 x 65, lens (65, 64, 1); entry 0 starts at row 68 of the buffer
    c = _case(sp)
    M = host_mask(sp)
    fr = A.ragged_fwd_ref(c, M)
    start = A.ragged_layout(sp).q_start[0]
    plant = _only(0, lambda cb, Mb: (cb, Mb, {"causal_shift": start}))
    o, lse = emul_ragged_fwd(c, M, plant=plant)
    _fault(sp, "causal on q_start + qi:o", lambda: _check(sp, "o", o, fr["o"]))
    _fault(sp, "causal on q_start + qi:lse", lambda: _check(sp, "lse", lse, fr["lse"]))
    lse32 = A.ragged_lse32(fr, sp)
    br = A.ragged_bwd_ref(c, lse32, M)
    got = emul_ragged_bwd(c, lse32, M, plant=plant)
    _fault(sp, "causal on q_start + qi:dq", lambda: _check(sp, "dq", got["dq"], br["dq"]))


def test_fault_last_live_row_read_from_row_q_len():
    sp = _spec("streamed", "holes")      # entry 1: 16 of 40 queries

    def plant(cb, Mb):
        cb = dict(cb, q=cb["q"].clone())
        cb["q"][0, 15] = c["q"][1, 16]
        return cb, Mb, {}

    c = _case(sp)
    fr = A.ragged_fwd_ref(c)
    o, lse = emul_ragged_fwd(c, plant=_only(1, plant))
    _fault(sp, "qc = q_len:o", lambda: _check(sp, "o", o, fr["o"]))
    lse32 = A.ragged_lse32(fr, sp)
    br = A.ragged_bwd_ref(c, lse32)
    got = emul_ragged_bwd(c, lse32, plant=_only(1, plant))
    _fault(sp, "qc = q_len:dq", lambda: _check(sp, "dq", got["dq"], br["dq"]))


def test_fault_key_keep_strided_by_k_len():
    sp = _spec("resident", "holes")      # entry 1: 64 of 130 keys
    c = _case(sp)
    fr = A.ragged_fwd_ref(c)
    plant = _only(1, lambda cb, Mb: (dict(cb, keep=c["keep"].reshape(-1)[64:128][None]), Mb, {}))
    o, lse = emul_ragged_fwd(c, plant=plant)
    _fault(sp, "keep + b k_len:o", lambda: _check(sp, "o", o, fr["o"]))
    _fault(sp, "keep + b k_len:lse", lambda: _check(sp, "lse", lse, fr["lse"]))
    lse32 = A.ragged_lse32(fr, sp)
    br = A.ragged_bwd_ref(c, lse32)
    got = emul_ragged_bwd(c, lse32, plant=plant)
    _fault(sp, "keep + b k_len:dk", lambda: _check(sp, "dk", got["dk"], br["dk"]))


def test_fault_dropout_counter_laid_out_for_q_len():
    sp = _spec("resident", "holes+p0.1")      # entry 1: 33 of 70 queries
    c = _case(sp)
    M = host_mask(sp)
    rows = M.reshape(sp.B * sp.H * sp.Sq, sp.Sk)
    wrong = torch.stack([rows[(1 * sp.H + h) * 33:(1 * sp.H + h) * 33 + 33, :64] for h in range(sp.H)])[None]
    fr = A.ragged_fwd_ref(c, M)
    plant = _only(1, lambda cb, Mb: (cb, wrong, {}))
    o, _ = emul_ragged_fwd(c, M, plant=plant)
    _fault(sp, "row key (b H + h) q_len + qi:o", lambda: _check(sp, "o", o, fr["o"]))
    lse32 = A.ragged_lse32(fr, sp)
    br = A.ragged_bwd_ref(c, lse32, M)
    got = emul_ragged_bwd(c, lse32, M, plant=plant)
    _fault(sp, "row key (b H + h) q_len + qi:dv", lambda: _check(sp, "dv", got["dv"], br["dv"]))


def test_fault_grouped_dk_takes_a_row_past_q_len():
    sp = _spec("grouped", "holes")      # entry 2: 16 of 30 queries, source 1
    c = _case(sp)
    fr = A.ragged_fwd_ref(c)
    lse32 = A.ragged_lse32(fr, sp)
    br = A.ragged_bwd_ref(c, lse32)
    got = emul_ragged_bwd(c, lse32)
    _check(sp, "dk", got["dk"], br["dk"])
    got = emul_ragged_bwd(c, lse32, extra={2: 1})
    _check(sp, "dq", got["dq"], br["dq"])      # the query side is untouched
    _fault(sp, "row q_len in dk:dk", lambda: _check(sp, "dk", got["dk"], br["dk"]))
    _fault(sp, "row q_len in dk:dv", lambda: _check(sp, "dv", got["dv"], br["dv"]))


def _delta_without_o_lo(sp):
    c = _case(sp)
    M = host_mask(sp)
    fr = A.ragged_fwd_ref(c, M)
    lse32 = A.ragged_lse32(fr, sp)
    o, lo = emul_halves(c, M)
    br = A.ragged_bwd_ref(c, lse32, M, o, lo)
    return br, emul_ragged_bwd(c, lse32, M, (o, torch.zeros_like(lo)))


@pytest.mark.parametrize("route,ragged", [("resident", True), ("streamed", False), ("grouped", True), ("grouped_stream", False)])
def test_fault_delta_from_o_without_o_lo(route, ragged):
    sp = _spec(route, "holes+p0.1", ragged)
    br, got = _delta_without_o_lo(sp)
    _fault(sp, "delta = dO . O:delta", lambda: _check(sp, "delta", got["delta"], br["delta"]))


# ---------------------------------------------------------------------------------------------------------------- 4. why the bounds
def test_norm_relative_check_misses_what_the_bound_catches():
    """tests/test_hip_packing.py holds ||packed - padded|| / ||padded|| to 2e-3 (outputs) and 5e-3 (gradients).  A delta formed without o_lo
    passes 5e-3 on dq, dk and dv, against a correct bf16 evaluation and against fp64; the elementwise bound catches it on delta.  (A key
    past k_len admitted into every row of an entry is at 3e-2 of the norm: that one the old measure sees too.)"""
    sp = _spec("resident", "holes+p0.1")
    br, got = _delta_without_o_lo(sp)
    c, M = _case(sp), host_mask(sp)
    ok = emul_ragged_bwd(c, A.ragged_lse32(A.ragged_fwd_ref(c, M), sp), M, emul_halves(c, M))      # the correct evaluation: the "padded run"
    for name in ("dq", "dk", "dv"):
        live = A.ragged_live(sp)[SIDE[name]]
        nr, nr64 = A.norm_rel(got[name][live], ok[name][live]), A.norm_rel(got[name][live], br[name][0][live])
        print(f"attn-normrel host delta without o_lo {name} {nr:.3g} (against fp64: {nr64:.3g})")
        assert nr <= 5e-3 and nr64 <= 5e-3
    with pytest.raises(AssertionError, match="past the bound"):
        _check(sp, "delta", got["delta"], br["delta"])
