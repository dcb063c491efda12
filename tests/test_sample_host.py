"""Host side of the fused sampling step without a GPU: ABI 18 and the argument checks of xfm_sample_token, the fp64 restatement
(sample_util) against the reference's own top_k_top_p_filtering (tests/golden/sampling_filter.npz; tools/oracle/gen_sampling.py), and
hand-worked draws."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from golden_util import load
from sample_util import DELTA, draw_ref, filter_ref, sample_ref, tempered64, token_accepted
from xfm_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -float("inf")


def test_abi_18_and_the_new_symbol():
    from xfm_amd import _lib
    assert _lib.ABI_VERSION >= 18
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "xfm_hip.h")) as f:
        hdr = f.read()
    assert f"#define XFM_ABI_VERSION {_lib.ABI_VERSION}" in hdr
    assert "xfm_sample_token" in _lib.SIGNATURES and lib.xfm_sample_token is not None and "int xfm_sample_token(" in hdr
    assert "xbert.py:1422-1462" in hdr and ":1487-1519" in hdr and "ASCENDING COLUMN ORDER" in hdr
    # the binding's struct against the header's field list, in order
    body = hdr[hdr.index("typedef struct {", hdr.index("xfm_sample_token (ABI 18)")):hdr.index("} xfm_sample_token_args;")]
    fields = []
    for stmt in re.sub(r"/\*.*?\*/", "", body[len("typedef struct {"):], flags=re.S).split(";"):
        fields += [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", part).group(1) for part in stmt.split(",") if part.strip()]
    assert fields == [n for n, _ in _lib.SampleTokenArgs._fields_]
    from xfm_amd import functional as Fx
    assert callable(Fx.sample_token)


def _args(**kw):
    from xfm_amd._lib import SampleTokenArgs
    P = 0x10000   # non-NULL, never read: every case below is refused before anything is launched
    a = dict(logits=P, ld=64, V=50, ids=P, ids_ld=9, cur_len=3, penalty=1.0, temperature=1.0, top_k=0, top_p=1.0, unfinished=P,
             hist_unfinished=P, hist_logprob=P, hist_ld=4, step=1, pad_id=1, n_eos=1, B=2)
    a.update(kw)
    return SampleTokenArgs(**a)


@pytest.mark.parametrize("bad,word", [(dict(cur_len=9), b"cur_len"), (dict(cur_len=-1), b"cur_len"), (dict(step=4), b"step"),
                                      (dict(V=65), b"V="), (dict(V=131073, ld=131080), b"exceeds"), (dict(n_eos=9), b"eos"),
                                      (dict(penalty=0.0), b"penalty"), (dict(logits=0), b"null"), (dict(ids=0), b"null"),
                                      (dict(temperature=0.0), b"temperature"), (dict(temperature=-1.0), b"temperature"),
                                      (dict(temperature=float("inf")), b"temperature"), (dict(temperature=float("nan")), b"temperature"),
                                      (dict(top_p=0.0), b"top_p"), (dict(top_p=1.5), b"top_p"), (dict(top_p=float("nan")), b"top_p"),
                                      (dict(top_k=-1), b"top_k"), (dict(filtered=0x10000, filtered_ld=49), b"filtered")])
def test_sample_token_refuses_bad_arguments(bad, word):
    """Every XFM_E_ARG case of the contract: an error code, a message that names the argument, and no launch (no device is needed)."""
    from xfm_amd import _lib
    lib = _lib.load()
    a = _args(**bad)
    assert lib.xfm_sample_token(ctypes.byref(a), None) == -1
    msg = lib.xfm_last_error()
    assert b"sample_token" in msg and word in msg, msg
    assert lib.xfm_sample_token(None, None) == -1


def test_cpu_tensors_raise():
    from xfm_amd import _lib
    from xfm_amd import functional as Fx
    with pytest.raises(_lib.XfmHipError):
        Fx.sample_token(torch.zeros(2, 8), 8, torch.zeros(2, 4, dtype=torch.int64), 1, torch.ones(2, dtype=torch.int32),
                        torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3), 0, 1, [2], 1.0, 0, 1.0, 7)


def test_restatement_reproduces_the_reference_filter():
    """sample_util.filter_ref on the fixture's formula rows: on the sharp cases the reference's kept mask bit for bit (and n_lo == n_hi);
    on the flat case the reference's fp32 count lies in [n_lo, n_hi] and its kept set is a prefix of the tie-ruled order."""
    z, meta = load("sampling_filter")
    V, rows = meta["V"], meta["rows"]
    assert meta["delta"] == DELTA
    settings = {(c["top_k"], c["top_p"], c["temperature"]) for c in meta["cases"]}
    assert {(50, 0.9, 0.7), (0, 0.9, 1.0), (0, 0.5, 1.0), (5, 1.0, 1.0)} <= settings and any(c["flat"] for c in meta["cases"])
    ids = torch.zeros(rows, 1, dtype=torch.int64)
    for i, c in enumerate(meta["cases"]):
        logits = syn.gaussian(c["name"], (rows, V), c["scale"])
        z64, _ = tempered64(logits, V, ids, 0, 1.0, c["temperature"])
        want = torch.from_numpy(np.unpackbits(z[f"kept/{i}"], axis=1)[:, :V].astype(bool))
        count = z[f"count/{i}"].tolist()
        assert want.sum(1).tolist() == count
        for r in range(rows):
            f = filter_ref(z64[r], c["top_k"], c["top_p"])
            if c["flat"]:
                assert f["n_lo"] < f["n_hi"], "the flat case is meant to have positions inside the band"
                assert f["n_lo"] <= count[r] <= f["n_hi"], (i, r, f["n_lo"], count[r], f["n_hi"])
                assert bool(want[r][f["order"][:count[r]]].all())
            else:
                assert f["n_lo"] == f["n_hi"] == f["n"], (i, r, f["n_lo"], f["n"], f["n_hi"])
                assert torch.equal(f["kept"], want[r]), (i, r, int(f["kept"].sum()), count[r])


def test_filter_rules_by_hand():
    """Equal values at the top-k cut all stay; equal values inside the nucleus leave in descending column order."""
    zrow = torch.tensor([1.0, 3.0, 2.0, 2.0, NEG, 2.0, 0.0], dtype=torch.float64)
    f = filter_ref(zrow, 2, 1.0)
    assert f["kept"].tolist() == [False, True, True, True, False, True, False] and f["order"].tolist() == [1, 2, 3, 5]
    four = torch.tensor([NEG, 0.0, 0.0, NEG, 0.0, 0.0], dtype=torch.float64)   # p = 1/4 each: c = .25 .5 .75 1
    assert filter_ref(four, 0, 0.6)["kept"].tolist() == [False, True, True, False, True, False]   # c[i-1] <= 0.6: positions 0, 1, 2
    assert filter_ref(four, 0, 0.5)["kept"].tolist() == [False, True, True, False, True, False]   # c[1] = 0.5 <= 0.5 keeps position 2
    assert filter_ref(four, 0, 0.4)["kept"].tolist() == [False, True, True, False, False, False]
    assert filter_ref(four, 0, 1e-6)["kept"].tolist() == [False, True, False, False, False, False]
    assert filter_ref(four, 1, 1.0)["kept"].tolist() == [False, True, True, False, True, True]


def test_draws_by_hand():
    """Four columns at logit 0, the rest -inf: u = 0.3 draws the second finite column, u = 0 the first, and u Z exactly equal to a
    running sum draws the NEXT kept column (the comparison is a strict >)."""
    zrow = torch.full((9,), NEG, dtype=torch.float64)
    cols = [1, 4, 5, 8]
    zrow[cols] = 0.0
    kept = torch.isfinite(zrow)
    assert draw_ref(zrow, kept, 0.3)["tok"] == cols[1]
    assert draw_ref(zrow, kept, 0.0)["tok"] == cols[0]
    assert draw_ref(zrow, kept, 0.25)["tok"] == cols[1] and draw_ref(zrow, kept, 0.5)["tok"] == cols[2] and draw_ref(zrow, kept, 0.75)["tok"] == cols[3]
    d = draw_ref(zrow, kept, 0.999999)
    assert d["tok"] == cols[3] and abs(d["lp"] - float(np.log(0.25))) < 1e-12
    assert token_accepted(d["C"], kept, cols[3], 0.999999) and not token_accepted(d["C"], kept, cols[0], 0.999999)
    assert not token_accepted(d["C"], kept, 0, 0.0)   # a column that is not kept is never accepted


def test_whole_step_restatement():
    """sample_ref: the penalty once per distinct id, the temperature, the filter, the draw, and next_token_ref's bookkeeping (pad for a
    finished row, eos clears the flag); a row without a finite value gives token 0 and NaN."""
    x = torch.tensor([[2.0, 4.0, 4.0, -2.0], [0.5, 0.25, 3.0, -1.0], [9.0, 0.0, 0.0, 0.0], [NEG, NEG, NEG, NEG]])
    ids = torch.tensor([[3, 3, 0], [2, 2, 2], [1, 1, 1], [0, 0, 0]])
    r = sample_ref(x, 4, ids, 3, 2.0, 0.5, 2, 1.0, torch.tensor([0.0, 0.99, 0.5, 0.5]), torch.tensor([1, 1, 0, 1]), 7, [1])
    assert r["z"][0].tolist() == [2.0, 8.0, 8.0, -8.0] and r["z"][1].tolist() == [1.0, 0.5, 3.0, -2.0]
    assert r["rows"][0]["kept"].tolist() == [False, True, True, False] and r["rows"][1]["kept"].tolist() == [True, False, True, False]
    assert r["tok"].tolist() == [1, 2, 0, 0] and r["add"].tolist() == [1, 2, 7, 0] and r["unfinished"].tolist() == [0, 1, 0, 1]
    assert r["count"] == 2 and r["rows"][3]["bad"] and np.isnan(r["rows"][3]["lp"])
    assert abs(r["rows"][0]["lp"] - float(np.log(0.5))) < 1e-12 and r["rows"][0]["b_lp"] > 0
