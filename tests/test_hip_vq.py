"""xfm_vq_assign on a real MI355X against the fp64 restatement and the derived bound of tests/vq_util.py (its header has the derivation
and the decided / undecided rule; nothing is fitted to the kernel's output).  Every operand is a strided slice of a poisoned parent, and
every parent is checked as untouched outside the view.

  grid          M in {1, 63, 65, 200} x n_code in {1, 33, 257, 1000} at K = 32 (one row, a tile minus one, a tile plus one, four tiles;
                one code, under a wave's 32, two chunks and a bit, eight chunks minus 24), K = 8 and K = 64 at (200, 257).
  |e|^2         a codebook with row norms in [0.5, 2]: the nearest code by angle is not the nearest code.
  ties          equal codebook rows at i < j inside one staging chunk and across two: i, never j.
  edge rows     an all-zero row takes the smallest-norm code; a NaN row and an inf row get an index in range.
  histogram     counts == bincount(index), accumulating over two calls.
  determinism   two launches, and a fresh child process under XFM_DETERMINISTIC=1: equal bits."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from vq_util import GRID, WIDTHS, VqBuffers, check_indices, make_case, unit_rows, vq_digest, vq_ref64  # noqa: E402


@pytest.mark.parametrize("M,n_code,K", [(M, n, 32) for M, n in GRID] + WIDTHS)
def test_vq_assign_matches_fp64_argmin(M, n_code, K):
    z, code, ref = make_case(M, n_code, K)
    b = VqBuffers(z, code, "cuda", counts=True)
    got = b.run()
    torch.cuda.synchronize()
    und = check_indices(got, ref, f"M={M} n_code={n_code} K={K}")
    print(f"M={M} n_code={n_code} K={K}: undecided rows {und}, smallest gap / 2B {float((ref['gap'] / (2 * ref['B'])).min()):.3g}")
    assert torch.equal(b.counts.cpu().long(), torch.bincount(got.cpu(), minlength=n_code))
    b.assert_untouched()
    first = got.clone()
    again = b.run()
    assert torch.equal(again, first), "two launches differ"
    assert torch.equal(b.counts.cpu().long(), 2 * torch.bincount(first.cpu(), minlength=n_code)), "counts must accumulate"
    b.assert_untouched()


def test_vq_assign_non_unit_codebook_uses_the_code_norms():
    z, code, ref = make_case(200, 257, 32, "norms")
    by_angle = torch.argmax(ref["zn"] @ unit_rows(code.double()).t(), dim=1)
    assert int((by_angle != ref["index"]).sum()) >= 50, "the case must separate the two rules"
    b = VqBuffers(z, code, "cuda")
    check_indices(b.run(), ref, "non-unit codebook")
    b.assert_untouched()


@pytest.mark.parametrize("i,j", [(5, 100), (40, 41), (100, 300), (127, 128), (3, 999)])
def test_vq_assign_equal_rows_go_to_the_lower_index(i, j):
    """code[j] = code[i], and z rows built around that code so that it is their nearest by far: i inside the chunk of 128, in another
    wave's 32, in another chunk."""
    z, code, _ = make_case(200, 1000, 32)
    code = code.clone()
    code[j] = code[i]
    z = z.clone()
    g = torch.Generator().manual_seed(i * 1000 + j)
    z[:64] = code[i] * 3.0 + 0.05 * torch.randn(64, 32, generator=g)
    ref = vq_ref64(z, code)
    # the twins tie exactly, so the rule between them is the tie rule; every other comparison keeps the fp64 rule with column j set aside
    d = ref["d"].clone()
    d[:, j] = float("inf")
    ref_wo = dict(ref, d=d, index=torch.argmin(d, dim=1), gap=torch.topk(d, 2, dim=1, largest=False).values.diff(dim=1)[:, 0])
    assert bool((ref_wo["index"][:64] == i).all()) and bool((ref_wo["gap"][:64] > 0.1).all())
    b = VqBuffers(z, code, "cuda")
    got = b.run().cpu()
    assert got[:64].tolist() == [i] * 64
    assert bool((got != j).all()), "the higher twin was returned"
    check_indices(got, ref_wo, f"twins {i} {j}")
    b.assert_untouched()


def test_vq_assign_zero_nan_and_inf_rows():
    z, code, _ = make_case(200, 257, 32, "norms")
    z = z.clone()
    z[7] = 0.0
    z[64] = 0.0
    z[9, 3] = float("nan")
    z[130] = float("nan")
    z[11, 0] = float("inf")
    smallest = int(code.double().norm(dim=1).argmin())
    b = VqBuffers(z, code, "cuda", counts=True)
    got = b.run().cpu()
    assert int(got[7]) == smallest and int(got[64]) == smallest
    assert int(got.min()) >= 0 and int(got.max()) < 257
    keep = torch.ones(200, dtype=torch.bool)
    keep[[9, 130, 11]] = False
    ref = vq_ref64(z[keep], code)
    check_indices(got[keep], ref, "the finite rows beside them")
    assert torch.equal(b.counts.cpu().long(), torch.bincount(got, minlength=257))
    b.assert_untouched()


def test_vq_assign_same_bits_under_xfm_deterministic():
    env = dict(os.environ, XFM_DETERMINISTIC="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "vq_util.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    child = [line for line in r.stdout.splitlines() if line.startswith("VQ ")][-1].split()[1]
    saved = os.environ.pop("XFM_DETERMINISTIC", None)
    try:
        own = vq_digest()
    finally:
        if saved is not None:
            os.environ["XFM_DETERMINISTIC"] = saved
    assert child == own
