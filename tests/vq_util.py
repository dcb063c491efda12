"""fp64 restatement, derived error bound and the cases of the nearest-code kernel xfm_vq_assign (tests/test_vq_host.py, tests/test_hip_vq.py).

The definition (models/norm_ema_quantizer.py:153-162), in fp64 from the fp32 inputs:
    zn = z / max(|z|, 1e-12),   d[r, c] = |zn|^2 + |e_c|^2 - 2 zn . e_c,   index[r] = the first c at which d[r, .] is smallest.

The bound on the kernel's error in d -- derived, not fitted.  u = 2^-24 is the unit roundoff of fp32, K the feature width.
  * |z|^2 is a sum of K non-negative terms; however the kernel orders it, a term passes through at most K roundings: relative error
    <= K u.  The square root halves that and rounds once, the division rounds once: every component of the kernel's zn carries a relative
    error <= (K / 2 + 2) u, and so does its contribution to the dot product: <= (K / 2 + 2) u sum_k |zn_k e_k| <= (K / 2 + 2) u |zn| |e|
    (Cauchy-Schwarz).
  * The dot product is K exact products summed with one rounding each (an fmaf chain, which is what the f32 MFMA is): <= K u |zn| |e|.
  * |e|^2, the same kind of sum: <= K u |e|^2.
  * Joining the two, s = fmaf(-2, dot, |e|^2), rounds once: <= u (2 |zn| |e| + |e|^2).
  * |zn|^2 is the same number for every code of a row; the kernel leaves it out, which moves no comparison.
  Together (second-order terms are covered by rounding K / 2 + 2 up to K / 2 + 3):
      |d_kernel - d| <= u ((3 K + 8) |zn| |e| + (K + 1) |e|^2)  <=  (1.5 K + 4) u (2 |zn| |e| + |e|^2)  =: bound[r, c].
  This is the issue's "(K + 8) 2^-24 (2 |zn||e| + |e|^2 + |zn|^2)" with the constant worked out: at K = 32 and unit norms 9.3e-6 here
  against 9.5e-6 there.

If the kernel prefers c' to the fp64 winner c*, its own scores say s(c') <= s(c*), so d(c') - d(c*) <= bound(c') + bound(c*) <= 2 B_r with
B_r = max_c bound[r, c].  Hence the rule of the tests: a row whose fp64 top-2 gap exceeds 2 B_r is DECIDED, the index must be equal; on the
others the kernel may return any code whose fp64 d is within B_r of the minimum.  make_case asserts, on the fp64 side, that at most 1 % of
a case's rows are undecided (with Gaussian rows against random unit codes the smallest gap seen at these sizes is about 2e-5: none are).
"""
import functools
import hashlib

import numpy as np
import torch

U = 2.0 ** -24
UNDECIDED_CAP = 0.01
IDX_FILL, RIM = -7777, -123456   # the index parent is poisoned; counts accumulate, so their view starts at zero inside a poisoned rim


def kernel_bound(K, zn_norm, e_norm):
    """bound[r, c] of the header, fp64 [M, n_code]."""
    zn, e = zn_norm[:, None], e_norm[None, :]
    return (1.5 * K + 4) * U * (2.0 * zn * e + e * e)


def vq_ref64(z, code):
    """The fp64 restatement on fp32 inputs -> dict(index [M], gap [M] = second smallest d - smallest, d [M, n], B [M] = max_c bound)."""
    assert z.dtype == torch.float32 and code.dtype == torch.float32
    Z, E = z.double(), code.double()
    zn = Z / Z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    d = zn.pow(2).sum(1, keepdim=True) + E.pow(2).sum(1) - 2.0 * zn @ E.t()
    index = torch.argmin(d, dim=1)
    if code.shape[0] > 1:
        two = torch.topk(d, 2, dim=1, largest=False).values
        gap = two[:, 1] - two[:, 0]
    else:
        gap = torch.full((z.shape[0],), float("inf"), dtype=torch.float64)
    B = kernel_bound(z.shape[1], zn.norm(dim=1), E.norm(dim=1)).max(dim=1).values
    return dict(index=index, gap=gap, d=d, B=B, zn=zn)


def check_indices(got, ref, what=""):
    """The rule of the header; returns the number of undecided rows."""
    got = got.cpu().long()
    n = ref["d"].shape[1]
    assert got.shape == ref["index"].shape and int(got.min()) >= 0 and int(got.max()) < n, what
    undecided = ref["gap"] <= 2.0 * ref["B"]
    wrong = (got != ref["index"]) & ~undecided
    assert not bool(wrong.any()), (what, "decided rows with another index", wrong.nonzero().flatten()[:8].tolist())
    dmin = ref["d"].min(dim=1).values
    dgot = ref["d"].gather(1, got[:, None])[:, 0]
    loose = undecided & ~(dgot - dmin <= ref["B"])
    assert not bool(loose.any()), (what, "undecided rows past the bound", loose.nonzero().flatten()[:8].tolist())
    return int(undecided.sum())


def unit_rows(t):
    return t / t.norm(dim=1, keepdim=True)


@functools.lru_cache(maxsize=None)
def make_case(M, n_code, K, kind="unit"):
    """z [M, K] Gaussian rows at mixed scales, code [n_code, K]: 'unit' = random unit rows, 'norms' = row norms spread over [0.5, 2].
    Returns (z, code, ref); asserts the cap on undecided rows."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * n_code + 17 * K + (5 if kind == "norms" else 0))
    z = torch.randn(M, K, generator=g) * (0.25 + 4.0 * torch.rand(M, 1, generator=g))
    code = unit_rows(torch.randn(n_code, K, generator=g).double()).float()
    if kind == "norms":
        code = code * (0.5 + 1.5 * torch.rand(n_code, 1, generator=g))
    ref = vq_ref64(z, code)
    undecided = int((ref["gap"] <= 2.0 * ref["B"]).sum())
    assert undecided <= UNDECIDED_CAP * M, (M, n_code, K, kind, undecided)
    return z, code, ref


GRID = [(M, n) for M in (1, 63, 65, 200) for n in (1, 33, 257, 1000)]
WIDTHS = [(200, 257, 8), (200, 257, 64)]


class VqBuffers:
    """Every operand of one call as a strided slice of a poisoned parent, on `device`: z and code inside NaN parents (rows on 16 bytes: column
    offsets and leading dimensions multiples of 4), the indices inside an int64 parent of IDX_FILL, the counts inside an int32 parent whose
    rim is RIM."""

    def __init__(self, z, code, device, counts=False):
        from gemm_strided_util import NAN, embed, embed_vec
        M, K = z.shape
        n = code.shape[0]
        self.z, self.z_parent = embed(z.to(device), K + 12, 4, 1, 2, NAN)
        self.code, self.code_parent = embed(code.to(device), K + 8, 8, 2, 1, NAN)
        self.index, self.index_parent = embed_vec(torch.full((M,), IDX_FILL, dtype=torch.int64, device=device), 3, 5, IDX_FILL)
        self.counts = self.counts_parent = None
        if counts:
            self.counts, self.counts_parent = embed_vec(torch.zeros(n, dtype=torch.int32, device=device), 5, 3, RIM)
        self.z0, self.code0 = self.z_parent.clone(), self.code_parent.clone()

    def run(self):
        from xfm_amd import functional as Fx
        out = Fx.vq_assign(self.z, self.code, counts=self.counts, out=self.index)
        assert out.data_ptr() == self.index.data_ptr()
        return out

    def assert_untouched(self):
        M = self.index.shape[0]
        assert torch.equal(self.z_parent.view(torch.int32), self.z0.view(torch.int32)), "z or its parent was written"
        assert torch.equal(self.code_parent.view(torch.int32), self.code0.view(torch.int32)), "code or its parent was written"
        p = self.index_parent.cpu()
        assert bool((p[:3] == IDX_FILL).all()) and bool((p[3 + M:] == IDX_FILL).all()), "indices written outside their view"
        if self.counts_parent is not None:
            c = self.counts_parent.cpu()
            assert bool((c[:5] == RIM).all()) and bool((c[-3:] == RIM).all()), "counts written outside their view"


# ------------------------------------------------------------------------------------------------------------ the vqkd_small fixture
def vqkd_state(spec):
    """The tokenizer weights of tests/golden/vqkd_small.npz from their spec (what tools/oracle/gen_vqkd.py saved to the checkpoint the
    reference loaded): formula values, the codebook rows l2-normalised in fp32 afterwards, `initted` set (a trained codebook)."""
    from golden_util import state_from_spec
    sd = state_from_spec(spec)
    w = sd["quantize.embedding.weight"].float()
    sd["quantize.embedding.weight"] = w / w.norm(dim=1, keepdim=True)
    sd["quantize.embedding.initted"] = torch.ones(1)
    return sd


def vqkd_images(meta):
    """The B images of the tokenizer part of the fixture, in [0, 1): the 'default' pre_process takes its x 255 branch."""
    from xfm_amd import synthetic as syn
    B, R = meta["B"], meta["image_res"]
    return torch.from_numpy(syn.uniform01("vqkd.image", B * 3 * R * R, meta["image_seed"]).astype(np.float32).reshape(B, 3, R, R))


def unit64(feat):
    f = feat.double()
    return f / f.norm(dim=1, keepdim=True).clamp_min(1e-12)


def decided_patches(feat_ref, code, delta_norm):
    """fp64 argmin of the reference features [M, K] and which patches are DECIDED against an error of norm `delta_norm` [M] in the
    NORMALISED features (|unit64(other) - unit64(feat_ref)|).  Moving zn by e moves d[., c] = |zn|^2 + |e_c|^2 - 2 zn . e_c by -2 e . e_c
    around a term common to all codes, so two codes move apart by at most 4 |e| max|e_c|: the reference's choice survives when its top-2
    gap exceeds 4 |delta| max|e_c| plus the fp32 bound of the kernel (twice B_r, the header's decided rule)."""
    ref = vq_ref64(feat_ref, code)
    emax = float(code.double().norm(dim=1).max())
    return ref, ref["gap"] > 4.0 * delta_norm.double() * emax + 2.0 * ref["B"]


def vq_digest(device="cuda"):
    """sha1 of the indices and counts of the case (200, 1000, 32): what the XFM_DETERMINISTIC child prints and the parent compares."""
    z, code, _ = make_case(200, 1000, 32)
    b = VqBuffers(z, code, device, counts=True)
    idx = b.run().cpu().numpy()
    cnt = b.counts.cpu().numpy()
    return hashlib.sha1(np.ascontiguousarray(idx).tobytes() + np.ascontiguousarray(cnt).tobytes()).hexdigest()


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("VQ " + vq_digest())
