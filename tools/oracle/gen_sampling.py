"""Generate tests/golden/sampling_filter.npz from the REAL reference's top_k_top_p_filtering (behind ref_shim, as gen_generation.py does).

Run in the build container only:   python tools/oracle/gen_sampling.py

The sampling branch of BertLMHeadModel._generate_no_beam_search (models/xbert.py:1434-1441) divides the last-position logits by the
temperature and hands them to top_k_top_p_filtering (:1487-1519); this generator does exactly that, in fp32, on formula rows.

Inputs are formulas, never stored: case i is syn.gaussian(f"sampling.logits.{i}", (ROWS, 50265), scale) -- the meta lists name, scale and
the (top_k, top_p, temperature) of every case.  Stored per case: kept/<i> = np.packbits of the reference's kept mask (filtered > -inf),
[ROWS, ceil(V / 8)] uint8, and count/<i> = the kept counts [ROWS].  Nothing else.

Scale 8 gives nuclei of 1 to a dozen tokens with wide gaps; the generator asserts that every top-p row of a case not marked flat is
DECISIVE: no c64[i - 1] (the fp64 running softmax over the sorted row, which the reference computes in fp32) within 1e-4 of top_p, so
the kept set does not depend on the summation's rounding.  Scale 1 is flat (about 20 positions inside that band): one such case is kept,
marked flat, for the band rule of the tests (the reference's count must lie in [n_lo, n_hi])."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402  (puts the repository root on sys.path)
import ref_shim  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

V, ROWS, DELTA = 50265, 3, 1e-4
# (top_k, top_p, temperature, scale, flat)
CASES = ((50, 0.9, 0.7, 8.0, False), (0, 0.9, 1.0, 8.0, False), (0, 0.5, 1.0, 8.0, False), (5, 1.0, 1.0, 8.0, False),
         (20, 0.95, 2.5, 8.0, False), (0, 0.9, 1.0, 1.0, True))


def band(z, top_k, top_p):
    """Smallest |c64[i - 1] - top_p| over the positions of one fp32 row after top-k (fp64 running softmax, descending order)."""
    z = z.double()
    if top_k > 0:
        z = z[z >= torch.topk(z, min(max(top_k, 1), z.numel())).values[-1]]
    c = torch.cumsum(torch.softmax(torch.sort(z, descending=True).values, 0), 0)
    return float((c[:-1] - float(torch.tensor(top_p, dtype=torch.float32))).abs().min()) if c.numel() > 1 else 1.0


def main():
    torch.set_num_threads(int(os.environ.get("GEN_THREADS", "8")))
    ref_shim.install()
    from models.xbert import top_k_top_p_filtering
    out, cases = {}, []
    for i, (top_k, top_p, temperature, scale, flat) in enumerate(CASES):
        name = f"sampling.logits.{i}"
        logits = syn.gaussian(name, (ROWS, V), scale)
        z = logits / temperature if temperature != 1.0 else logits.clone()   # :1436-1437
        kept = top_k_top_p_filtering(z.clone(), top_k=top_k, top_p=top_p) > -float("inf")
        gaps = [band(z[r], top_k, top_p) for r in range(ROWS)] if top_p < 1.0 else [1.0] * ROWS
        if not flat:
            assert min(gaps) > DELTA, (i, gaps)
        out[f"kept/{i}"] = np.packbits(kept.numpy(), axis=1)
        out[f"count/{i}"] = kept.sum(1).numpy().astype(np.int64)
        cases.append({"name": name, "scale": scale, "top_k": top_k, "top_p": top_p, "temperature": temperature, "flat": flat})
        print(f"case {i}: k={top_k} p={top_p} T={temperature} scale={scale} flat={flat}: kept {out[f'count/{i}'].tolist()}, "
              f"smallest |c64 - top_p| {min(gaps):.2e}", flush=True)
    G.save("sampling_filter", out, {"V": V, "rows": ROWS, "delta": DELTA, "cases": cases})


if __name__ == "__main__":
    main()
