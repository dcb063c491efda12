"""The one-round 320 x 256 tile (tile_hint 6) against the automatic plan (tile_hint 0: a round of 256 x 256 tiles + the small-tile tail)
on the ViT trunk's three N = 768 shapes, isolated, on cold operands rotated through a ring of buffers as tools/bench_nt256.py does.
The two hints alternate REPS times on one GPU; printed per shape: the median and the spread (min .. max) of each, and the difference.

    python tools/bench_nt320.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from xfm_amd import functional as Fx  # noqa: E402

SHAPES = [(25216, 768, 3072, 0), (25216, 768, 768, 0), (25216, 768, 2304, 0)]
REPS, ITERS = 7, 20


def timeit(fn, iters=ITERS):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    for M, N, K, epi in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(M + N + K + epi)
        nbuf = max(2, int(1.2e9 / ((M * K + N * K + 2 * M * N) * 2)))
        As = [torch.randn(M, K, device="cuda", generator=g).bfloat16() for _ in range(nbuf)]
        Bs = [(torch.randn(N, K, device="cuda", generator=g) * 0.05).bfloat16() for _ in range(nbuf)]
        bias = torch.randn(N, device="cuda", generator=g) * 0.1
        Os = [torch.empty(M, N, device="cuda", dtype=torch.bfloat16) for _ in range(nbuf)]
        cnt = [0]

        def run(hint):
            i = cnt[0] % nbuf
            cnt[0] += 1
            Fx.gemm_nt(As[i], Bs[i], out=Os[i], bias=bias, epi=epi, tile_hint=hint)
        t = {0: [], 6: []}
        for _ in range(REPS):
            for hint in (0, 6):
                t[hint].append(timeit(lambda: run(hint)))
        run(0)
        ref = Os[(cnt[0] - 1) % nbuf].clone()
        cnt[0] -= 1
        run(6)
        same = torch.equal(ref, Os[(cnt[0] - 1) % nbuf])
        m0, m6 = statistics.median(t[0]), statistics.median(t[6])
        print(f"{M:6d} {N:5d} {K:5d} | hint 0 {m0:6.1f} us ({min(t[0]):.1f} .. {max(t[0]):.1f}) | hint 6 {m6:6.1f} us ({min(t[6]):.1f} .. {max(t[6]):.1f}) | "
              f"{m0 - m6:+5.1f} us | {2.0 * M * N * K / m6 / 1e6:4.0f} TF | bit-identical {same}", flush=True)
        del As, Bs, Os


if __name__ == "__main__":
    main()
