"""The one-round 320 x 256 GEMM tile (csrc/nt320_gemm.hip, xfm_gemm_nt tile_hint 6) without a GPU: the register budget of its five
builds from the gfx950 compile, and its place in the launch plan, asked of the library alone."""
import json
import os
import re
import subprocess
import sys


def test_nt320_kernel_builds_once_per_epilogue_inside_its_register_budget():
    """Two waves per SIMD inside a counted-vmcnt pipeline: <= 256 registers, nothing spilled (scratch traffic is VMEM traffic that the
    wait counts do not know about), and the LDS ring is dynamic (144 KiB, under the 160 KiB of a CU)."""
    from xfm_amd import build
    use = {n: u for n, u in build.resource_usage().items() if "gemm_nt_320_kernel" in n}
    assert sorted(use) == ["_Z18gemm_nt_320_kernelILi%dEEv6GemmNT" % e for e in range(5)], sorted(use)
    for name, u in use.items():
        assert u["vgprs"] + u.get("agprs", 0) <= 256, (name, u)
        assert u["spill"] == 0 and u["scratch"] == 0, (name, u)
        assert u["lds"] == 0, (name, u)   # no static LDS beside the ring
    src = open(os.path.join(os.path.dirname(build.__file__), "csrc", "nt320_gemm.hip")).read()
    units = int(re.search(r"NT320_LDS = (\d+) \* NT320_UNIT", src).group(1))
    assert units * 64 * 128 <= 160 * 1024, units


# ((M, N, K, epilogue, tile_hint), cfg, rows_a); without a device the CU count reads 256
PLAN_TABLE = [
    ((25216, 768, 768, 0, 6), 6, 0), ((25216, 768, 768, 0, 0), 5, 21760),
    ((25216, 768, 3072, 0, 6), 6, 0), ((25216, 768, 2304, 0, 6), 6, 0), ((25216, 768, 3072, 3, 6), 6, 0),
    ((320, 256, 64, 0, 6), 6, 0), ((321, 768, 128, 4, 6), 6, 0),
    ((27200, 768, 768, 0, 6), 6, 0),            # 85 x 3 = 255 tiles: one round
    ((27521, 768, 768, 0, 6), 5, 21760),        # 87 x 3 = 261 tiles: more than one round, planned as hint 0 (the tail split)
    ((1000, 520, 64, 0, 6), 3, 0),              # N % 256 != 0
    ((25216, 3072, 768, 2, 6), 5, 0),           # 79 x 12 tiles
]


def _plans(rows, env=None):
    from xfm_amd import build
    child = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I, P = ctypes.c_int, ctypes.c_void_p
lib.xfm_gemm_nt_plan.argtypes = [I] * 5 + [P] * 2
c, r, out = I(), I(), []
for a in json.load(sys.stdin):
    assert lib.xfm_gemm_nt_plan(*a, ctypes.addressof(c), ctypes.addressof(r)) == 0
    out.append([c.value, r.value])
print(json.dumps(out))
"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("XFM_")}
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", child, build.build()], input=json.dumps(rows), env=e, capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


def test_nt320_plan_is_reached_by_hint_6_alone_and_only_where_it_fits():
    """Fresh processes that load the library alone (no GPU, no torch, no XFM_* knobs)."""
    args = [a for a, _, _ in PLAN_TABLE]
    got = _plans(args)
    assert got == [[c, ra] for _, c, ra in PLAN_TABLE], list(zip(args, got))
    # an ineligible call with hint 6 is the call with hint 0, and so is every call under XFM_GEMM_NT320=0
    as0 = _plans([a[:4] + (0,) for a in args])
    assert [g for g, (_, c, _) in zip(got, PLAN_TABLE) if c != 6] == [g for g, (_, c, _) in zip(as0, PLAN_TABLE) if c != 6]
    assert _plans(args, {"XFM_GEMM_NT320": "0"}) == as0
