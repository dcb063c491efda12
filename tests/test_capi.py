"""CPU-side checks of the C-ABI boundary: the library builds for gfx950, loads, and exports exactly the symbols that
include/xfm_hip.h declares; the ctypes binding mirrors the header; the product path refuses to run without the HIP
extension or on CPU tensors (no silent fallback)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xfm_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(xfm_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    from xfm_amd import build
    lib_path = build.build()
    assert os.path.exists(lib_path)
    lib = ctypes.CDLL(lib_path)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/xfm_hip.h but not exported"


def test_binding_covers_the_header_and_abi_version():
    from xfm_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    hdr = open(HEADER).read()
    assert f"#define XFM_ABI_VERSION {_lib.ABI_VERSION}" in hdr


def test_struct_layouts_match_header_field_order():
    from xfm_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, struct in (("xfm_ln_fwd_args", _lib.LnFwdArgs), ("xfm_ln_bwd_args", _lib.LnBwdArgs),
                          ("xfm_attn_args", _lib.AttnArgs), ("xfm_embed_args", _lib.EmbedArgs), ("xfm_adamw_args", _lib.AdamWArgs)):
        end = hdr.index("} " + cname + ";")
        body = hdr[hdr.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                name = re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?\s*$", part.strip())
                fields.append(name[0])
        assert fields == [f[0] for f in struct._fields_], cname


def test_argument_errors_are_reported_not_crashed():
    from xfm_amd import _lib
    lib = _lib.load()
    rc = lib.xfm_gemm_nt(None, 0, None, 0, None, 0, None, None, 0, 1, 1, 64, 0, 0, None)
    assert rc == -1 and b"null operand" in lib.xfm_last_error()
    rc = lib.xfm_layernorm_fwd(None, 768, 0, None)
    assert rc == -1


def test_rccl_entry_points_report_argument_errors():
    """xfm_dp_*: no communicator -> an error code and a message, never a crash (XFM_E_ARG; XFM_E_UNSUPPORTED where librccl.so cannot be
    loaded -- the library itself must load without it: it is resolved at the first xfm_dp_* call, not at link time)."""
    from xfm_amd import _lib
    lib = _lib.load()
    rc = lib.xfm_dp_bucket_allreduce(None, None, 16, 0, 1, None)
    assert rc in (-1, -3) and lib.xfm_last_error()
    rc = lib.xfm_dp_init(None, 0, 1, None)
    assert rc in (-1, -3)
    import subprocess
    needed = subprocess.run(["readelf", "-d", _lib.LIB_PATH if hasattr(_lib, "LIB_PATH") else os.path.join(ROOT, "xfm_amd", "libxfm_hip.so")],
                            capture_output=True, text=True).stdout
    assert "rccl" not in needed   # no link-time dependency on RCCL


def test_product_path_refuses_cpu_tensors():
    from xfm_amd import _lib, functional as Fx
    a = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.XfmHipError):
        Fx.gemm_nt(a, a)


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "xfm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("tools/oracle", ""), f"{f} references the oracle"


def test_register_bound_kernels_keep_their_budgets():
    """The 256 x 256 GEMM kernels run two waves per SIMD (<= 256 VGPRs) inside counted-vmcnt pipelines, the short-sequence attention
    backward kernels three (<= 168): a compiler or source change that spills them to scratch (VMEM traffic the wait counts do not
    know about) or drops their occupancy must fail here, not show up as a slow bench.  The shipped ViT forward kernel sits at its
    256-register limit with two spilled registers outside its loops; more than that is a regression."""
    from xfm_amd import build
    use = build.resource_usage()
    seen = []
    for name, u in use.items():
        if "gemm_nt_256_kernel" in name or "gemm_tn_256_kernel" in name:
            seen.append(name)
            assert u["vgprs"] + u.get("agprs", 0) <= 256, (name, u)
            assert u["spill"] == 0 and u["scratch"] == 0, (name, u)
        if "attn_bwd_dq_short_kernel" in name or "attn_bwd_dkv_short_kernel" in name:
            seen.append(name)
            assert u["vgprs"] <= 168 and u["spill"] == 0 and u["scratch"] == 0, (name, u)
        if "gemm_tn_group_kernel" in name:   # the grouped weight-gradient kernel: one build (a throttled second one spilled 5 registers)
            seen.append(name)
            assert u["vgprs"] <= 256 and u["spill"] == 0 and u["scratch"] == 0, (name, u)
        if "attn_fwd_vit_kernelILb1ELi13ELb1E" in name:   # <bias, 13 tiles, tiled bias>: the pre-training step's instantiation
            seen.append(name)
            assert u["scratch"] <= 16, (name, u)
    # exactly these: an experiment's second build of one of them (another look-ahead, a stamped or throttled variant) does not ship
    want = ["_Z18gemm_nt_256_kernelILi%dELb%dEEv6GemmNTi" % (e, p) for e in range(5) for p in (0, 1)]      # <EPI, PERSIST>
    want += ["_Z18gemm_tn_256_kernel6GemmTN", "_Z20gemm_tn_group_kernel7TnGroup"]
    want += ["_Z24attn_bwd_dq_short_kernelILi3ELi%dELb%dEEv13xfm_attn_argsii" % (n, p) for n in (4, 7, 8) for p in (0, 1)]   # <3, NP, PRE>
    want += ["_Z25attn_bwd_dkv_short_kernelILi%dEEv13xfm_attn_argsii" % n for n in (4, 7)]
    want += ["_Z19attn_fwd_vit_kernelILb1ELi13ELb1EEv13xfm_attn_args6VitMap"]
    assert len(want) == 21 and sorted(seen) == sorted(want), sorted(set(seen) ^ set(want))


def test_persistent_gemm_epilogue_issues_the_stores_its_wait_counts_assume():
    """gemm_nt_256_kernel<EPI, PERSIST> retires the next tile's first staging units with `s_waitcnt vmcnt(6 + NS)`: the 2 D
    staging loads are OLDER than the NS output stores of an interior tile, so the wait is only sufficient if the compiler really
    issues >= NS store instructions per lane on that path (fewer -- merged or dropped stores -- and a wave would read a ring slot
    whose direct-to-LDS load has not landed; more are harmless, the wait only gets stricter).  Pinned here from the gfx950 ISA:
    the full-width path of every instantiation holds exactly NS `global_store_dwordx4` (16: bf16 / GELU-dgrad; 32: fp32 and
    GELU + gelu'), the ragged-edge path stores element-wise with narrower instructions."""
    import re
    from xfm_amd import build
    isa = build.kernel_isa()
    want = {0: 16, 1: 32, 2: 32, 3: 16}   # EPI_BF16, EPI_F32, EPI_GELU, EPI_DGELU (EPI_F32_ACC waits without the allowance)
    seen = 0
    for name, body in isa.items():
        m = re.match(r"_Z18gemm_nt_256_kernelILi(\d)ELb([01])EEv", name)
        if not m or int(m.group(1)) not in want:
            continue
        seen += 1
        x4 = sum(1 for l in body if l.startswith("global_store_dwordx4"))
        assert x4 == want[int(m.group(1))], (name, x4)
        if m.group(2) == "1":   # the allowance itself: vmcnt(6 + NS) is in the persistent instantiation's code
            assert any(re.search(r"s_waitcnt vmcnt\(%d\)" % (6 + want[int(m.group(1))]), l) for l in body), name
    assert seen == 8, seen   # 4 epilogues x {one workgroup per tile, persistent}



def test_default_library_carries_no_diagnostic_entry_point_and_the_diagnostic_build_compiles():
    """The timeline stamps of tools/tile_timeline.py / attn_timeline.py and their setter compile under -DXFM_DIAG only
    (`python -m xfm_amd.build --diag`): the default library has no xfm_diag_* symbol, and the diagnostic code still compiles for gfx950."""
    from xfm_amd import build
    with open(build.build(), "rb") as f:
        assert b"xfm_diag_" not in f.read()
    assert not any("xfm_diag_" in n for n in _declared())
    remarks, asm = build._device_compile(diag=True)
    stamped = [n for n in re.findall(r"^(_Z\w+):", asm, flags=re.M) if "attn_bwd_dq_short_kernel" in n and n.endswith("Px")]
    assert len(stamped) == 8, stamped   # <3, NP, PRE, false> x 6 + the two stamped <3, 7, PRE, true>: the timeline argument exists here


RETIRED_KNOBS = ["XFM_GEMM_SKEW_US", "XFM_GEMM_NT_D", "XFM_GEMM_KROT", "XFM_GEMM_EXP_CFG", "XFM_KSPLIT_FORCE", "XFM_KSPLIT_TILE",
                 "XFM_TN_SYNC_WINDOW", "XFM_RL_SKIP_WGRAD", "XFM_TN_BATCH", "XFM_GEMM_DBG_PTR", "XFM_ATTN_DBG_PTR"]


def _text_files(*dirs):
    for d in dirs:
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith((".hip", ".h", ".py", ".sh", ".md")):
                    path = os.path.join(base, f)
                    yield os.path.relpath(path, ROOT), open(path, errors="replace").read()


def test_environment_knobs_have_one_reader_and_a_documented_name():
    """The library reads its environment through xfm_env_int / xfm_env_flag (csrc/common.h) and nowhere else; the experiment paths
    retired from it are not selectable any more from the library or the tools; every knob the library still reads has a row in
    tools/README.md."""
    csrc = dict(_text_files(os.path.join("xfm_amd", "csrc")))
    assert len(csrc) >= 11
    assert [p for p, s in csrc.items() if "getenv" in s] == [os.path.join("xfm_amd", "csrc", "common.h")]
    for path, s in _text_files("xfm_amd", "tools"):
        for name in RETIRED_KNOBS:
            assert not re.search(name + r"(?![A-Z0-9_])", s), (path, name)
    read = set()
    for s in csrc.values():
        read |= set(re.findall(r"xfm_env_(?:int|flag)\(\"(XFM_[A-Z0-9_]+)\"", s))
        assert not re.search(r"xfm_env_(?:int|flag)\((?!\"XFM_[A-Z0-9_]+\"|const char|name,)", s)   # a literal name at every call outside common.h's own two
    assert {"XFM_DETERMINISTIC", "XFM_ATTN_SHORT_PRE", "XFM_GEMM_PERSIST", "XFM_LN_BWD_ROWS"} <= read, sorted(read)
    table = open(os.path.join(ROOT, "tools", "README.md")).read()
    documented = set(re.findall(r"XFM_[A-Z0-9_]+", table))
    assert read <= documented, sorted(read - documented)


ATTENTION_SOURCES = ("attention.hip", "attention_common.h", "attention_general.hip", "attention_short.hip", "attention_grouped.hip",
                     "attention_vit.hip", "attention_long.hip", "attention_aux.hip")


def _attn_ws_args(B, H, Sq, Sk, ld=None, dbias=True, mask=False, phase=0, single_pass=False):
    """xfm_attn_args of a dense backward call with an additive bias (rows padded to a multiple of 16 keys unless `ld` says otherwise)
    and dummy non-NULL, 16-byte aligned pointers: xfm_attn_bwd_workspace is host-only and dereferences none of them."""
    from xfm_amd import _lib
    a = _lib.AttnArgs()
    P = 0x10000
    for f in ("q", "k", "v", "o", "lse", "bias", "dout", "dq", "dk", "dv", "delta", "bias_t", "o_lo", "bias_tiled", "bias_t_tiled"):
        setattr(a, f, P)
    for f in ("q_rs", "k_rs", "v_rs", "o_rs", "do_rs", "dq_rs", "dk_rs", "dv_rs"):
        setattr(a, f, 64 * H)
    a.B, a.H, a.Sq, a.Sk, a.scale, a.bwd_phase = B, H, Sq, Sk, 0.125, phase
    a.bias_ld = ld if ld is not None else (Sk + 15) // 16 * 16
    a.bias_t_ld = a.stat_ld = (Sq + 15) // 16 * 16
    a.dbias = P if dbias else None
    a.key_keep = P if mask else None
    if single_pass:   # what the opt-in single-pass ViT backward wants: the forward's O without its low half
        a.o_lo = None
    return a


# (arguments of _attn_ws_args, environment, bytes).  The values are those of the library BEFORE the backward plan existed (two
# derivations of the route, one in the dispatcher and one here), recorded from it; the two rows marked "discarded" are the exception:
# there it asked for a buffer that its own dispatcher then dropped, and the plan asks for none.
ATTN_WORKSPACE_TABLE = [
    (dict(B=9, H=12, Sq=197, Sk=197), {}, 0),                                                 # short pair, atomics
    (dict(B=9, H=12, Sq=197, Sk=197), {"XFM_DETERMINISTIC": "1"}, 5900544),                   # ... 3 slices x [12, 197, 208] planes
    (dict(B=64, H=12, Sq=197, Sk=197), {"XFM_DETERMINISTIC": "1"}, 7867392),                  # 4 slices
    (dict(B=128, H=12, Sq=197, Sk=197), {"XFM_DETERMINISTIC": "1"}, 7867392),
    (dict(B=9, H=12, Sq=197, Sk=197, phase=2), {"XFM_DETERMINISTIC": "1"}, 0),                # dK/dV alone: no bias gradient
    (dict(B=9, H=12, Sq=197, Sk=197, phase=1), {"XFM_DETERMINISTIC": "1"}, 5900544),
    (dict(B=9, H=12, Sq=197, Sk=197, dbias=False), {"XFM_DETERMINISTIC": "1"}, 0),
    (dict(B=9, H=12, Sq=197, Sk=197, ld=224), {"XFM_DETERMINISTIC": "1"}, 0),                 # rows wider than the key tiles: atomics
    (dict(B=9, H=2, Sq=40, Sk=40), {"XFM_DETERMINISTIC": "1"}, 138240),                       # 9 slices x [2, 40, 48]
    (dict(B=9, H=2, Sq=40, Sk=40), {"XFM_DETERMINISTIC": "0"}, 0),
    (dict(B=3, H=12, Sq=30, Sk=30), {"XFM_DETERMINISTIC": "1"}, 138240),
    (dict(B=3, H=12, Sq=30, Sk=30), {}, 0),
    (dict(B=1, H=12, Sq=197, Sk=197), {"XFM_DETERMINISTIC": "1"}, 0),                         # one slice
    (dict(B=3, H=12, Sq=30, Sk=30, mask=True), {"XFM_DETERMINISTIC": "1"}, 0),                # masked, resident: atomics
    (dict(B=5, H=2, Sq=577, Sk=577), {}, 8198016),                                            # long: 3 slices x [2, 577, 592]
    (dict(B=5, H=2, Sq=577, Sk=577), {"XFM_DETERMINISTIC": "1"}, 8198016),
    (dict(B=5, H=2, Sq=577, Sk=577, dbias=False), {}, 0),
    (dict(B=5, H=2, Sq=577, Sk=577), {"XFM_ATTN_LONG": "0"}, 13663360),                       # general kernel: [5, 2, 577, 592] per entry
    (dict(B=5, H=2, Sq=577, Sk=577, mask=True), {}, 13663360),
    (dict(B=9, H=1, Sq=260, Sk=258), {}, 2545920),
    (dict(B=9, H=1, Sq=260, Sk=258), {"XFM_DETERMINISTIC": "1"}, 2545920),
    (dict(B=1, H=2, Sq=130, Sk=300), {}, 0),                                                  # long, one slice: adds in place
    (dict(B=1, H=2, Sq=130, Sk=300), {"XFM_DETERMINISTIC": "1"}, 0),
    (dict(B=1, H=2, Sq=130, Sk=300, mask=True), {}, 316160),
    (dict(B=1, H=2, Sq=130, Sk=300, mask=True), {"XFM_DETERMINISTIC": "1"}, 316160),
    (dict(B=1, H=2, Sq=130, Sk=300, mask=True, ld=384), {}, 0),                               # discarded (399360): rows past the key chunks
    (dict(B=3, H=2, Sq=197, Sk=197, single_pass=True), {"XFM_ATTN_VIT_BWD": "4"}, 983424),    # block kernel: 3 slices x [2, 197, 208]
    (dict(B=64, H=12, Sq=197, Sk=197, single_pass=True), {"XFM_ATTN_VIT_BWD": "4"}, 9834240),   # 5 slices
    (dict(B=9, H=12, Sq=197, Sk=197, single_pass=True), {"XFM_ATTN_VIT_BWD": "3", "XFM_DETERMINISTIC": "1"}, 0),   # discarded (5900544)
]


def test_attention_backward_workspace_table():
    """xfm_attn_bwd_workspace over a fixed table of argument sets.  One process per row: XFM_ATTN_LONG is read once per process, and a
    fresh process shows that the answer does not depend on an earlier call.  (The child loads the library alone: no GPU, no torch.)"""
    import subprocess
    import sys
    from xfm_amd import build
    child = ("import ctypes, sys\n"
             "f = ctypes.CDLL(sys.argv[1]).xfm_attn_bwd_workspace\n"
             "f.restype = ctypes.c_long\n"
             "for line in sys.stdin:\n"
             "    print(f(ctypes.c_char_p(bytes.fromhex(line.strip()))))\n")
    by_env = {}
    for i, (kw, env, _) in enumerate(ATTN_WORKSPACE_TABLE):
        by_env.setdefault(tuple(sorted(env.items())), []).append(i)
    got = {}
    for env, rows in by_env.items():
        e = {k: v for k, v in os.environ.items() if not k.startswith("XFM_")}
        e.update(dict(env))
        r = subprocess.run([sys.executable, "-c", child, build.build()], input="".join(bytes(_attn_ws_args(**ATTN_WORKSPACE_TABLE[i][0])).hex() + "\n" for i in rows),
                           env=e, capture_output=True, text=True, check=True)
        got.update(zip(rows, map(int, r.stdout.split())))
    assert [got[i] for i in range(len(ATTN_WORKSPACE_TABLE))] == [w for _, _, w in ATTN_WORKSPACE_TABLE], \
        [(kw, env, got[i], w) for i, (kw, env, w) in enumerate(ATTN_WORKSPACE_TABLE) if got[i] != w]


GEMM_SOURCES = ("gemm.hip", "gemm_common.h", "gemm_nt_small.hip", "gemm_nt_256.hip", "gemm_tn_small.hip", "gemm_tn_256.hip", "gemm_cast.hip")


def test_kernel_sources_set_the_lds_attribute_once_and_include_at_the_top():
    """One launcher (lds_launch, common.h) owns hipFuncAttributeMaxDynamicSharedMemorySize for every kernel instantiation of the library,
    no hand-kept `attr_set` guard is left, and attention.hip / gemm.hip (the host sides) pull in their kernel families before their first
    function: no file order to work around."""
    csrc = os.path.join(ROOT, "xfm_amd", "csrc")
    assert sorted(f for f in os.listdir(csrc) if f.startswith("attention")) == sorted(ATTENTION_SOURCES)
    assert sorted(f for f in os.listdir(csrc) if f.startswith("gemm")) == sorted(GEMM_SOURCES)
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h"))}
    assert sum(s.count("hipFuncSetAttribute") for s in text.values()) == 1
    assert not [f for f, s in text.items() if "attr_set" in s]
    for host in ("attention.hip", "gemm.hip"):
        lines = text[host].splitlines()
        first_fn = next(i for i, l in enumerate(lines) if re.match(r"^(static |int |long |template |__global__ |struct |enum )", l))
        includes = [i for i, l in enumerate(lines) if l.lstrip().startswith("#include")]
        assert includes and max(includes) < first_fn, (host, includes, first_fn)
        assert {l.split('"')[1] for l in lines if l.startswith('#include "')} >= {f for f in text if f.startswith(host[:-4] + "_")}, host


def test_every_kernel_file_is_included_from_capi_exactly_once():
    """The library is one translation unit: a csrc/*.hip that capi.hip does not reach through #include lines is dead code that the build
    never notices (and that is_stale() keeps rebuilding for), one reached twice defines its kernels twice.  Read from the include lines
    alone; the headers carry `#pragma once` and may be named by every file."""
    csrc = os.path.join(ROOT, "xfm_amd", "csrc")
    times = {}

    def walk(name):
        with open(os.path.join(csrc, name)) as f:
            lines = f.readlines()
        for line in lines:
            m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
            if m and m.group(1).endswith(".hip"):
                assert "/" not in m.group(1), (name, m.group(1))
                times[m.group(1)] = times.get(m.group(1), 0) + 1
                if times[m.group(1)] == 1:
                    walk(m.group(1))

    walk("capi.hip")
    assert times == {f: 1 for f in os.listdir(csrc) if f.endswith(".hip") and f != "capi.hip"}, times


# (query, arguments, bytes): the answers of the library BEFORE one plan served the query and the launch (the ladder of xfm_gemm_tn written
# twice, the batched hint twice, the K-slice rule twice), recorded from it.  Host-only calls; without a device the CU count reads 256.
GEMM_WORKSPACE_TABLE = [
    ("tn", (4096, 768, 1536), 37748736),            # 256 x 256 kernel: 18 tiles x 8 splits
    ("tn", (4032, 768, 1536), 28311552),            # under 4096 rows: 128 x 128 plan, 72 tiles x 6 splits
    ("tn", (4160, 768, 1536), 37748736),
    ("tn", (4096, 768, 1280), 27525120),            # 15 tiles of 256 x 256 < 18: 128 x 128 plan
    ("tn", (4096, 1536, 1536), 66060288),
    ("tn", (21624, 2304, 768), 63700992),           # ragged M: the 21568-row body's planes
    ("tn", (8250, 768, 1536), 61341696),            # ragged, body 8192 rows
    ("tn", (8190, 768, 1536), 28311552),            # ragged, body 8128 rows < 8192: one 128 x 128 call
    ("tn", (8250, 768, 1280), 27525120),            # ragged, 15 tiles
    ("tn", (21624, 2432, 768), 29884416),           # ragged, N % 256 != 0
    ("tn", (1920, 768, 768), 0),                    # 4 splits x 36 tiles = 9.4 MB < 16 MB: atomics
    ("tn", (3360, 768, 768), 0),                    # 7 x 36 x 64 KB = 16.5e6 bytes < 16 MiB
    ("tn", (3840, 768, 768), 18874368),             # 8 x 36 x 64 KB
    ("tn", (928, 768, 768), 0),                     # the two-split case, 4.7 MB
    ("tn", (928, 3072, 768), 18874368),             # ... with 144 tiles
    ("tn", (600, 3072, 768), 0),                    # one split
    ("tn", (4096, 1000, 768), 25165824),            # N % 128 != 0: 8 x 6 tiles
    ("tn", (5252, 3072, 768), 28311552),            # ragged under 8192 rows (the fusion tower)
    ("tn", (0, 768, 768), 0),
    ("batch", (1, 1920, 768, 768), 0),
    ("batch", (2, 1920, 768, 768), 28311552),
    ("batch", (4, 1920, 768, 768), 28311552),
    ("batch", (5, 1920, 768, 768), 0),              # more than TN_BATCH_MAX: single calls
    ("batch", (3, 5248, 768, 768), 28311552),
    ("batch", (2, 1920, 1000, 768), 0),             # N % 128 != 0: single calls
    ("batch", (2, 300, 768, 768), 23592960),
    ("group", (12608, [(768, 768)] * 4), 134742016),
    ("group", (12608, [(2304, 768), (768, 768), (3072, 768), (768, 3072)] * 3), 134742016),
    ("group", (12608, [(2304, 768), (1000, 768), (768, 3072)]), 134742016),     # one item the grouped kernel does not take
    ("group", (4096, [(768, 1536), (768, 1000)]), 37896192),                    # 18 cut tiles, and 25165824 for the single call
    ("group", (12608, [(768, 768)] * 50), 134742016),                           # 48 + 2 items: two launches
    ("group", (5252, [(3072, 768), (768, 3072)] * 26), 134742016),
    ("group", (1000, [(768, 768)] * 3), 0),                                     # under 1024 rows: single calls of 0 bytes
    ("group", (12608, [(768, 768)] * 26), 0),                                   # 234 tiles: a last round >= 90 % full runs whole
    ("group", (1024, [(768, 768)]), 4737024),                                   # 144 K-steps shared by 9 workgroups
    ("ksplit", (192, 768, 50304), 16515072),
    ("ksplit", (2624, 768, 50304), 0),
    ("ksplit", (192, 768, 8192), 4718592),
    ("ksplit", (192, 768, 8128), 0),                # K < 8192
    ("ksplit", (2048, 768, 50304), 0),              # 192 tiles of 64 x 128
    ("ksplit", (1984, 768, 50304), 12189696),       # 186 tiles
    ("ksplit", (64, 128, 16384), 524288),
]
# ((M, N, K, epilogue, tile_hint), cfg, rows_a) of xfm_gemm_nt_plan, recorded from the same library
GEMM_NT_PLAN_TABLE = [
    ((12608, 768, 768, 0, 0), 5, 0), ((25216, 768, 768, 0, 0), 5, 21760), ((25216, 3072, 768, 2, 0), 5, 0), ((5248, 1536, 768, 0, 0), 1, 0),
    ((2624, 768, 3072, 0, 0), 8, 0), ((192, 768, 50304, 4, 0), 7, 0), ((928, 768, 768, 0, 0), 3, 0), ((64, 64, 64, 0, 0), 3, 0),
    ((12608, 768, 768, 0, 4), 4, 0),
]
NO_LIMIT = 2 ** 63 - 1
# ((M, N, K, ldy, ldx, splits_hint, workspace bytes), kernel, splits, bytes used) of xfm_gemm_tn_plan (kernel 0 = 256 x 256, 1 = ring,
# 2 = register-staged), derived from that library's xfm_gemm_tn: what it launched with a workspace of that size
GEMM_TN_PLAN_TABLE = [
    ((4096, 768, 1536, 768, 1536, 0, NO_LIMIT), 0, 8, 37748736),
    ((4096, 768, 1536, 768, 1536, 0, 37748736), 0, 8, 37748736),
    ((4096, 768, 1536, 768, 1536, 0, 37748735), 1, 6, 28311552),      # a byte short: steps down to the 128 x 128 plan
    ((4096, 768, 1536, 768, 1536, 0, 28311552), 1, 6, 28311552),
    ((4096, 768, 1536, 768, 1536, 0, 28311551), 1, 6, 0),             # ... and that one to atomics
    ((4096, 768, 1536, 768, 1536, 0, 0), 1, 6, 0),
    ((4096, 768, 1536, 768, 1536, -3, 0), 0, 8, 0),                   # forced 256 x 256 without a workspace: atomics
    ((4096, 768, 1536, 768, 1536, -4, NO_LIMIT), 1, 6, 28311552),     # never the 256 x 256 kernel
    ((4096, 768, 1536, 768, 1536, -5, NO_LIMIT), 2, 6, 28311552),
    ((1920, 768, 768, 768, 768, 0, NO_LIMIT), 1, 4, 0),               # under the 16 MB floor
    ((1920, 768, 768, 768, 768, 4, NO_LIMIT), 1, 4, 9437184),         # explicit splits use the planes whatever their size
    ((1920, 768, 768, 768, 768, 1, NO_LIMIT), 1, 1, 0),
    ((21624, 2304, 768, 2304, 768, 0, NO_LIMIT), 0, 9, 63700992),     # the body of the ragged split
    ((21624, 2304, 768, 2304, 768, 0, 0), 1, 4, 0),                   # no workspace: all rows in one 128 x 128 call
    ((4096, 1000, 768, 1000, 768, 0, NO_LIMIT), 2, 8, 25165824),
    ((4096, 768, 1536, 1 << 21, 1536, 0, NO_LIMIT), 1, 6, 28311552),  # rows too far apart for the 256 x 256 kernel's 32-bit offsets
]


def test_gemm_workspace_and_plan_tables():
    """xfm_gemm_tn_workspace / _batch_workspace / _group_workspace / xfm_gemm_nt_ksplit_workspace, xfm_gemm_nt_plan and xfm_gemm_tn_plan
    over fixed tables, in a fresh process without XFM_* knobs (the child loads the library alone: no GPU, no torch)."""
    import json
    import subprocess
    import sys
    from xfm_amd import build
    child = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I, L, P = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
class Item(ctypes.Structure):
    _fields_ = [("dY", P), ("ldy", L), ("X", P), ("ldx", L), ("dW", P), ("ldw", L), ("dbias", P), ("N", I), ("K", I)]
sig = {"tn": ("xfm_gemm_tn_workspace", [I] * 3), "batch": ("xfm_gemm_tn_batch_workspace", [I] * 4),
       "group": ("xfm_gemm_tn_group_workspace", [I, P, I]), "ksplit": ("xfm_gemm_nt_ksplit_workspace", [I] * 3)}
for name, args in sig.values():
    getattr(lib, name).restype, getattr(lib, name).argtypes = L, args
lib.xfm_gemm_nt_plan.argtypes = [I] * 5 + [P] * 2
lib.xfm_gemm_tn_plan.argtypes = [I] * 3 + [L] * 2 + [I, L] + [P] * 3
ws, nt, tn = json.load(sys.stdin)
out = [[], [], []]
for kind, a in ws:
    if kind == "group":   # dummy non-NULL, 16-byte aligned pointers: the query dereferences none of them
        arr = (Item * len(a[1]))(*[Item(0x10000, N, 0x10000, K, 0x10000, K, None, N, K) for N, K in a[1]])
        a = (len(a[1]), ctypes.addressof(arr), a[0])
    out[0].append(getattr(lib, sig[kind][0])(*a))
c, r, u = I(), I(), L()
for a in nt:
    assert lib.xfm_gemm_nt_plan(*a, ctypes.addressof(c), ctypes.addressof(r)) == 0
    out[1].append([c.value, r.value])
for a in tn:
    assert lib.xfm_gemm_tn_plan(*a, ctypes.addressof(c), ctypes.addressof(r), ctypes.addressof(u)) == 0
    out[2].append([c.value, r.value, u.value])
print(json.dumps(out))
"""
    assert len(GEMM_WORKSPACE_TABLE) >= 25
    e = {k: v for k, v in os.environ.items() if not k.startswith("XFM_")}
    rows = [[(k, a) for k, a, _ in GEMM_WORKSPACE_TABLE], [a for a, _, _ in GEMM_NT_PLAN_TABLE], [a for a, _, _, _ in GEMM_TN_PLAN_TABLE]]
    r = subprocess.run([sys.executable, "-c", child, build.build()], input=json.dumps(rows), env=e, capture_output=True, text=True, check=True)
    ws, nt, tn = json.loads(r.stdout)
    assert ws == [w for _, _, w in GEMM_WORKSPACE_TABLE], [(row, got) for row, got in zip(GEMM_WORKSPACE_TABLE, ws) if got != row[2]]
    assert nt == [[c, ra] for _, c, ra in GEMM_NT_PLAN_TABLE], nt
    assert tn == [[k, s, u] for _, k, s, u in GEMM_TN_PLAN_TABLE], tn
