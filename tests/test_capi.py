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


def test_attention_sources_set_the_lds_attribute_once_and_include_at_the_top():
    """One launcher owns hipFuncAttributeMaxDynamicSharedMemorySize for every attention kernel instantiation, and attention.hip (the host
    side) pulls in its kernel families before its first function: no file order to work around."""
    csrc = os.path.join(ROOT, "xfm_amd", "csrc")
    assert sorted(f for f in os.listdir(csrc) if f.startswith("attention")) == sorted(ATTENTION_SOURCES)
    text = {f: open(os.path.join(csrc, f)).read() for f in ATTENTION_SOURCES}
    assert sum(s.count("hipFuncSetAttribute") for s in text.values()) == 1
    lines = text["attention.hip"].splitlines()
    first_fn = next(i for i, l in enumerate(lines) if re.match(r"^(static |int |long |template |__global__ |struct |enum )", l))
    includes = [i for i, l in enumerate(lines) if l.lstrip().startswith("#include")]
    assert includes and max(includes) < first_fn, (includes, first_fn)
