"""The bias path of the dense attention kernels (csrc/attention_aux.hip) inside poisoned buffers: bit for bit where values only move,
under elementwise fp64 bounds where they are summed.

tests/test_hip_kernels.py sees xfm_bias_tile only through attention outputs at 1e-2, never asks xfm_relpos_gather for its transposed
copy, and holds the three table gradients to max |err| / max |ref| <= 1e-5 / 2e-6 on fresh contiguous operands.  Here
  xfm_bias_tile       both copies equal attention_util.bias_tile_ref (the accumulator layout of include/xfm_hip.h restated as indices;
                      tests/test_bias_path_host.py shows that it inverts), the bias's padding columns are NaN, each output ends at a
                      sentinel, either output may be absent, and a rejected call writes nothing;
  xfm_relpos_gather   dense and dense_t equal the index, padding columns zero, sentinels around both;
  table gradients     every entry within (n + 1) u32 (|initial| + sum |term|) of an fp64 index_add of the same fp32 ddense, onto a random
                      initial table inside a sentinel parent, NaN in ddense's padding columns; the sorted and grid forms give the same
                      bits twice;
  end to end          table -> relpos_gather -> bias_tile -> the ViT forward at S = 197 gives the bits of the forward on a bias built on
                      the CPU from the same table.
Every bounded check prints `bias-ratio gpu <form> <index> <G or N>x<H> <worst err / bound>` (pytest -s)."""
import ctypes

import pytest
import torch

import attention_util as A
from attention_util import BF16, F32, I32, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda"
XFM_E_ARG = -1


def _lib():
    from xfm_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _out(n):
    """an fp32 output of n floats on a 16-byte boundary inside a 7.0-filled parent"""
    return A.embed_vec(torch.full((n,), A.SENTINEL, dtype=F32, device=DEV), 8, 8, A.SENTINEL)


def _bias(H, S, ld, seed):
    """(view [H * S, ld], parent, cpu copy [H, S, ld]): NaN in columns [S, ld) and in the rows around"""
    b = torch.full((H, S, ld), A.NAN)
    b[:, :, :S] = _randn((H, S, S), seed)
    view, parent = A.embed(b.reshape(H * S, ld).to(DEV), ld, 0, 4, 3, A.NAN)
    return view, parent, b


def grid_index(G):
    from xfm_amd.beit2 import build_relative_position_index
    return build_relative_position_index(G, G)


# -------------------------------------------------------------------------------------------------------------------- xfm_bias_tile
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("S", [16, 17, 65, 197, 208, 224])
def test_bias_tile_is_the_layout(S, H):
    T = (S + 15) // 16
    n, n_t = H * T * T * 256, H * (T + 1) * T * 256
    for ld, scale in ((S, SCALE), (S + 7, 0.3)):       # 0.3: fl(1 / scale) is inexact, bias fl(1 / scale) is not bias / scale
        bias, _, b_cpu = _bias(H, S, ld, 10 * S + H)
        want, want_t = (t.to(DEV).reshape(-1) for t in A.bias_tile_ref(b_cpu, S, scale))
        for ask, ask_t in ((True, True), (True, False), (False, True)):
            (tiled, parent), (tiled_t, parent_t) = _out(n), _out(n_t)
            rc = _lib().xfm_bias_tile(bias.data_ptr(), H, S, ld, scale, tiled.data_ptr() if ask else 0, tiled_t.data_ptr() if ask_t else 0,
                                      _stream())
            torch.cuda.synchronize()
            assert rc == 0, _lib().xfm_last_error()
            A.assert_outside_untouched(parent, tiled, A.SENTINEL, "tiled")
            A.assert_outside_untouched(parent_t, tiled_t, A.SENTINEL, "tiled_t")
            for name, got, ref, asked in (("tiled", tiled, want, ask), ("tiled_t", tiled_t, want_t, ask_t)):
                if not asked:
                    assert bool((got == A.SENTINEL).all()), f"{name} was not requested and was written"
                    continue
                bad = _bits(got) != _bits(ref)
                assert not bool(bad.any()), (f"{name} S={S} ld={ld}: {int(bad.sum())} of {got.numel()} floats differ from the layout, first at "
                                             f"{int(bad.nonzero()[0])}")


@pytest.mark.parametrize("what", ["null bias", "ld < S", "misaligned tiled", "misaligned tiled_t"])
def test_bias_tile_rejections_launch_nothing(what):
    H, S = 2, 17
    T = (S + 15) // 16
    bias, _, _ = _bias(H, S, S + 3, 1)
    (tiled, parent), (tiled_t, parent_t) = _out(H * T * T * 256 + 4), _out(H * (T + 1) * T * 256 + 4)
    rc = _lib().xfm_bias_tile(0 if what == "null bias" else bias.data_ptr(), H, S, S - 1 if what == "ld < S" else S + 3, SCALE,
                              tiled.data_ptr() + (4 if what == "misaligned tiled" else 0),
                              tiled_t.data_ptr() + (4 if what == "misaligned tiled_t" else 0), _stream())
    torch.cuda.synchronize()
    assert rc == XFM_E_ARG
    assert bool((parent == A.SENTINEL).all()) and bool((parent_t == A.SENTINEL).all()), "a rejected call wrote an output"


# ---------------------------------------------------------------------------------------------------------------- xfm_relpos_gather
@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("G", [1, 2, 3, 14])
def test_relpos_gather_is_the_index(G, H):
    N, E = G * G + 1, (2 * G - 1) ** 2 + 3
    index = grid_index(G)
    table, table_parent = A.embed(_randn((E, H), 30 + G).to(DEV), H, 0, 2, 2, A.NAN)
    idx32 = index.to(I32).to(DEV).contiguous()
    for ld in sorted({(N + 3) // 4 * 4, (N + 15) // 16 * 16}):
        want, want_t = A.relpos_ref(table.cpu(), index, H, N, ld)
        for with_t in (True, False):
            (dense, parent), (dense_t, parent_t) = _out(H * N * ld), _out(H * N * ld)
            rc = _lib().xfm_relpos_gather(table.data_ptr(), idx32.data_ptr(), H, N, ld, dense.data_ptr(), dense_t.data_ptr() if with_t else 0,
                                          _stream())
            torch.cuda.synchronize()
            assert rc == 0, _lib().xfm_last_error()
            A.assert_outside_untouched(parent, dense, A.SENTINEL, "dense")
            A.assert_outside_untouched(parent_t, dense_t, A.SENTINEL, "dense_t")
            assert torch.equal(_bits(dense), _bits(want.to(DEV).reshape(-1))), f"dense G={G} H={H} ld={ld}"
            if with_t:
                assert torch.equal(_bits(dense_t), _bits(want_t.to(DEV).reshape(-1))), f"dense_t G={G} H={H} ld={ld}"
            else:
                assert bool((dense_t == A.SENTINEL).all()), "dense_t was not requested and was written"


# ------------------------------------------------------------------------------------------------------------------ table gradients
def _ddense(H, N, seed):
    """(view [H * N, ld], parent): NaN in the padding columns [N, ld) and in the rows around"""
    ld = (N + 3) // 4 * 4 + 4
    dd = torch.full((H, N, ld), A.NAN)
    dd[:, :, :N] = _randn((H, N, N), seed)
    view, parent = A.embed(dd.reshape(H * N, ld).to(DEV), ld, 0, 4, 3, A.NAN)
    return view, parent, ld


def _launch(form, dd, ld, index, E, H, N, G, dtable):
    from xfm_amd import functional as Fx
    idx32 = index.to(I32).to(DEV).contiguous()
    if form == "scatter":
        return _lib().xfm_relpos_scatter(dd.data_ptr(), idx32.data_ptr(), H, N, ld, dtable.data_ptr(), _stream())
    if form == "sorted":
        order, start = Fx.relpos_sorted_index(idx32, E)
        return _lib().xfm_relpos_scatter_sorted(dd.data_ptr(), order.data_ptr(), start.data_ptr(), E, H, N, ld, dtable.data_ptr(), _stream())
    return _lib().xfm_relpos_grid_grad(dd.data_ptr(), H, G, ld, dtable.data_ptr(), _stream())


def _table_grad(forms, index, E, H, N, G, tag, seed):
    dd, dd_parent, ld = _ddense(H, N, seed)
    initial = _randn((E, H), seed + 1).to(DEV)
    ref, b32 = A.table_grad_ref(dd.reshape(H, N, ld), index, E, initial)
    before = dd_parent.clone()
    for form in forms:
        runs = []
        for _ in range(2):
            dtable, parent = A.embed(initial, H, 0, 3, 3, A.SENTINEL)
            rc = _launch(form, dd, ld, index, E, H, N, G, dtable)
            torch.cuda.synchronize()
            assert rc == 0, _lib().xfm_last_error()
            A.assert_outside_untouched(parent, dtable, A.SENTINEL, f"dtable ({form})")
            print(f"bias-ratio gpu {form} {tag} {G or N}x{H} {A.check_f32(dtable, ref, b32, form):.3g}")
            runs.append(dtable.clone())
        if form != "scatter":      # one owner per entry, a fixed order: no atomics
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), f"{form}: two launches gave different bits"
    assert torch.equal(_bits(dd_parent), _bits(before)), "ddense was written"


@pytest.mark.parametrize("H", [1, 3, 5, 12])
@pytest.mark.parametrize("G", [1, 2, 3, 14, 32, 33])
def test_table_gradients_within_bounds_on_the_grid_index(G, H):
    _table_grad(("scatter", "sorted", "grid"), grid_index(G), (2 * G - 1) ** 2 + 3, H, G * G + 1, G, "grid", 40 + G)


@pytest.mark.parametrize("H", [1, 3, 5, 12])
def test_table_gradients_within_bounds_on_a_random_index(H):
    """An index without the grid's structure, with entries that own no position (they must keep their bits) and one that owns 70: more
    than a trip of the sorted form's 64 lanes."""
    N, E = 21, 90
    index = torch.randint(0, E - 1, (N, N), generator=torch.Generator(device="cpu").manual_seed(9))
    index[index == 7] = 8
    index.reshape(-1)[:70] = 11
    _table_grad(("scatter", "sorted"), index, E, H, N, 0, "random", 60)


# ----------------------------------------------------------------------------------------------------------------------- end to end
def test_table_to_vit_forward_end_to_end():
    """table -> xfm_relpos_gather -> xfm_bias_tile -> xfm_attn_fwd (the 13-tile ViT forward reading the tiled copy) at S = 197 against the
    same forward on a row-major bias built on the CPU from the same table: equal bits in o and lse.  (The ViT forward starts its
    accumulators from fl(bias fl(1 / scale)) whichever copy it reads: include/xfm_hip.h.)"""
    G, H, B = 14, 2, 2
    S, E = G * G + 1, (2 * G - 1) ** 2 + 3
    ld = 208
    index = grid_index(G)
    table = (0.5 * _randn((E, H), 70)).to(DEV)
    idx32 = index.to(I32).to(DEV).contiguous()
    dense = torch.full((H, S, ld), A.NAN, dtype=F32, device=DEV)
    assert _lib().xfm_relpos_gather(table.data_ptr(), idx32.data_ptr(), H, S, ld, dense.data_ptr(), 0, _stream()) == 0
    T = (S + 15) // 16
    tiled, _ = _out(H * T * T * 256)
    assert _lib().xfm_bias_tile(dense.data_ptr(), H, S, ld, SCALE, tiled.data_ptr(), 0, _stream()) == 0
    cpu_bias = A.relpos_ref(table.cpu(), index, H, S, ld)[0].to(DEV)
    sp = A.Spec("vit", B, H, S, S, B, None, False, None, False, 0.0, "randn", False, "end-to-end")
    c = A.make_case(sp)
    outs = []
    for bias, bias_tiled in ((dense, tiled), (cpu_bias, None)):
        buf = A.AttnBuffers(c, DEV)
        o, lse = buf.out16("o", B * S), buf.stat("lse")
        a = _lib_mod().AttnArgs(q=buf.q.data_ptr(), q_rs=buf.q.stride(0), k=buf.k.data_ptr(), k_rs=buf.k.stride(0), v=buf.v.data_ptr(),
                                v_rs=buf.v.stride(0), o=o.data_ptr(), o_rs=o.stride(0), lse=lse.data_ptr(), stat_ld=buf.ld_stat,
                                bias=bias.data_ptr(), bias_ld=ld, bias_tiled=0 if bias_tiled is None else bias_tiled.data_ptr(),
                                B=B, H=H, Sq=S, Sk=S, scale=SCALE, drop_scale=1.0)
        rc = _lib().xfm_attn_fwd(ctypes.byref(a), _stream())
        torch.cuda.synchronize()
        assert rc == 0, _lib().xfm_last_error()
        buf.check_outside()
        outs.append((o.clone(), lse[:, :S].clone()))
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)), "o differs between the device-built and the CPU-built bias"
    assert torch.equal(_bits(outs[0][1]), _bits(outs[1][1])), "lse differs between the device-built and the CPU-built bias"
    assert bool(torch.isfinite(outs[0][0].float()).all()) and bool(torch.isfinite(outs[0][1]).all())


def _lib_mod():
    from xfm_amd import _lib
    return _lib
