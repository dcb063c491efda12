"""Host-side twin of tests/test_hip_bias_path_bounds.py (CPU, no GPU): the restatements and bounds that file holds the kernels to are
themselves right, and bite.

1. attention_util.bias_tile_index inverts: every (q, k) of a head appears exactly once in `tiled` and once in `tiled_t`, the rest of both
   is padding (-1e30 / 0), and bias_tile_ref reads none of the bias's padding columns.
2. A plain fp32 emulation of the three table-gradient forms of csrc/attention_aux.hip -- sequential additions onto the table (the atomic
   scatter, in position order), 64 lane sums + a wave tree + one addition (the sorted form), per-wave sums over the query rows + a fixed
   four-way merge + one addition (the grid form) -- stays within HOST_MAX of attention_util.table_grad_ref's bound, and prints
   `bias-ratio host <form> <G>x<H> <ratio>` (pytest -s).
3. Planted faults land past the bound: a gradient that skips the cls row, and one that swaps cls -> patch with patch -> cls."""
import pytest
import torch

import attention_util as A
from attention_util import F32
from test_attention_host import HOST_MAX

GRIDS = [(1, 1), (2, 3), (3, 5), (14, 12), (14, 3), (32, 1), (33, 1)]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def grid_index(G):
    from xfm_amd.beit2 import build_relative_position_index
    return build_relative_position_index(G, G)


def grad_case(G, H, seed=0):
    """(ddense fp32 [H, N, ld] with NaN in columns [N, ld), index [N, N], initial table fp32 [entries, H])"""
    N, E = G * G + 1, (2 * G - 1) ** 2 + 3
    ld = (N + 3) // 4 * 4 + 4
    dd = torch.full((H, N, ld), A.NAN)
    dd[:, :, :N] = _randn((H, N, N), 100 + seed)
    return dd, grid_index(G), _randn((E, H), 200 + seed)


# ---------------------------------------------------------------------------------------------------------------- the tile layout
@pytest.mark.parametrize("S", [16, 17, 65, 197, 208, 224])
def test_tile_layout_inverts(S):
    T = (S + 15) // 16
    q, k, k_t, q_t = A.bias_tile_index(S)
    assert q.shape == (T, T, 64, 4) and k_t.shape == (T + 1, T, 64, 4)
    for qq, kk in ((q, k), (q_t, k_t)):
        inside = (qq < S) & (kk < S)
        seen = torch.bincount((qq * S + kk)[inside], minlength=S * S)
        assert bool((seen == 1).all()), "a (q, k) pair is missing from the layout or appears twice"
        assert int(qq.max()) < 16 * (T + 1) and int(kk.max()) < 16 * (T + 1)
    assert bool((k_t[T] >= S).all()), "the extra key-tile row must lie wholly past the sequence"
    H, ld = 3, S + 5
    bias = torch.full((H, S, ld), A.NAN)
    bias[:, :, :S] = _randn((H, S, S), S)
    for scale in (0.125, 0.3):
        inv = torch.ones((), dtype=F32) / torch.tensor(scale, dtype=F32)
        tiled, tiled_t = A.bias_tile_ref(bias, S, scale)
        assert not bool(torch.isnan(tiled).any()) and not bool(torch.isnan(tiled_t).any()), "the reference read the bias's padding"
        inside = ((q < S) & (k < S)).expand(H, T, T, 64, 4)
        back = torch.zeros((H, S, S))
        hh = torch.arange(H).reshape(H, 1, 1, 1, 1).expand(H, T, T, 64, 4)
        back[hh[inside], q.expand_as(hh)[inside], k.expand_as(hh)[inside]] = tiled[inside]
        assert torch.equal(back, bias[:, :, :S] * inv)
        assert bool((tiled[(k >= S).expand_as(hh)] == -1.0e30).all()) and bool((tiled[((q >= S) & (k < S)).expand_as(hh)] == 0).all())
        # tiled_t is the same tile of the transposed bias, plus one key-tile row of -1e30
        want_t, _ = A.bias_tile_ref(bias[:, :, :S].transpose(1, 2).contiguous(), S, scale)
        keys_past = (k_t[:T] >= S).expand(H, T, T, 64, 4)
        same = torch.where(keys_past, torch.full((), -1.0e30), torch.where((q_t[:T] >= S).expand_as(keys_past), torch.zeros(()), want_t))
        assert torch.equal(tiled_t[:, :T], same) and bool((tiled_t[:, T] == -1.0e30).all())


def test_relpos_ref_is_the_index():
    G, H = 3, 5
    N, E = G * G + 1, (2 * G - 1) ** 2 + 3
    table, index = _randn((E, H), 1), grid_index(G)
    dense, dense_t = A.relpos_ref(table, index, H, N, 12)
    for h in range(H):
        for i in range(N):
            for j in range(N):
                assert float(dense[h, i, j]) == float(table[index[i, j], h]) == float(dense_t[h, j, i])
    assert float(dense[:, :, N:].abs().max()) == 0.0 and float(dense_t[:, :, N:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------- fp32 emulation
def _positions(index, entries):
    """positions sorted by entry, padded: (pos int64 [entries, nmax], valid bool [entries, nmax])"""
    flat = index.reshape(-1)
    order = torch.sort(flat, stable=True).indices
    count = torch.bincount(flat, minlength=entries)
    start = torch.cumsum(count, 0) - count
    nmax = int(count.max())
    slot = torch.arange(nmax)[None, :]
    valid = slot < count[:, None]
    pos = order[(start[:, None] + slot).clamp(max=flat.numel() - 1)]
    return pos, valid


def _terms(dd, pos, valid):
    """fp32 [entries, nmax, H]: ddense at every position of every entry, 0 in the padding slots"""
    N = dd.shape[1]
    t = dd[:, pos // N, pos % N].permute(1, 2, 0)
    return torch.where(valid.unsqueeze(-1), t, torch.zeros(()))


def emul_scatter(dd, index, initial, skip_row=None, swap=None):
    """relpos_scatter_kernel with its atomics in position order: one fp32 addition onto the table per position.  Faults: skip_row (query
    row i contributes nothing), swap (two entries exchanged in the index)."""
    E = initial.shape[0]
    index = index.clone()
    if swap is not None:
        a, b = index == swap[0], index == swap[1]
        index[a], index[b] = swap[1], swap[0]
    dd = dd.clone()
    if skip_row is not None:
        dd[:, skip_row, :index.shape[0]] = 0.0
    pos, valid = _positions(index, E)
    t = _terms(dd, pos, valid)
    out = initial.clone()
    for n in range(t.shape[1]):
        out = torch.where(valid[:, n:n + 1], out + t[:, n], out)
    return out


def emul_sorted(dd, index, initial):
    """relpos_gather_grad_kernel: lane l sums positions l, l + 64, ... of the entry in order; a butterfly over the 64 lanes; += once"""
    E = initial.shape[0]
    pos, valid = _positions(index, E)
    t = _terms(dd, pos, valid)
    pad = (-t.shape[1]) % 64
    t = torch.cat([t, torch.zeros((E, pad, t.shape[2]))], 1).reshape(E, -1, 64, t.shape[2])
    lanes = torch.zeros((E, 64, t.shape[3]))
    for trip in range(t.shape[1]):
        lanes = lanes + t[:, trip]
    for step in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, torch.arange(64) ^ step]
    return initial + lanes[:, 0]


def emul_grid(dd, G, initial):
    """relpos_grid_grad_kernel: workgroup = (head, dy), lane = dx, wave w sums the query rows y0 + w, y0 + w + 4, ... over xi in order;
    (w0 + w1) + (w2 + w3), += once.  The cls entries: 256 threads stride the row / the column, a wave tree, the same merge."""
    H = dd.shape[0]
    N, W = G * G + 1, 2 * G - 1
    out = initial.clone()
    dy = torch.arange(W) - (G - 1)
    dx = torch.arange(W) - (G - 1)
    y0 = dy.clamp(min=0)
    y1 = torch.where(dy < 0, G + dy, torch.full_like(dy, G))
    acc = torch.zeros((4, W, W, H))
    rows = torch.arange(W)
    for yi in range(G):
        live_y = (yi >= y0) & (yi < y1)                                                  # [W] over dy
        wsel = (yi - y0) % 4
        yj = (yi - dy).clamp(0, G - 1)
        for xi in range(G):
            xj = xi - dx
            live = live_y[:, None] & ((xj >= 0) & (xj < G))[None, :]                      # [dy, dx]
            i = 1 + yi * G + xi
            j = 1 + yj[:, None] * G + xj.clamp(0, G - 1)[None, :]
            term = torch.where(live.unsqueeze(-1), dd[:, i, j].permute(1, 2, 0), torch.zeros(()))
            acc[wsel, rows] = acc[wsel, rows] + term
    out[:W * W] = out[:W * W] + ((acc[0] + acc[1]) + (acc[2] + acc[3])).reshape(W * W, H)

    def strided(v):     # v fp32 [n, H], element t of it on thread t % 256 -> the workgroup's sum
        pad = (-v.shape[0]) % 256
        v = torch.cat([v, torch.zeros((pad, H))], 0).reshape(-1, 256, H)
        th = torch.zeros((256, H))
        for trip in range(v.shape[0]):
            th = th + v[trip]
        th = th.reshape(4, 64, H)
        for step in (32, 16, 8, 4, 2, 1):
            th = th + th[:, torch.arange(64) ^ step]
        return (th[0, 0] + th[1, 0]) + (th[2, 0] + th[3, 0])

    E = W * W + 3
    out[E - 3] = out[E - 3] + strided(dd[:, 0, 1:N].t())
    out[E - 2] = out[E - 2] + strided(dd[:, 1:N, 0].t())
    out[E - 1] = out[E - 1] + dd[:, 0, 0]
    return out


def _ratio(got, ref, b32, what):
    return A.check_f32(got, ref, b32, what)


@pytest.mark.parametrize("G,H", GRIDS)
def test_emulated_table_gradients_stay_within_the_bound(G, H):
    dd, index, initial = grad_case(G, H)
    ref, b32 = A.table_grad_ref(dd, index, initial.shape[0], initial)
    forms = {"scatter": emul_scatter(dd, index, initial), "sorted": emul_sorted(dd, index, initial), "grid": emul_grid(dd, G, initial)}
    for name, got in forms.items():
        ratio = _ratio(got, ref, b32, name)
        print(f"bias-ratio host {name} {G}x{H} {ratio:.3g}")
        assert ratio <= HOST_MAX, f"{name} {G}x{H}: a correct fp32 evaluation at {ratio:.3g} of the bound: the derivation misses a rounding"


def test_emulated_gradient_on_a_random_index_with_an_empty_entry():
    H, N, E = 5, 10, 40
    g = torch.Generator(device="cpu").manual_seed(3)
    index = torch.randint(0, E - 1, (N, N), generator=g)
    index[index == 7] = 8                                                                # entries 7 and E - 1 own no position
    dd, initial = _randn((H, N, 12), 4), _randn((E, H), 5)
    ref, b32 = A.table_grad_ref(dd, index, E, initial)
    assert torch.equal(ref[7], initial[7].double()) and torch.equal(ref[E - 1], initial[E - 1].double())
    for name, got in (("scatter", emul_scatter(dd, index, initial)), ("sorted", emul_sorted(dd, index, initial))):
        assert _ratio(got, ref, b32, name) <= HOST_MAX
        assert torch.equal(got[7], initial[7]), "an entry without positions keeps its bits"


# ------------------------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("G,H", [(2, 3), (14, 12)])
def test_planted_gradient_faults_land_past_the_bound(G, H):
    dd, index, initial = grad_case(G, H)
    E = initial.shape[0]
    ref, b32 = A.table_grad_ref(dd, index, E, initial)
    with pytest.raises(AssertionError, match="past the bound"):
        _ratio(emul_scatter(dd, index, initial, skip_row=0), ref, b32, "the cls row skipped")
    with pytest.raises(AssertionError, match="past the bound"):
        _ratio(emul_scatter(dd, index, initial, swap=(E - 3, E - 2)), ref, b32, "cls -> patch swapped with patch -> cls")
    dd2 = dd.clone()
    dd2[:, 1, 1] = 0.0                                                                   # (yi, xi) = (yj, xj) = (0, 0): the centre entry
    got = emul_scatter(dd2, index, initial)
    with pytest.raises(AssertionError, match="past the bound"):
        _ratio(got, ref, b32, "one position dropped")
