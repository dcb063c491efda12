"""The decoding kernels (csrc/decode.hip) against fp64 restatements, elementwise, on a real MI355X: xfm_decode_attn inside poisoned cache
buffers (nothing past the end is read, exactly one row is appended) and xfm_next_token (token, flags, counter and the written column exact,
the log-probability within the cross-entropy forward bound).  References and bounds: tests/decode_util.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_util import SCALE  # noqa: E402
from decode_util import decode_attn_ref, next_token_ref  # noqa: E402
from gemm_strided_util import NAN, SENTINEL, check_bf16, check_f32  # noqa: E402

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
B = 3


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _keep(family, rows, n):
    """int32 [rows, n]: tail = a ragged masked tail; holes = every third key masked; new = only the last (the new) key kept"""
    keep = torch.ones((rows, n), dtype=I32)
    for r in range(rows):
        if family == "tail":
            keep[r, n - (1 + (7 * r + 3) % max(n // 2, 1)):] = 0
        elif family == "holes":
            keep[r, torch.arange(n) % 3 == r % 2] = 0
        elif family == "new":
            keep[r] = 0
            keep[r, n - 1] = 1
    return keep


@pytest.mark.parametrize("family", [None, "tail", "holes", "new"])
@pytest.mark.parametrize("pos", [0, 1, 15, 16, 17, 63, 64, 65, 200])
@pytest.mark.parametrize("H", [12, 2])
def test_decode_attn_self_mode(H, pos, family):
    from xfm_amd import functional as Fx
    if family == "tail" and pos == 0:
        family = "new"   # a one-key row whose tail is masked IS the all-masked row; keep the single key instead
    D, cap, n = H * 64, pos + 3, pos + 1
    rs = 2 * D + 8                      # K | V side by side with slack columns; rows stay on 16 bytes
    seed = 1000 * H + pos
    past_k, past_v = _randn((B, pos, H, 64), seed).to(BF16), _randn((B, pos, H, 64), seed + 1).to(BF16)
    qkv = _randn((B, 3 * D), seed + 2).to(BF16)
    # the cache: rows >= pos are NaN (nothing past the end may be read), the slack columns hold a sentinel
    cache = torch.full((B, cap, rs), NAN, dtype=BF16)
    cache[:, :, 2 * D:] = SENTINEL
    cache[:, :pos, :D] = past_k.reshape(B, pos, D)
    cache[:, :pos, D:2 * D] = past_v.reshape(B, pos, D)
    before = cache.clone()
    keep = None if family is None else _keep(family, B, n)
    dev = torch.device("cuda")
    g_cache, g_qkv = cache.to(dev), qkv.to(dev)
    rows = g_cache.view(B * cap, rs)
    out_parent = torch.full((B + 2, D + 8), SENTINEL, dtype=BF16, device=dev)
    out = out_parent[1:1 + B, :D]
    Fx.decode_attn(g_qkv[:, :D], rows[:, :D], rows[:, D:2 * D], cap, H, SCALE, k_new=g_qkv[:, D:2 * D], v_new=g_qkv[:, 2 * D:], pos=pos,
                   key_keep=None if keep is None else keep.to(dev), out=out)
    torch.cuda.synchronize()
    # exactly one row written, with exactly k_new / v_new
    after = g_cache.cpu()
    want = before.clone()
    want[:, pos, :D], want[:, pos, D:2 * D] = qkv[:, D:2 * D], qkv[:, 2 * D:]
    assert torch.equal(after.view(torch.int16), want.view(torch.int16)), "the cache differs outside row pos, or row pos is not k_new | v_new"
    o_cpu = out_parent.cpu()
    inside = torch.zeros_like(o_cpu, dtype=torch.bool)
    inside[1:1 + B, :D] = True
    assert bool((o_cpu[~inside] == SENTINEL).all()), "output written outside its rows"
    K = torch.cat([past_k, qkv[:, D:2 * D].view(B, 1, H, 64)], dim=1)
    V = torch.cat([past_v, qkv[:, 2 * D:].view(B, 1, H, 64)], dim=1)
    ref, b32 = decode_attn_ref(qkv[:, :D].view(B, H, 64), K, V, keep, SCALE)
    ratio = check_bf16(o_cpu[1:1 + B, :D], ref, b32, f"decode_attn self H={H} pos={pos} {family}")
    print(f"decode_attn self H={H} pos={pos} mask={family}: worst err / bound {ratio:.3g}")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Sk", [1, 30, 197, 577])
def test_decode_attn_cross_mode(Sk, masked):
    from xfm_amd import functional as Fx
    H, U, Bq = 12, 3, 5
    D = H * 64
    idx = torch.tensor([2, 0, 2, 1, 0], dtype=I32)          # repeats: rows share a source
    kv = _randn((U * Sk, 2 * D), 77 + Sk).to(BF16)          # the K | V projection of the encoder states IS the cache
    q = _randn((Bq, D), 78 + Sk).to(BF16)
    keep = None
    if masked:
        keep = torch.ones((U, Sk), dtype=I32)
        keep[1] = _keep("holes", 2, Sk)[1]
        keep[2, Sk - Sk // 3:] = 0                           # (Sk = 1: nothing masked in source 2)
        if Sk > 1:
            keep[0, 1:] = 0                                  # a source with one visible key
    dev = torch.device("cuda")
    parent = torch.full((U * Sk + 2, 2 * D), NAN, dtype=BF16)   # a NaN row before and after: nothing outside the sources is read
    parent[1:1 + U * Sk] = kv
    g = parent.to(dev)[1:1 + U * Sk]
    out = Fx.decode_attn(q.to(dev), g[:, :D], g[:, D:], Sk, H, SCALE, Sk=Sk, key_keep=None if keep is None else keep.to(dev),
                         kv_index=idx.to(dev))
    torch.cuda.synchronize()
    src = idx.long()
    K = kv[:, :D].view(U, Sk, H, 64)[src]
    V = kv[:, D:].view(U, Sk, H, 64)[src]
    ref, b32 = decode_attn_ref(q.view(Bq, H, 64), K, V, None if keep is None else keep[src], SCALE)
    ratio = check_bf16(out.cpu(), ref, b32, f"decode_attn cross Sk={Sk} masked={masked}")
    print(f"decode_attn cross Sk={Sk} masked={masked}: worst err / bound {ratio:.3g}")
    # the identity index
    out_id = Fx.decode_attn(q[:U].to(dev), g[:, :D], g[:, D:], Sk, H, SCALE, Sk=Sk, key_keep=None if keep is None else keep.to(dev))
    ref, b32 = decode_attn_ref(q[:U].view(U, H, 64), kv[:, :D].view(U, Sk, H, 64), kv[:, D:].view(U, Sk, H, 64), keep, SCALE)
    check_bf16(out_id.cpu(), ref, b32, f"decode_attn cross identity Sk={Sk}")


NT_B = 5
NT_SHAPES = [(50265, 50304), (30522, 30528), (257, 264), (7, 8)]


def _next_token_case(V, ld, seed):
    """Rows: 0 two equal maxima; 1 -inf entries around the maximum; 2 a planted eos as the argmax; 3 already finished; 4 plain."""
    x = 2.0 * _randn((NT_B, ld), seed)
    x[:, V:] = float("nan")                        # the padding columns are never read
    hi = float(x[:, :V].max()) + 3.0
    a, b = (1, V - 2) if V > 3 else (0, V - 1)
    x[0, a] = x[0, b] = hi                          # equal maxima: the lowest column wins
    x[1, 0] = float("-inf")
    x[1, V - 1] = float("-inf")
    x[1, V // 2] = hi
    eos = [min(5, V - 1), min(3, V - 2)]
    x[2, eos[0]] = hi
    max_length, cur_len = 9, 6
    ids = torch.full((NT_B, max_length), -7, dtype=I64)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    ids[:, :cur_len] = torch.randint(0, V, (NT_B, cur_len), generator=g)
    return x, ids, cur_len, eos


@pytest.mark.parametrize("penalty", [1.0, 1.3])
@pytest.mark.parametrize("V,ld", NT_SHAPES)
def test_next_token_greedy(V, ld, penalty):
    from xfm_amd import functional as Fx
    x, ids, cur_len, eos = _next_token_case(V, ld, 31 + V)
    if penalty != 1.0:
        # duplicate ids in a row, on a positive and on a negative logit: the restatement applies the penalty once per DISTINCT id, so a
        # kernel that applied it per occurrence would move row 4's maximum (hi / 1.69 for hi / 1.3) and its log-probability past the bound
        p, n = (2, 4) if V > 6 else (1, 3)
        hi = float(x[:, :V].max()) + 1.0
        x[4, p], x[4, n] = hi, -1.0
        ids[4, :4] = torch.tensor([p, n, p, n])
    pad, steps, step = (1 if V > 2 else 0), 4, 2
    unfinished = torch.tensor([1, 1, 1, 0, 1], dtype=I32)
    dev = torch.device("cuda")
    g_x, g_ids, g_unf = x.to(dev), ids.to(dev), unfinished.to(dev)
    hist_u = torch.full((NT_B, steps), -3, dtype=I32, device=dev)
    hist_lp = torch.full((NT_B, steps), SENTINEL, dtype=F32, device=dev)
    count = torch.tensor([100], dtype=I32, device=dev)
    Fx.next_token(g_x, V, g_ids, cur_len, g_unf, hist_u, hist_lp, step, pad, eos, penalty=penalty, n_unfinished=count)
    torch.cuda.synchronize()
    r = next_token_ref(x, V, ids, cur_len, penalty, unfinished, pad, eos)
    if penalty == 1.0:   # the case is what it claims to be (with a penalty the random ids may move the planted maxima)
        assert r["tok"][0] == (1 if V > 3 else 0) and r["tok"][2] == eos[0] and r["unfinished"][2] == 0
    got_ids = g_ids.cpu()
    assert got_ids[:, cur_len].tolist() == r["add"].tolist(), (got_ids[:, cur_len], r["add"])
    assert got_ids[3, cur_len] == pad
    want_ids = ids.clone()
    want_ids[:, cur_len] = r["add"]
    assert torch.equal(got_ids, want_ids), "ids written outside column cur_len"
    assert g_unf.cpu().tolist() == r["unfinished"].tolist() and r["unfinished"][3] == 0
    assert int(count) == 100 + r["count"]
    hu, hl = hist_u.cpu(), hist_lp.cpu()
    assert hu[:, step].tolist() == r["flag"].tolist() and hu[3, step] == 0
    other = [c for c in range(steps) if c != step]
    assert bool((hu[:, other] == -3).all()) and bool((hl[:, other] == SENTINEL).all()), "history written outside column step"
    assert torch.equal(g_x.cpu().view(I32), x.view(I32)), "the logits were modified"
    ratio = check_f32(hl[:, step].contiguous(), r["lp"], r["b_lp"], f"next_token log-probability V={V} penalty={penalty}")
    print(f"next_token V={V} ld={ld} penalty={penalty}: tokens {r['tok'].tolist()}, log-prob worst err / bound {ratio:.3g}")


def test_next_token_pre_drawn_and_bits():
    """The sampling mode takes the token as given and does the rest; two launches on the same inputs give the same bits."""
    from xfm_amd import functional as Fx
    V, ld = 257, 264
    x, ids, cur_len, eos = _next_token_case(V, ld, 5)
    x[1, 7] = float("-inf")
    drawn = torch.tensor([4, 11, eos[1], 9, 200], dtype=I64)
    unfinished = torch.tensor([1, 1, 1, 0, 1], dtype=I32)
    dev = torch.device("cuda")
    outs = []
    for _ in range(2):
        g_ids, g_unf = ids.to(dev), unfinished.to(dev)
        hist_u = torch.zeros((NT_B, 1), dtype=I32, device=dev)
        hist_lp = torch.zeros((NT_B, 1), dtype=F32, device=dev)
        count = torch.zeros(1, dtype=I32, device=dev)
        Fx.next_token(x.to(dev), V, g_ids, cur_len, g_unf, hist_u, hist_lp, 0, 1, eos, next_token=drawn.to(dev), n_unfinished=count)
        torch.cuda.synchronize()
        outs.append((g_ids.cpu(), g_unf.cpu(), hist_u.cpu(), hist_lp.cpu(), int(count)))
    r = next_token_ref(x, V, ids, cur_len, 1.0, unfinished, 1, eos, next_token=drawn)
    got_ids, got_unf, hu, hl, cnt = outs[0]
    assert got_ids[:, cur_len].tolist() == r["add"].tolist() == [4, 11, eos[1], 1, 200]
    assert got_unf.tolist() == r["unfinished"].tolist() == [1, 1, 0, 0, 1] and cnt == r["count"] == 3
    check_f32(hl[:, 0].contiguous(), r["lp"], r["b_lp"], "next_token pre-drawn log-probability")
    assert torch.equal(outs[0][3].view(I32), outs[1][3].view(I32)) and torch.equal(outs[0][0], outs[1][0])
