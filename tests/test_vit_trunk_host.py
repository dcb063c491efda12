"""Host-side checks of xfm_amd/vit_trunk.py, the part the three vision towers share: arena slots, what the trunk node asks a tower,
the layer-scale accessor, the drop-path draw and the relative-position bias plan.  CPU tensors only, no launch, no library call."""
import inspect
import types

import pytest
import torch

from xfm_amd import beit2, model_vqkd, vit, vit_trunk

D = 128   # two heads of 64; 32 px / 16 = a 2 x 2 patch grid


def _beit(depth=2, **kw):
    return beit2.VisionTransformer(img_size=32, embed_dim=D, depth=depth, num_heads=2, **kw)


def _plain(depth=2, **kw):
    return vit.VisionTransformer(img_size=32, embed_dim=D, depth=depth, num_heads=2, **kw)


def _tokenizer(depth=2):
    return model_vqkd.TokenizerEncoder(img_size=32, embed_dim=D, depth=depth, num_heads=2)


def _describe(tower):
    """[(slot name, weight operands, bias operands, need_t)], every Parameter named through its identity."""
    names = {id(p): n for n, p in tower.named_parameters()}
    return [(s.name, [names[id(w)] for w in s.weights], [b if isinstance(b, int) else names[id(b)] for b in s.biases], s.need_t)
            for s in tower.linear_slots()]


def _slots(qkv_bias_0, qkv_bias_1):
    return [("patch_embed", ["patch_embed.proj.weight"], ["patch_embed.proj.bias"], False),
            ("blocks.0.qkv", ["blocks.0.attn.qkv.weight"], qkv_bias_0, True),
            ("blocks.0.proj", ["blocks.0.attn.proj.weight"], ["blocks.0.attn.proj.bias"], True),
            ("blocks.0.fc1", ["blocks.0.mlp.fc1.weight"], ["blocks.0.mlp.fc1.bias"], True),
            ("blocks.0.fc2", ["blocks.0.mlp.fc2.weight"], ["blocks.0.mlp.fc2.bias"], True),
            ("blocks.1.qkv", ["blocks.1.attn.qkv.weight"], qkv_bias_1, True),
            ("blocks.1.proj", ["blocks.1.attn.proj.weight"], ["blocks.1.attn.proj.bias"], True),
            ("blocks.1.fc1", ["blocks.1.mlp.fc1.weight"], ["blocks.1.mlp.fc1.bias"], True),
            ("blocks.1.fc2", ["blocks.1.mlp.fc2.weight"], ["blocks.1.mlp.fc2.bias"], True)]


# the lists the three linear_slots() copies produced before they became one (recorded from them with _describe)
COMPOSED = _slots(["blocks.0.attn.q_bias", D, "blocks.0.attn.v_bias"], ["blocks.1.attn.q_bias", D, "blocks.1.attn.v_bias"])
FUSED_BIAS = _slots(["blocks.0.attn.qkv.bias"], ["blocks.1.attn.qkv.bias"])


@pytest.mark.parametrize("make, want", [(_beit, COMPOSED), (_plain, FUSED_BIAS), (_tokenizer, COMPOSED)], ids=["beit", "plain", "tokenizer"])
def test_linear_slots(make, want):
    tower = make()
    assert _describe(tower) == want
    assert tower._slot_patch.name == "patch_embed"
    assert [list(s) for s in tower._slots] == [["qkv", "proj", "fc1", "fc2"]] * 2
    assert [s[k].name for s in tower._slots for k in s] == [w[0] for w in want[1:]]


def test_what_the_node_asks_a_tower():
    b, p, t = _beit(), _plain(), _tokenizer()
    assert (b._rel_pos, b._pool_tail) == (True, True) and b._final_norm is b.fc_norm
    assert (p._rel_pos, p._pool_tail) == (False, False) and p._final_norm is p.norm
    assert (t._rel_pos, t._pool_tail) == (False, False) and t._final_norm is t.fc_norm
    assert not hasattr(t, "norm") and "norm.weight" not in t.state_dict() and "fc_norm.weight" in t.state_dict()
    assert vit_trunk._FusedViT._trunk_bwd_done is None and vit_trunk._FusedViT._block_grad_hook is None
    for tower in (b, p, t):
        assert tower._trunk_bwd_done is None and tower._block_grad_hook is None and tower._arena is None


def test_a_tower_must_say_its_final_norm_and_qkv_bias():
    class Forgetful(vit_trunk._FusedViT):
        pass
    with pytest.raises(AttributeError, match="_final_norm"):   # no default: a tower that forgets one fails, it does not borrow another's
        Forgetful()._final_norm
    with pytest.raises(AttributeError, match="_qkv_bias_parts"):
        Forgetful()._qkv_bias_parts


def test_trunk_node_probes_nothing():
    src = inspect.getsource(vit_trunk._TrunkFn)
    assert "getattr(vit" not in src and "hasattr(vit" not in src


def test_moved_names_stay_importable_from_beit2():
    for name in ("_TrunkFn", "_Affine", "_Dense", "PatchEmbed"):
        assert getattr(beit2, name) is getattr(vit_trunk, name)
    for name in ("_FAST_DELTA", "_VIT_FUSED_BWD", "_DEFER_WGRAD", "_RELPOS_AHEAD", "_DEFER_LN", "_WGRAD_GROUP_BLOCKS", "_GRAD_CHUNK_BLOCKS"):
        assert getattr(beit2, name) == getattr(vit_trunk, name)


def test_layer_scale_accessor(monkeypatch):
    asked = []
    monkeypatch.setattr(vit_trunk, "grad_of", lambda p: asked.append(p) or ("grad of", p))
    b = _beit()
    blk = b.blocks[1]
    for gamma in (blk.gamma_1, blk.gamma_2):
        got, dest = b._layer_scale(gamma)
        assert got is gamma and dest is None and not asked      # the forward marks no gradient live
        got, dest = b._layer_scale(gamma, grad=True)
        assert got is gamma and dest[1] is gamma and asked.pop() is gamma
    p = _plain()
    p._ones = torch.ones(D)
    for gamma in (p.blocks[1].gamma_1, p.blocks[1].gamma_2):
        assert gamma is None
        got, dest = p._layer_scale(gamma, grad=True)
        assert got is p._ones and dest is None and not asked


def test_ready_refuses_a_foreign_arena_that_lost_its_parameters():
    b = _beit()
    b._arena = types.SimpleNamespace(attached=lambda: False)
    with pytest.raises(RuntimeError, match=r"parameters were moved after the arena was built; call finalize\(\) again"):
        b._ready()


# ---- the drop-path draw ---------------------------------------------------------------------------
CPU = torch.device("cpu")


def test_plain_vit_without_drop_path_draws_nothing():
    p = _plain(depth=3).train()
    torch.manual_seed(7)
    before = torch.get_rng_state()
    assert p._drop_path_scales(4, CPU) is None
    assert torch.equal(torch.get_rng_state(), before) and p._dp_keep is None


def test_beit_without_drop_path_still_draws():
    b = _beit(depth=3).train()
    torch.manual_seed(7)
    before = torch.get_rng_state()
    dp = b._drop_path_scales(4, CPU)
    assert dp.shape == (3, 2, 4) and dp.dtype == torch.float32 and bool((dp == 1).all())
    assert not torch.equal(torch.get_rng_state(), before)


@pytest.mark.parametrize("make", [_beit, _plain], ids=["beit", "plain"])
def test_draw_values_and_cached_keep(make):
    tower = make(depth=3, drop_path_rate=0.1).train()
    probs = [blk.drop_path_prob for blk in tower.blocks]
    assert probs == pytest.approx([0.0, 0.05, 0.1])
    torch.manual_seed(7)
    dp = tower._drop_path_scales(512, CPU)
    assert dp.shape == (3, 2, 512)
    for i, prob in enumerate(probs):
        scale = 1.0 / (1.0 - torch.tensor(prob, dtype=torch.float32))
        assert bool(((dp[i] == 0) | (dp[i] == scale)).all())
    assert bool((dp[0] == 1).all()) and bool((dp[2] == 0).any()) and bool((dp[2] != 0).any())
    keep = tower._dp_keep
    torch.manual_seed(7)
    again = tower._drop_path_scales(512, CPU)
    assert tower._dp_keep is keep and torch.equal(again, dp)


@pytest.mark.parametrize("make", [_beit, _plain], ids=["beit", "plain"])
def test_eval_mode_draws_nothing(make):
    tower = make(depth=3, drop_path_rate=0.1).eval()
    torch.manual_seed(7)
    before = torch.get_rng_state()
    assert tower._drop_path_scales(4, CPU) is None
    assert torch.equal(torch.get_rng_state(), before)


# ---- the relative-position bias plan --------------------------------------------------------------
def _plan_want(N, need_grad, fused_bwd):
    """(transposed dense copy, forward tiles, backward tiles)"""
    if N in (65, 224):       # the batch-walking ViT-shape kernels: 64 < N <= 224
        return True, True, fused_bwd and need_grad
    if N == 257 and need_grad:   # the long route: N > 256 with a backward
        return False, True, True
    return True, False, False    # 64, 225, 256, and 257 without a backward


PLAN_CASES = [(N, g, f) for N in (64, 65, 224, 225, 256, 257) for g in (False, True) for f in (False, True)]


@pytest.mark.parametrize("N, need_grad, fused_bwd", PLAN_CASES)
def test_bias_plan(N, need_grad, fused_bwd):
    assert vit_trunk._bias_plan(N, need_grad, fused_bwd) == _plan_want(N, need_grad, fused_bwd)


@pytest.mark.parametrize("N, need_grad, fused_bwd", PLAN_CASES)
def test_block_bias_follows_the_plan(monkeypatch, N, need_grad, fused_bwd):
    calls = []

    def relpos_gather(table, index, H, n, ld, transposed):
        calls.append(("gather", table, index, H, n, ld, transposed))
        return ("dense", "dense_t") if transposed else "dense"

    def bias_tiles(dense, n, scale, fwd, bwd):
        calls.append(("tiles", dense, n, scale, fwd, bwd))
        return ("tiles",)

    monkeypatch.setattr(vit_trunk, "Fx", types.SimpleNamespace(relpos_gather=relpos_gather, bias_tiles=bias_tiles))
    monkeypatch.setattr(vit_trunk, "_VIT_FUSED_BWD", fused_bwd)
    tower = types.SimpleNamespace(_index32="index")
    blk = types.SimpleNamespace(attn=types.SimpleNamespace(relative_position_bias_table="table", scale=0.125))
    transposed, tiles_fwd, tiles_bwd = _plan_want(N, need_grad, fused_bwd)
    got = vit_trunk._block_bias(tower, blk, 12, N, 272, need_grad)
    assert got == ("dense", "dense_t" if transposed else None, ("tiles",) if tiles_fwd else None)
    want = [("gather", "table", "index", 12, N, 272, transposed)]
    if tiles_fwd:
        want.append(("tiles", "dense", N, 0.125, True, tiles_bwd))
    assert calls == want


# ---- the region glue switch stays beit2's ---------------------------------------------------------
def test_region_outputs_aten_branch(monkeypatch):
    def no_kernel(*a):
        raise AssertionError("the fused region kernel was asked for")

    monkeypatch.setattr(beit2, "REGION_GLUE_FUSED", False)
    monkeypatch.setattr(beit2._RegionPoolFn, "apply", no_kernel)
    torch.manual_seed(3)
    full = torch.randn(2, 5, 8).to(torch.bfloat16)
    idx = torch.tensor([1, 0, 1])
    atts = torch.tensor([[1, 1, 0, 1, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 1]])
    out = beit2.region_outputs(full, idx, atts)
    rows = full[idx][:, 1:].float()
    w = atts[:, 1:].float()
    cls = (w[:, :, None] * rows).sum(1) / w.sum(1, keepdim=True)
    assert out.dtype == torch.bfloat16 and out.shape == (3, 5, 8)
    assert torch.equal(out[:, 1:], full[idx][:, 1:])
    torch.testing.assert_close(out[:, 0].float(), cls.to(torch.bfloat16).float(), atol=0, rtol=2 ** -7)
