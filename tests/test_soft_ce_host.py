"""Host side of the soft-target CE / Mixup feature (no GPU): Mixup's parameter draw under a seeded numpy.random, and the no-fallback rule
(tests/test_capi.py) for the new functional wrappers."""
import numpy as np
import pytest
import torch

H, W = 32, 40


def _mix(**kw):
    from xfm_amd.mixup import Mixup
    return Mixup(**{**dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=10), **kw})


def _is_cut(box):
    return (box[:, 1] > box[:, 0]) & (box[:, 3] > box[:, 2])


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_draw_ranges_boxes_and_corrected_lam(mode):
    np.random.seed(0)
    mix = _mix(mode=mode)
    seen_cut = seen_mix = 0
    for _ in range(50):
        lam, box = mix.draw(6, H, W)
        assert lam.shape == (6,) and lam.dtype == np.float32 and box.shape == (6, 4) and box.dtype == np.int32
        assert np.all((lam >= 0) & (lam <= 1))
        if mode == "batch":
            assert np.all(lam == lam[0]) and np.all(box == box[0])
        cut = _is_cut(box)
        assert np.all(box[~cut] == 0)   # mixup rows carry the empty box
        yl, yh, xl, xh = box[cut].T
        assert np.all((0 <= yl) & (yl < yh) & (yh <= H) & (0 <= xl) & (xl < xh) & (xh <= W))   # inside the image
        area = (yh - yl) * (xh - xl)
        assert np.array_equal(lam[cut], (1.0 - area / float(H * W)).astype(np.float32))   # correct_lam
        seen_cut += int(cut.sum())
        seen_mix += int((~cut).sum())
    assert seen_cut > 0 and seen_mix > 0


def test_draw_switch_and_mix_probabilities():
    np.random.seed(1)
    for _ in range(20):
        lam, box = _mix(switch_prob=0.0).draw(4, H, W)
        assert not _is_cut(box).any()   # always mixup
        lam, box = _mix(switch_prob=1.0).draw(4, H, W)
        assert np.all(_is_cut(box) | (lam == 1.0))   # always CutMix (a box of no area is the identity)
        lam, box = _mix(prob=0.0, mode="elem").draw(4, H, W)
        assert np.all(lam == 1.0) and np.all(box == 0)
        lam, box = _mix(mixup_alpha=0.0).draw(4, H, W)   # only the CutMix alpha is set
        assert np.all(_is_cut(box) | (lam == 1.0))
        lam, box = _mix(cutmix_alpha=0.0).draw(4, H, W)
        assert not _is_cut(box).any()


def test_uncorrected_lam_is_the_beta_draw():
    np.random.seed(5)
    state = np.random.get_state()
    lam, box = _mix(switch_prob=1.0, correct_lam=False).draw(2, H, W)
    np.random.set_state(state)
    np.random.rand(), np.random.rand()   # the mix and the switch draw
    assert lam[0] == np.float32(np.random.beta(1.0, 1.0))


def test_unbuilt_modes_raise():
    from xfm_amd.mixup import Mixup
    with pytest.raises(NotImplementedError, match="pair"):
        Mixup(mode="pair")
    with pytest.raises(NotImplementedError, match="cutmix_minmax"):
        Mixup(cutmix_minmax=(0.2, 0.8))
    with pytest.raises(AssertionError):   # odd batch, as timm asserts (before anything touches the device)
        Mixup()(torch.zeros(3, 3, 8, 8), torch.zeros(3, dtype=torch.int64))


def test_new_wrappers_refuse_cpu_tensors():
    from xfm_amd import _lib, functional as Fx
    from xfm_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    x, y = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    lam, box, lse = torch.ones(4), torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4)
    for call in (lambda: Fx.ce_smooth_fwd(x, 8, y, 0.9, 0.0125), lambda: Fx.ce_smooth_bwd(x, 8, y, 0.9, 0.0125, lse, torch.ones(1), 8),
                 lambda: Fx.ce_soft_fwd(x, 8, x), lambda: Fx.ce_soft_bwd(x, 8, x, lse, lse, torch.ones(1), 8),
                 lambda: Fx.mixup_(torch.zeros(4, 3, 8, 8), lam, box), lambda: Fx.mixup_target(y, lam, 10, 0.1),
                 lambda: SoftTargetCrossEntropy()(x, x), lambda: LabelSmoothingCrossEntropy(0.1)(x, y)):
        with pytest.raises(_lib.XfmHipError):
            call()


def test_lm_head_models_accept_label_smoothing():
    """The constructors take the keyword (xbert.py:1240; model_generation.py:275) and build the reference's parameter set."""
    from xfm_amd.xbert import BertConfig, BertLMHeadModel
    from xfm_amd.xroberta import RobertaConfig, RobertaForCausalLM
    a = BertLMHeadModel(BertConfig(num_hidden_layers=1, fusion_layer=0, encoder_width=768), label_smoothing=0.1)
    b = BertLMHeadModel(BertConfig(num_hidden_layers=1, fusion_layer=0, encoder_width=768))
    assert a.label_smoothing == 0.1 and sorted(a.state_dict()) == sorted(b.state_dict())
    c = RobertaForCausalLM(RobertaConfig(num_hidden_layers=1, fusion_layer=0, encoder_width=768), label_smoothing=0.1)
    d = RobertaForCausalLM(RobertaConfig(num_hidden_layers=1, fusion_layer=0, encoder_width=768))
    assert c.label_smoothing == 0.1 and d.label_smoothing == 0.0 and sorted(c.state_dict()) == sorted(d.state_dict())
