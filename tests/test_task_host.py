"""xfm_amd.task -- what the three task scripts and their loops share -- without a GPU: the cycled batch pool and the five synthetic
loaders built on it, the upload / rank / wrapper helpers, the process start-up check and the accelerator block.  Small image sizes: the
loaders' contents are compared with direct calls of the generators, not run."""
import pytest
import torch

from xfm_amd import synthetic as syn
from xfm_amd import task as T


def test_cycled_batches_length_cycling_and_pool_size():
    loader = T.CycledBatches(5, ["a", "b"])
    assert len(loader) == 5 and list(loader) == ["a", "b", "a", "b", "a"]
    assert list(loader) == list(loader)   # a fresh pass every time
    assert T.pool_seeds(10, 5, 2) == [10, 10 + 7919]
    assert T.pool_seeds(10, 3, 4) == [10, 10 + 7919, 10 + 2 * 7919]   # a pool larger than the pass builds only `steps` batches
    import Imagenet
    short = Imagenet.SyntheticLoader(2, 3, seed=1, image_res=16, num_labels=5, pool=4)
    assert len(short) == 2 and len(short.batches) == 2


def _same(got, want):
    """Two batches position by position: tensors torch.equal, (ids, mask) pairs entry by entry, host lists equal."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if torch.is_tensor(w):
            assert torch.equal(g, w)
        elif isinstance(w, tuple):
            _same(g, w)
        else:
            assert g == w


def _check(loader, steps, pool, direct):
    assert len(loader) == steps and len(loader.batches) == min(pool, steps)
    batches = list(loader)
    assert len(batches) == steps
    for i, got in enumerate(batches):
        _same(got, direct(i % pool))


def test_pretrain_loaders_yield_the_generators_batches():
    import Pretrain
    seed, res, V = 11, 32, 2048
    text = ("text_ids", "text_atts", "text_ids_masked", "masked_pos", "masked_ids")

    def image_batch(k, with_image=True):
        b = syn.pretrain_batch(3, seed=seed + 7919 * k, image_res=res, max_tokens=12, max_masks=4, with_image=with_image, vocab=V)
        return ((b["image"],) if with_image else ()) + tuple(b[n] for n in text)

    _check(Pretrain.SyntheticLoader(5, 3, seed, image_res=res, max_tokens=12, max_masks=4, vocab=V), 5, 4, image_batch)
    _check(Pretrain.SyntheticLoader(3, 3, seed, image_res=res, max_tokens=12, max_masks=4, vocab=V, with_image=False, pool=2), 3, 2,
           lambda k: image_batch(k, with_image=False))
    regions = {"batch_size": 6, "max_images": 4, "max_regions": 2}
    _check(Pretrain.SyntheticRegionLoader(5, regions, seed, image_res=res, patch_size=16, max_tokens=12, max_masks=4, vocab=V), 5, 4,
           lambda k: syn.region_batch(6, 4, 2, seed=seed + 7919 * k, image_res=res, patch_size=16, max_tokens=12, max_masks=4, vocab=V))


def test_imagenet_loaders_yield_the_generators_batches():
    import Imagenet
    cfg = {"synthetic": True, "image_res": 16, "num_labels": 7, "batch_size_train": 3, "batch_size_test": 4, "train_dataset_size": 16,
           "val_dataset_size": 8}
    train, val = Imagenet.synthetic_loaders(cfg, seed=5)
    _check(train, 5, 4, lambda k: syn.imagenet_batch(3, seed=5 + 7919 * k, image_res=16, num_labels=7))          # 16 // 3: floor
    _check(val, 2, 4, lambda k: syn.imagenet_batch(4, seed=5 + 104729 + 7919 * k, image_res=16, num_labels=7))


def test_vqa_loaders_yield_the_generators_batches_and_count_the_question_ids():
    import VQA
    cfg = {"synthetic": True, "image_res": 32, "max_tokens": 12, "max_answers": 3, "answer_len": 5, "batch_size_train": 3,
           "batch_size_test": 4, "train_dataset_size": 14, "test_dataset_size": 12, "answer_list_size": 10}
    train, test = VQA.synthetic_loaders(cfg, seed=9)

    def train_batch(k):
        x = syn.vqa_batch(3, seed=9 + 7919 * k, image_res=32, max_tokens=12, max_answers=3, answer_len=5)
        return x.image, (x.q_ids, x.q_atts), (x.a_ids, x.a_atts), x.weights, x.k

    _check(train, 5, 4, train_batch)   # ceil(14 / 3)
    assert len(test) == 3 and len(test.batches) == 2 and test.batch_size == 4
    for i, (image, question, qid) in enumerate(test):
        want = syn.vqa_eval_batch(4, seed=9 + 104729 + 7919 * (i % 2), image_res=32, max_tokens=12)
        _same((image, question), want[:2])
        assert qid.tolist() == list(range(4 * i, 4 * i + 4))
    assert [int(q) for _, _, qid in test for q in qid] == list(range(3 * 4))   # 0 .. steps * batch_size - 1, on every pass
    ids, atts, names = syn.vqa_answer_list(10, seed=9 + 15485863, answer_len=5)
    assert test.dataset.answer_list == names and torch.equal(test.dataset.answer_input[0], ids)
    assert torch.equal(test.dataset.answer_input[1], atts) and len(test.dataset.ann) == 12


def test_to_device_and_read():
    assert T.to_device("cpu", None) is None
    t = torch.arange(6).view(2, 3)
    got = T.to_device("cpu", t)
    assert torch.is_tensor(got) and torch.equal(got, t)
    pair = T.to_device("cpu", (t, t + 1))
    assert isinstance(pair, tuple) and len(pair) == 2 and torch.equal(pair[0], t) and torch.equal(pair[1], t + 1)
    assert T.read(t) == [[0, 1, 2], [3, 4, 5]]


def test_rank_and_wrapper_helpers_without_a_process_group():
    assert not T.is_distributed() and T.is_main_process()
    inner = torch.nn.Linear(2, 2)

    class Wrapper:
        module = inner

    assert T.unwrap(Wrapper()) is inner and T.unwrap(inner) is inner


def test_start_process_refuses_to_run_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="X.py needs a GPU: the HIP path has no CPU fallback"):
        T.start_process("X.py")


def test_make_accelerator_default_and_given_section(monkeypatch):
    from xfm_amd import accelerators
    seen = []
    monkeypatch.setattr(accelerators, "ACCELERATOR_MAP", {"RCCLDDP": lambda args, logger: seen.append((args, logger)) or "rccl",
                                                          "Other": lambda args, logger: seen.append((args, logger)) or "other"})
    assert T.make_accelerator(None, 7) == "rccl" and T.make_accelerator({}, 8) == "rccl"
    assert seen[0] == ({"ACCELERATOR": "RCCLDDP", "RNG_SEED": 7, "GRAD_ACCUMULATE_STEPS": 1, "CLIP_GRAD_NORM": 0.0}, None)
    assert seen[1][0]["RNG_SEED"] == 8 and isinstance(seen[0][0], T.AttrDict) and seen[0][0].CLIP_GRAD_NORM == 0.0
    section = {"ACCELERATOR": "Other", "RNG_SEED": 42, "GRAD_ACCUMULATE_STEPS": 1, "CLIP_GRAD_NORM": 1.0, "SYNCBN": False}
    assert T.make_accelerator(section, 7) == "other"
    assert seen[2] == (section, None)   # passed through untouched: the seed argument is the default's only


def test_the_pretrain_loop_re_exports_the_moved_classes():
    from xfm_amd import pretrain_loop as PL
    from xfm_amd.pretrain_loop import AttrDict, LossMeters, create_optimizer  # noqa: F401  (the import the benchmark and the tools use)
    assert PL.LossMeters is T.LossMeters and PL.AttrDict is T.AttrDict
    from xfm_amd import imagenet_loop as IL
    from xfm_amd import vqa_loop as VL
    assert IL._read is T.read and VL._read is T.read


def test_yaml_round_trip(tmp_path):
    cfg = {"schedular": {"epochs": 2, "lr": 1e-4}, "synthetic": True, "train_file": []}
    T.dump_yaml(cfg, str(tmp_path))
    assert T.load_yaml(str(tmp_path / "config.yaml")) == cfg
