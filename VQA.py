"""VQA fine-tune / evaluation task script on the HIP hot path: the `main()` of the reference's VQA.py:125-273 (argparse + YAML config ->
XFMForVQA, the four-group AdamW and the linear schedule, train / checkpoint / evaluate epochs, result files), started one process per
GPU by run.py.  The loop itself is xfm_amd.vqa_loop.

What differs, on purpose: the dataset side (dataset/vqa_dataset.py, the tokenizer, collect_result's multi-node gather) is outside the
hot-path scope, so the loaders here are synthetic (`synthetic: true`: formula images, question / answer token ids and a candidate answer
list in which several candidates share a first token, xfm_amd.synthetic.vqa_batch / vqa_eval_batch / vqa_answer_list); a caller with real
loaders passes them to `xfm_amd.vqa_loop.train` / `evaluation` directly.  `--checkpoint` is optional: without one the model starts from
its random initialisation.
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from xfm_amd import task as T  # noqa: E402


class SyntheticTrainLoader(T.CycledBatches):
    """`steps` batches (image, question, answer, weights, n) in the layout of VQA.py:46's loader with token ids for strings, from a small
    pool of distinct formula batches."""

    def __init__(self, steps, batch_size, seed, image_res=480, max_tokens=40, max_answers=10, answer_len=8, pool=4):
        from xfm_amd import synthetic as syn
        batches = []
        for s in T.pool_seeds(seed, steps, pool):
            x = syn.vqa_batch(batch_size, seed=s, image_res=image_res, max_tokens=max_tokens, max_answers=max_answers,
                              answer_len=answer_len)
            batches.append((x.image, (x.q_ids, x.q_atts), (x.a_ids, x.a_atts), x.weights, x.k))
        super().__init__(steps, batches)


class SyntheticTestSet:
    """What evaluation() and calculate_acc() read of the reference's vqa_test_dataset: `answer_list`, its token ids `answer_input`, and
    `ann` (no answers: a test split, so calculate_acc returns without a figure, VQA.py:105-109)."""

    def __init__(self, num_questions, num_answers, seed, answer_len=8):
        from xfm_amd import synthetic as syn
        ids, atts, names = syn.vqa_answer_list(num_answers, seed=seed, answer_len=answer_len)
        self.answer_list, self.answer_input = names, (ids, atts)
        self.ann = [{"question_id": q} for q in range(num_questions)]


class SyntheticTestLoader(T.CycledBatches):
    """`steps` batches (image, question, question_id) in the layout of VQA.py:89's loader; question ids count up over the pass."""

    def __init__(self, steps, batch_size, seed, dataset, image_res=480, max_tokens=40, pool=2):
        from xfm_amd import synthetic as syn
        super().__init__(steps, [syn.vqa_eval_batch(batch_size, seed=s, image_res=image_res, max_tokens=max_tokens)
                                 for s in T.pool_seeds(seed, steps, pool)])
        self.batch_size, self.dataset = batch_size, dataset

    def __iter__(self):
        for i, (image, question, qid) in enumerate(super().__iter__()):
            yield image, question, qid + i * self.batch_size


def synthetic_loaders(config, seed, world_size=1):
    """(train_loader, test_loader) sized by `train_dataset_size` / `test_dataset_size` and the reference's batch_size_train / _test."""
    if not config.get("synthetic", False):
        raise NotImplementedError("file-backed datasets (dataset/vqa_dataset.py, the tokenizer) are outside the hot-path scope: set "
                                  "`synthetic: true` or drive xfm_amd.vqa_loop.train with your own loaders")
    kw = dict(image_res=config["image_res"], max_tokens=config.get("max_tokens", 40))
    n_train = max(math.ceil(config["train_dataset_size"] / (config["batch_size_train"] * world_size)), 1)   # VQA.py:219
    n_test = max(config["test_dataset_size"] // config["batch_size_test"], 1)
    test_set = SyntheticTestSet(n_test * config["batch_size_test"], config["answer_list_size"], seed + 15485863,
                                answer_len=config.get("answer_len", 8))
    return (SyntheticTrainLoader(n_train, config["batch_size_train"], seed, max_answers=config.get("max_answers", 10),
                                 answer_len=config.get("answer_len", 8), **kw),
            SyntheticTestLoader(n_test, config["batch_size_test"], seed + 104729, test_set, **kw))


def main(args, config):
    from xfm_amd import pretrain_loop as PL
    from xfm_amd import vqa_loop as VL
    from xfm_amd.model_generation import XFMForVQA

    rank, local_rank, world_size, device = T.start_process("VQA.py")
    if args.bs > 0:
        config['batch_size_train'] = args.bs // world_size   # VQA.py:134-135

    seed = args.seed + rank  # VQA.py:137
    T.seed_all(seed)
    train_loader, test_loader = synthetic_loaders(config, seed, world_size)

    print("Creating model", flush=True)
    config.setdefault('pad_token_id', 1)   # VQA.py:154 takes it from the tokenizer; <pad> = 1 in the RoBERTa vocabulary
    model = XFMForVQA(config=config)
    if args.checkpoint and os.path.exists(args.checkpoint):
        model.load_pretrained(args.checkpoint, config, is_eval=args.evaluate or config.get('load_vqa_pretrain', False))
    model = model.to(device)
    print("### Total Params: ", sum(p.numel() for p in model.parameters() if p.requires_grad), flush=True)

    arg_opt = T.AttrDict(config['optimizer'])
    optimizer = PL.create_optimizer(arg_opt, model)
    arg_sche = T.AttrDict(config['schedular'])
    arg_sche['step_per_epoch'] = len(train_loader)
    lr_scheduler = PL.create_scheduler(arg_sche, optimizer)
    # the reference's loop clips nothing (no clip call between backward and step, VQA.py:56-60)
    accelerator = T.make_accelerator(config.get("accelerator"), seed)
    model, optimizer, lr_scheduler = accelerator.set_up(model, optimizer, lr_scheduler, local_rank, world_size, rank)

    start_time = time.time()
    print("### output_dir, ", args.output_dir, flush=True)
    if args.evaluate:
        print("Start evaluating", flush=True)
        vqa_result = VL.evaluation(model, test_loader, device, config)
        if rank == 0:
            result_rpath = VL.save_result(vqa_result, args.result_dir, 'vqa_eval')
            VL.calculate_acc(result_rpath, test_loader.dataset)
            print("### result file, ", result_rpath, flush=True)
    else:
        print("Start training", flush=True)
        if rank == 0:
            print(f"### data {config['train_dataset_size']}, batch size, {config['batch_size_train']} x {world_size} x "
                  f"{config.get('accumulate_steps', 1)}", flush=True)
        checkpointer = T.Checkpointer(args.output_dir)
        results = VL.train(model, train_loader, test_loader, optimizer, device, lr_scheduler, config, accelerator, checkpointer,
                           args.output_dir, args.result_dir, print_freq=config.get("print_freq", 50))
        torch.cuda.synchronize()
        if rank == 0:
            with open(os.path.join(args.output_dir, "log.txt")) as f:   # VQA.py:269 `cat log.txt`
                print(f.read(), end="", flush=True)
            print("### result files, ", results, flush=True)
    print('### Time {:.1f} s'.format(time.time() - start_time), flush=True)
    T.finish_process(world_size)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--checkpoint", type=str, default="")
    parser.add_argument("--config", required=True)
    parser.add_argument("--output_dir", default="output/vqa")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=42, type=int)
    parser.add_argument("--bs", default=-1, type=int)
    parser.add_argument("--evaluate", action="store_true")
    parser.add_argument("--load_vqa_pretrain", action="store_true")
    a = parser.parse_args()
    cfg = T.load_yaml(a.config)
    a.result_dir = os.path.join(a.output_dir, "result")
    os.makedirs(a.output_dir, exist_ok=True)
    os.makedirs(a.result_dir, exist_ok=True)
    T.dump_yaml(cfg, a.output_dir)
    main(a, cfg)
