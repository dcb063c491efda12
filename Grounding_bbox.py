"""Referring-expression grounding fine-tune / evaluation task script on the HIP hot path: the `main()` of the reference's
Grounding_bbox.py:96-246 (argparse + YAML config -> XFMForGrounding, the four-group AdamW and the linear schedule, train / evaluate /
best-checkpoint epochs, the result files), started one process per GPU by run.py.  The loop itself is xfm_amd.grounding_loop.

What differs, on purpose: the dataset side (dataset/grounding_dataset.py, the tokenizer, the REFER tools, collect_tensor_result's
per-rank files and HDFS copy) is outside the hot-path scope, so the loaders here are synthetic (`synthetic: true`: formula images,
expression token ids, target boxes and ref tables with all three splits, xfm_amd.synthetic.grounding_batch / grounding_eval_batch /
grounding_refs); a caller with real loaders passes them to `xfm_amd.grounding_loop.train` / `evaluation` directly.  `--checkpoint` is
optional: without one the model starts from its random initialisation.  A non-empty `--output_hdfs` raises NotImplementedError.
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
    """`steps` batches (image, text, target_bbox) in the layout of Grounding_bbox.py:50's loader with token ids for strings, from a small
    pool of distinct formula batches."""

    def __init__(self, steps, batch_size, seed, image_res=384, max_tokens=40, pool=4):
        from xfm_amd import synthetic as syn
        super().__init__(steps, [syn.grounding_batch(batch_size, seed=s, image_res=image_res, max_tokens=max_tokens)
                                 for s in T.pool_seeds(seed, steps, pool)])


class SyntheticTestSet:
    """What evaluation() reads in place of the reference's REFER object: the three ref tables and `ref_index` (ref_id -> row)."""

    def __init__(self, num_refs, seed):
        from xfm_amd import synthetic as syn
        refs = syn.grounding_refs(num_refs, seed=seed)
        self.ref_box, self.ref_size, self.ref_split, self.ref_index = refs.ref_box, refs.ref_size, refs.ref_split, refs.ref_index


class SyntheticTestLoader(T.CycledBatches):
    """`steps` batches (image, text, ref_ids) in the layout of Grounding_bbox.py:81's loader; ref ids count up over the pass."""

    def __init__(self, steps, batch_size, seed, dataset, image_res=384, max_tokens=40, pool=2):
        from xfm_amd import synthetic as syn
        super().__init__(steps, [syn.grounding_eval_batch(batch_size, seed=s, image_res=image_res, max_tokens=max_tokens)
                                 for s in T.pool_seeds(seed, steps, pool)])
        self.batch_size, self.dataset = batch_size, dataset

    def __iter__(self):
        for i, (image, text, ref_ids) in enumerate(super().__iter__()):
            yield image, text, ref_ids + i * self.batch_size


def synthetic_loaders(config, seed, world_size=1):
    """(train_loader, test_loader) sized by `train_dataset_size` / `test_dataset_size` and the reference's batch_size."""
    if not config.get("synthetic", False):
        raise NotImplementedError("file-backed datasets (dataset/grounding_dataset.py, the tokenizer, the REFER tools) are outside the "
                                  "hot-path scope: set `synthetic: true` or drive xfm_amd.grounding_loop.train with your own loaders")
    kw = dict(image_res=config["image_res"], max_tokens=config.get("max_tokens", 40))
    n_train = max(math.ceil(config["train_dataset_size"] / (config["batch_size"] * world_size)), 1)   # Grounding_bbox.py:192
    n_test = max(config["test_dataset_size"] // config["batch_size"], 1)
    test_set = SyntheticTestSet(n_test * config["batch_size"], seed + 15485863)
    return (SyntheticTrainLoader(n_train, config["batch_size"], seed, **kw),
            SyntheticTestLoader(n_test, config["batch_size"], seed + 104729, test_set, **kw))


def main(args, config):
    from xfm_amd import grounding_loop as GL
    from xfm_amd import pretrain_loop as PL
    from xfm_amd.model_grounding import XFMForGrounding

    if len(args.output_hdfs):
        raise NotImplementedError("--output_hdfs (collect_tensor_result among nodes, Grounding_bbox.py:102-103) is not built: one node, "
                                  "local result files")
    rank, local_rank, world_size, device = T.start_process("Grounding_bbox.py")
    if args.bs > 0:
        config['batch_size'] = args.bs // world_size   # Grounding_bbox.py:105-106

    seed = args.seed + rank  # Grounding_bbox.py:108
    T.seed_all(seed)
    train_loader, test_loader = synthetic_loaders(config, seed, world_size)

    print("Creating model", flush=True)
    model = XFMForGrounding(config=config)
    if args.checkpoint and os.path.exists(args.checkpoint):
        model.load_pretrained(args.checkpoint, config, load_bbox_pretrain=args.load_bbox_pretrain, is_eval=args.evaluate)
    model = model.to(device)
    print("### Total Params: ", sum(p.numel() for p in model.parameters() if p.requires_grad), flush=True)

    arg_opt = T.AttrDict(config['optimizer'])
    optimizer = PL.create_optimizer(arg_opt, model)
    arg_sche = T.AttrDict(config['schedular'])
    arg_sche['step_per_epoch'] = len(train_loader)
    lr_scheduler = PL.create_scheduler(arg_sche, optimizer)
    # the reference's loop clips nothing (no clip call between backward and step, Grounding_bbox.py:58-60)
    accelerator = T.make_accelerator(config.get("accelerator"), seed)
    model, optimizer, lr_scheduler = accelerator.set_up(model, optimizer, lr_scheduler, local_rank, world_size, rank)

    start_time = time.time()
    print("### output_dir, ", args.output_dir, flush=True)
    if args.evaluate:
        print("Start evaluating", flush=True)
        grounding_acc = GL.evaluation(T.unwrap(model), test_loader, device, config, result_dir=args.result_dir,
                                      filename='grounding_bbox_eval')
        if rank == 0:
            print({**{f'{k}': v for k, v in grounding_acc.items()}}, flush=True)
    else:
        print("Start training", flush=True)
        if rank == 0:
            print(f"### data {config['train_dataset_size']}, batch size, {config['batch_size']} x {world_size}", flush=True)
        checkpointer = T.Checkpointer(args.output_dir)
        GL.train(model, train_loader, test_loader, optimizer, device, lr_scheduler, config, accelerator, checkpointer, args.output_dir,
                 args.result_dir, print_freq=config.get("print_freq", 50))
        torch.cuda.synchronize()
        if rank == 0:
            with open(os.path.join(args.output_dir, "log.txt")) as f:   # Grounding_bbox.py:242 `cat log.txt`
                print(f.read(), flush=True)
    print('### Time {:.1f} s'.format(time.time() - start_time), flush=True)
    T.finish_process(world_size)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--checkpoint", type=str, default="")
    parser.add_argument("--config", type=str, default="configs/Grounding_bbox_synthetic.yaml")
    parser.add_argument("--output_dir", type=str, default="output/refcoco_bbox")
    parser.add_argument("--output_hdfs", type=str, default="", help="to collect eval results among nodes (not built)")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=42, type=int)
    parser.add_argument("--evaluate", action="store_true")
    parser.add_argument("--load_bbox_pretrain", action="store_true")
    parser.add_argument("--bs", default=-1, type=int, help="for each gpu, batch_size = bs // num_gpus")
    a = parser.parse_args()
    cfg = T.load_yaml(a.config)
    a.result_dir = os.path.join(a.output_dir, "result")
    os.makedirs(a.output_dir, exist_ok=True)
    os.makedirs(a.result_dir, exist_ok=True)
    T.dump_yaml(cfg, a.output_dir)
    main(a, cfg)
