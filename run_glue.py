"""GLUE fine-tune task script on the HIP hot path: the `main()` of the reference's run_glue.py:97-421 (argparse + YAML config ->
XFMForClassification on the text tower, AdamW in two groups, get_scheduler, train / evaluate epochs with the glue metric, checkpoints),
started one process per GPU by run.py.  The loop itself is xfm_amd.glue_loop.

What differs, on purpose: the dataset side (`datasets.load_dataset`, the tokenizer, DataCollatorWithPadding) is outside the hot-path
scope, so the loaders here are synthetic (`synthetic: true`: formula token ids padded to the batch's longest and formula labels,
xfm_amd.synthetic.glue_batch); a caller with real loaders passes them to `xfm_amd.glue_loop.train` directly.  HF
AutoModelForSequenceClassification (`use_huggingface_models: true`) is not built.  Without a `vision_config` the (unused) vision tower
starts from a random-init checkpoint written next to the outputs (the model always loads its tower from a file, xfm.py:230-232).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from Imagenet import random_vision_checkpoint  # noqa: E402
from xfm_amd import task as T  # noqa: E402


class SyntheticLoader(T.CycledBatches):
    """`steps` batches (input_ids, attention_mask, labels) of run_glue.py:285-288's loaders, from a small pool of distinct formula
    batches, each padded to its own longest sequence."""

    def __init__(self, steps, batch_size, seed, max_length=128, num_labels=2, vocab=None, pool=4):
        from xfm_amd import synthetic as syn
        kw = {} if vocab is None else {"vocab": vocab}
        super().__init__(steps, [syn.glue_batch(batch_size, seed=s, max_length=max_length, num_labels=num_labels, **kw)
                                 for s in T.pool_seeds(seed, steps, pool)])


def synthetic_loaders(config, seed, world_size=1):
    """(train_loader, eval_loader, mismatched_loader or None) sized by `train_dataset_size` / `val_dataset_size` and the reference's
    per_device_train_batch_size / per_device_eval_batch_size; mnli gets the second validation loader (run_glue.py:396-402)."""
    if not config.get("synthetic", False):
        raise NotImplementedError("file-backed datasets (run_glue.py:138-152 load_dataset, the tokenizer, :246-288) are outside the "
                                  "hot-path scope: set `synthetic: true` or drive xfm_amd.glue_loop.train with your own loaders")
    from xfm_amd.glue_loop import task_num_labels
    kw = dict(max_length=config["max_length"], num_labels=task_num_labels(config["task_name"]),
              vocab=(config.get("text_config") or {}).get("vocab_size"))
    n_train = max(config["train_dataset_size"] // (config["per_device_train_batch_size"] * world_size), 1)
    n_val = max(config["val_dataset_size"] // config["per_device_eval_batch_size"], 1)
    train = SyntheticLoader(n_train, config["per_device_train_batch_size"], seed, **kw)
    val = SyntheticLoader(n_val, config["per_device_eval_batch_size"], seed + 104729, **kw)
    mm = SyntheticLoader(n_val, config["per_device_eval_batch_size"], seed + 15485863, **kw) if config["task_name"] == "mnli" else None
    return train, val, mm


def main(args, config):
    from xfm_amd import glue_loop as GL
    from xfm_amd.model_classification import XFMForClassification

    rank, local_rank, world_size, device = T.start_process("run_glue.py")
    seed = args.seed + rank
    T.seed_all(seed)   # run_glue.py:123-124
    if config.get("use_huggingface_models", False):
        raise NotImplementedError("use_huggingface_models: true (run_glue.py:180-187 AutoModelForSequenceClassification) is not built")
    config["num_labels"] = GL.task_num_labels(config["task_name"])   # run_glue.py:157-163, :198
    train_loader, eval_loader, mm_loader = synthetic_loaders(config, seed, world_size)

    print("Creating model XFM for classification", flush=True)
    if not config.get("vision_config"):
        if rank == 0:
            random_vision_checkpoint(config, args.output_dir)
        if world_size > 1:
            dist.barrier()
        config["vision_config"] = os.path.join(args.output_dir, "config_beit2_random_init.json")
    model = XFMForClassification(config=config)
    if args.checkpoint and os.path.exists(args.checkpoint):
        model.load_pretrained(args.checkpoint, config)
    model = model.to(device)
    optimizer = GL.create_optimizer(config, model)
    lr_scheduler = GL.create_scheduler(config, optimizer, len(train_loader))
    # the reference's loop clips nothing (no clip call between backward and step, run_glue.py:359-361); accumulation is the loop's own
    accelerator = T.make_accelerator(config.get("accelerator"), seed)
    model, optimizer, lr_scheduler = accelerator.set_up(model, optimizer, lr_scheduler, local_rank, world_size, rank)

    def log(epoch, i, avg):
        if rank == 0:
            print(json.dumps({"epoch": epoch, "iter": i, **{k: round(v, 8) for k, v in avg.items()}}), flush=True)

    start_time = time.time()
    if args.evaluate:
        res = GL.evaluate(model, eval_loader, device, config)
        print(json.dumps({**res, "count": res.count}), flush=True)
    else:
        print("***** Running training *****", flush=True)
        if rank == 0:
            print(f"  Num Epochs = {config['num_train_epochs']}, batch {config['per_device_train_batch_size']} x {world_size} x "
                  f"{config['gradient_accumulation_steps']}, total optimization steps = {config['max_train_steps']}", flush=True)
        checkpointer = T.Checkpointer(args.output_dir)
        GL.train(model, train_loader, eval_loader, optimizer, lr_scheduler, device, config, accelerator, checkpointer, args.output_dir,
                 mismatched_loader=mm_loader, print_freq=config.get("print_freq", 50), log=log)
        torch.cuda.synchronize()
        if rank == 0:
            print("Training time {:.1f} s".format(time.time() - start_time), flush=True)
    T.finish_process(world_size)


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Finetune XFM on a GLUE text classification task")
    parser.add_argument("--config", required=True)
    parser.add_argument("--output_dir", default="output/glue")
    parser.add_argument("--checkpoint", default="")
    parser.add_argument("--evaluate", action="store_true")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=42, type=int)
    a = parser.parse_args()
    cfg = T.load_yaml(a.config)
    os.makedirs(a.output_dir, exist_ok=True)
    T.dump_yaml(cfg, a.output_dir)
    main(a, cfg)
