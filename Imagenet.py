"""ImageNet fine-tune / linear-probe task script on the HIP hot path: the `main()` of the reference's Imagenet.py:539-645 (argparse +
YAML config -> XFMForClassification, torch.optim.AdamW, Mixup, criterion, train / evaluate epochs, checkpoint_best.pth), started one
process per GPU by run.py.  The loop itself is xfm_amd.imagenet_loop.

What differs, on purpose: the dataset side (ImageFolder / torchvision datasets, timm's create_transform, RandAugment) is outside the
hot-path scope, so the loaders here are synthetic (`synthetic: true`: formula images and labels, xfm_amd.synthetic.imagenet_batch); a
caller with real loaders passes them to `xfm_amd.imagenet_loop.train` directly.  Without a `vision_config` the vision tower starts from
a random-init checkpoint written next to the outputs (the model always loads its tower from a file, xfm.py:230-232).
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

from xfm_amd import task as T  # noqa: E402

# Imagenet.py:84-106
DATASET2NLABELS = {'imagenet': 1000, 'food101': 101, 'cifar10': 10, 'cifar100': 100, 'stanfordcars': 196, 'fgvcaircraft': 102, 'dtd': 47,
                   'oxfordiiitpet': 37, 'flowers102': 103, 'mnist': 10, 'stl10': 10, 'sun397': 397, 'caltech101': 101, 'caltech256': 256,
                   'gtsrb': 43, 'country211': 211, 'fer2013': 7, 'pcam': 2, 'kitti': 9, 'renderedsst2': 2}


class SyntheticLoader(T.CycledBatches):
    """`steps` batches of (images, labels) in the layout of Imagenet.py:453's loader, from a small pool of distinct formula batches."""

    def __init__(self, steps, batch_size, seed, image_res=224, num_labels=1000, pool=4):
        from xfm_amd import synthetic as syn
        super().__init__(steps, [syn.imagenet_batch(batch_size, seed=s, image_res=image_res, num_labels=num_labels)
                                 for s in T.pool_seeds(seed, steps, pool)])


def synthetic_loaders(config, seed, world_size=1):
    """(train_loader, val_loader) sized by `train_dataset_size` / `val_dataset_size` and the reference's batch_size_train / _test."""
    if not config.get("synthetic", False):
        raise NotImplementedError("file-backed datasets (Imagenet.py:298-434 gen_loader / gen_loader_others) are outside the hot-path "
                                  "scope: set `synthetic: true` or drive xfm_amd.imagenet_loop.train with your own loaders")
    kw = dict(image_res=config["image_res"], num_labels=config["num_labels"])
    n_train = max(config["train_dataset_size"] // (config["batch_size_train"] * world_size), 1)
    n_val = max(config["val_dataset_size"] // config["batch_size_test"], 1)
    return (SyntheticLoader(n_train, config["batch_size_train"], seed, **kw),
            SyntheticLoader(n_val, config["batch_size_test"], seed + 104729, **kw))


def random_vision_checkpoint(config, out_dir):
    """A random-init BEiT-v2 checkpoint + the vision_config JSON that names it (what `vision_config` points at in a real run)."""
    from xfm_amd.beit2 import VisionTransformer
    v = VisionTransformer(img_size=config["image_res"], depth=config.get("vision_depth", 12), drop_path_rate=0.1)
    sd = dict(v.state_dict())
    sd["head.weight"], sd["head.bias"] = torch.zeros(1000, 768), torch.zeros(1000)   # dropped by load_pretrained_beit2
    torch.save({"model": sd}, os.path.join(out_dir, "beit_random_init.pth"))
    path = os.path.join(out_dir, "config_beit2_random_init.json")
    with open(path, "w") as f:
        json.dump({"ckpt": os.path.join(out_dir, "beit_random_init.pth"), "vision_width": 768, "patch_size": config["patch_size"]}, f)
    return path


def main(args, config):
    from xfm_amd import imagenet_loop as IL
    from xfm_amd.model_classification import XFMForClassification

    rank, local_rank, world_size, device = T.start_process("Imagenet.py")
    seed = args.seed + rank  # Imagenet.py:544
    T.seed_all(seed)
    if not config.get("synthetic", False) or "num_labels" not in config:
        config["num_labels"] = DATASET2NLABELS[config["task_name"]]  # Imagenet.py:550 (a synthetic config may name a smaller label set)
    train_loader, val_loader = synthetic_loaders(config, seed, world_size)

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
    print("config['optimizer']", config["optimizer"], flush=True)
    optimizer = IL.create_optimizer(config, model)
    # the reference's loop clips nothing (no clip call between backward and step, Imagenet.py:483-485)
    accelerator = T.make_accelerator(config.get("accelerator"), seed)
    model, optimizer, _ = accelerator.set_up(model, optimizer, None, local_rank, world_size, rank)

    mixup_fn = IL.create_mixup(config)
    if mixup_fn is not None:
        print("Mixup is activated!", flush=True)
    criterion = IL.create_criterion(config, mixup_fn)
    print("criterion = %s" % str(criterion), flush=True)

    def log(epoch, i, avg):
        if rank == 0:
            print(json.dumps({"epoch": epoch, "iter": i, **{k: round(v, 8) for k, v in avg.items()}}), flush=True)

    start_time = time.time()
    if args.evaluate:
        acc1 = IL.evaluate(model, val_loader, device)
        print(json.dumps({"acc1": float(acc1), "acc2": acc1.acc2, "loss": acc1.loss_avg}), flush=True)
    else:
        print("Start training", flush=True)
        best_acc1, best_epoch = IL.train(model, train_loader, val_loader, optimizer, criterion, mixup_fn, device, config, accelerator,
                                         args.output_dir, print_freq=config.get("print_freq", 50), log=log)
        torch.cuda.synchronize()
        if rank == 0:
            with open(os.path.join(args.output_dir, "log.txt"), "a") as f:
                f.write("best epoch: %d" % best_epoch)   # Imagenet.py:643-645
            print("Training time {:.1f} s, best_acc1 {:.3f}".format(time.time() - start_time, best_acc1), flush=True)
    T.finish_process(world_size)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", required=True)
    parser.add_argument("--output_dir", default="output/imagenet")
    parser.add_argument("--checkpoint", default="")
    parser.add_argument("--evaluate", action="store_true")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=42, type=int)
    a = parser.parse_args()
    cfg = T.load_yaml(a.config)
    os.makedirs(a.output_dir, exist_ok=True)
    T.dump_yaml(cfg, a.output_dir)
    main(a, cfg)
