"""What the task scripts (Pretrain.py, Imagenet.py, VQA.py) and their loops (pretrain_loop, imagenet_loop, vqa_loop) share: process
start-up and teardown, seeding, the accelerator block, the cycled synthetic-batch pool, the checkpointer, the loss meters and the small
rank / wrapper / upload helpers.  Plain Python, no device code; what differs between the tasks because the reference differs stays in
the task's own files."""
import os
import random
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist
import yaml


class AttrDict(dict):
    """utils.AttrDict: the reference's configs are dicts read both as args['k'] and args.k."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


class LossMeters:
    """Running means of the per-source losses without a device sync per update: tensors are parked and read in one go."""

    def __init__(self):
        self.pending = []
        self.total = OrderedDict()
        self.count = OrderedDict()

    def update(self, **kw):
        for k, v in kw.items():
            self.pending.append((k, v.detach() if torch.is_tensor(v) else v))

    def flush(self):
        for k, v in self.pending:
            self.total[k] = self.total.get(k, 0.0) + float(v)
            self.count[k] = self.count.get(k, 0) + 1
        self.pending = []

    def global_avg(self):
        self.flush()
        return {k: self.total[k] / self.count[k] for k in self.total}


class Checkpointer:
    """utils/checkpointer.py:20-47, local paths only."""

    def __init__(self, serialization_dir=".output"):
        self._dir = serialization_dir
        os.makedirs(self._dir, exist_ok=True)

    def save_checkpoint(self, epoch, model_state, training_states, step=-1):
        if step > 0:
            torch.save(model_state, os.path.join(self._dir, "model_state_step_{}.th".format(step)))
        else:
            torch.save(model_state, os.path.join(self._dir, "model_state_epoch_{}.th".format(epoch)))
            torch.save({**training_states, "epoch": epoch}, os.path.join(self._dir, "training_state_latest.th"))


def is_distributed():
    return dist.is_available() and dist.is_initialized()


def is_main_process():
    """utils.is_main_process()."""
    return not is_distributed() or dist.get_rank() == 0


def unwrap(model):
    """The model behind a DDP-style wrapper (`model_without_ddp`)."""
    return model.module if hasattr(model, 'module') else model


def to_device(device, x):
    """None stays None, a tensor is copied with non_blocking=True, an (input_ids, attention_mask) tuple becomes a tuple of copies."""
    if x is None:
        return None
    if isinstance(x, (tuple, list)):
        return tuple(to_device(device, t) for t in x)
    return x.to(device, non_blocking=True)


def read(t):
    """The loops' single device-to-host read helper (an evaluation pass calls it once; the tests count its calls)."""
    return t.tolist()


def pool_seeds(seed, steps, pool):
    """Seeds of a small pool of distinct batches (host generation is not what is being run)."""
    return [seed + 7919 * k for k in range(min(pool, steps))]


class CycledBatches:
    """A loader of `steps` batches that cycles through the pool `batches`."""

    def __init__(self, steps, batches):
        self.steps, self.batches = steps, list(batches)

    def __len__(self):
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            yield self.batches[i % len(self.batches)]


def start_process(script_name):
    """What every task script's main() starts with: the launcher's environment, the GPU check, the device, and the process group of a
    multi-GPU run (utils.init_distributed_mode, utils/__init__.py:388-410).  Returns (rank, local_rank, world_size, device)."""
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world_size = int(os.environ.get("WORLD_SIZE", 1))
    if not torch.cuda.is_available():
        raise RuntimeError(f"{script_name} needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world_size > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", world_size=world_size, rank=rank)
    return rank, local_rank, world_size, device


def finish_process(world_size, barrier=True):
    """What every main() ends with.  `barrier=False`: the caller has met the other ranks already (Pretrain.py, before its files)."""
    if world_size > 1:
        if barrier:
            dist.barrier()
        dist.destroy_process_group()


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def make_accelerator(section, seed):
    """The accelerator a config's `accelerator:` section names; without a section, the default of a loop that clips nothing."""
    from .accelerators import ACCELERATOR_MAP
    arg_acc = AttrDict(section or {"ACCELERATOR": "RCCLDDP", "RNG_SEED": seed, "GRAD_ACCUMULATE_STEPS": 1, "CLIP_GRAD_NORM": 0.0})
    return ACCELERATOR_MAP[arg_acc["ACCELERATOR"]](arg_acc, logger=None)


def load_yaml(path):
    with open(path) as f:
        return yaml.safe_load(f)


def dump_yaml(cfg, out_dir):
    with open(os.path.join(out_dir, "config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
