"""Weakly-supervised grounding evaluation task script on the HIP hot path: the evaluate branch of the reference's Grounding.py:129-212
(argparse + YAML config -> XFMForRetrieval, `val` = the Grad-CAM map of every referring expression at fusion layer `--block_num`,
`grounding_eval` = the detector-box ranking of dataset/utils.py:178-223).  The pass itself is xfm_amd.gradcam (val, grounding_eval).

What differs, on purpose: evaluate only -- the ITC + ITM training loop of Grounding.py:35-73 is the retrieval fine-tune loop, which is not
built, so the script raises without `--evaluate`; `--gradcam_mode itc` raises as it does in the reference (:117-118).  The dataset side
(dataset/grounding_dataset.py, the tokenizer, the REFER tools, the detector files) is outside the hot-path scope: the loader is synthetic
(`synthetic: true`: formula images, expression token ids, ref tables with all three splits and formula detector boxes,
xfm_amd.synthetic.grounding_eval_batch / grounding_refs / grounding_dets); a caller with real data passes its own loader, tables and boxes
to `xfm_amd.gradcam.val` / `grounding_eval`.  `--checkpoint` is optional: without one the model keeps its random initialisation.  The
reference's launcher has no task that reaches Grounding.py, so run.py has none either.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from xfm_amd import task as T  # noqa: E402


class SyntheticTestLoader(T.CycledBatches):
    """`steps` batches (image, text, ref_ids) in the layout of Grounding.py:87's loader with token ids for strings; ref ids count up over
    the pass; `dataset` carries the ref tables and `dets`, the detector boxes of every ref's image."""

    def __init__(self, steps, batch_size, seed, image_res, max_tokens, pool=2):
        from xfm_amd import synthetic as syn
        super().__init__(steps, [syn.grounding_eval_batch(batch_size, seed=s, image_res=image_res, max_tokens=max_tokens)
                                 for s in T.pool_seeds(seed, steps, pool)])
        self.batch_size = batch_size
        self.dataset = syn.grounding_refs(steps * batch_size, seed=seed + 15485863)
        self.dataset.dets = syn.grounding_dets(self.dataset, seed=seed + 32452843)

    def __iter__(self):
        for i, (image, text, ref_ids) in enumerate(super().__iter__()):
            yield image, text, ref_ids + i * self.batch_size


def synthetic_loader(config, seed):
    if not config.get("synthetic", False):
        raise NotImplementedError("file-backed datasets (dataset/grounding_dataset.py, the tokenizer, the REFER tools, dets.json) are "
                                  "outside the hot-path scope: set `synthetic: true` or call xfm_amd.gradcam.val / grounding_eval yourself")
    n_test = max(config["test_dataset_size"] // config["batch_size"], 1)
    return SyntheticTestLoader(n_test, config["batch_size"], seed + 104729, config["image_res"], config.get("max_tokens", 40))


def main(args, config):
    from xfm_amd import gradcam as GC
    from xfm_amd.model_retrieval import XFMForRetrieval

    if not args.evaluate:
        raise NotImplementedError("Grounding.py trains with the ITC + ITM loop of the retrieval fine-tune (Grounding.py:35-73), which is "
                                  "not built: run with --evaluate")
    if args.gradcam_mode != 'itm':
        raise NotImplementedError("gradcam_mode 'itc' (Grounding.py:117-118 raises there too)")
    rank, local_rank, world_size, device = T.start_process("Grounding.py")
    if world_size > 1:
        raise NotImplementedError("sharded multi-GPU evaluation (collect_result among ranks) is not built: one process")
    seed = args.seed + rank
    T.seed_all(seed)
    test_loader = synthetic_loader(config, seed)

    print("Creating model", flush=True)
    model = XFMForRetrieval(config=config)
    if args.checkpoint and os.path.exists(args.checkpoint):
        model.load_pretrained(args.checkpoint, config, is_eval=True)
    model = model.to(device)
    model.finalize()
    print("### Total Params: ", sum(p.numel() for p in model.parameters() if p.requires_grad), flush=True)

    start_time = time.time()
    print("Start evaluating", flush=True)
    num_patches = config['image_res'] // config['patch_size']
    cams, ref_ids = GC.val(model, test_loader, device, args.block_num, num_patches)
    refs = test_loader.dataset
    rows = [refs.ref_index[r] for r in ref_ids]
    from types import SimpleNamespace as NS
    picked = NS(ref_box=refs.ref_box[rows], ref_size=refs.ref_size[rows], ref_split=refs.ref_split[rows])
    grounding_acc = GC.grounding_eval(cams, picked, [refs.dets[r] for r in rows], alpha=config.get('alpha', 0.5))
    if rank == 0:
        print({**{f'{k}': v for k, v in grounding_acc.items()}}, flush=True)
    print('### Time {:.1f} s'.format(time.time() - start_time), flush=True)
    T.finish_process(world_size)
    return grounding_acc


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--checkpoint", type=str, default="")
    parser.add_argument("--config", type=str, default="configs/Grounding_synthetic.yaml")
    parser.add_argument("--output_dir", type=str, default="output/refcoco")
    parser.add_argument("--gradcam_mode", default="itm", choices=["itm", "itc"])
    parser.add_argument("--block_num", default=None, type=int, help="the fusion layer whose cross-attention is read (default: the config's)")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=42, type=int)
    parser.add_argument("--evaluate", action="store_true")
    return parser.parse_args(argv)


if __name__ == "__main__":
    a = parse_args()
    cfg = T.load_yaml(a.config)
    if a.block_num is None:
        a.block_num = cfg.get("block_num", 8)
    os.makedirs(a.output_dir, exist_ok=True)
    T.dump_yaml(cfg, a.output_dir)
    main(a, cfg)
