"""Build-owned deterministic data: formula weights and synthetic image-text batches.

A counter-based generator (splitmix64 over `crc32(name) , element index`) written against numpy
integer arithmetic only, so that the build container, the GPU box and any later round regenerate
bit-identical tensors without shipping them.  Used by the golden-fixture generator (weights are
loaded into the reference with load_state_dict(strict=True)), the parity tests, smoke() and bench.py.

Batch layout mirrors what the reference's collate emits for the image-text pre-training source
(dataset/pretrain_dataset.py:264-312).
"""
import zlib

import numpy as np
import torch

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def uniform01(name, n, seed=0):
    """n doubles in [0,1), a pure function of (name, seed, index)."""
    with np.errstate(over="ignore"):
        key = np.uint64(zlib.crc32(name.encode()) + (int(seed) << 32))
        base = _splitmix64(np.array([key], dtype=np.uint64))[0]
        i = np.arange(n, dtype=np.uint64)
        z = _splitmix64(i * np.uint64(0x2545F4914F6CDD1D) + base)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def symmetric(name, shape, scale, seed=0):
    n = int(np.prod(shape)) if len(shape) else 1
    u = uniform01(name, n, seed)
    return torch.from_numpy(((u * 2.0 - 1.0) * scale).astype(np.float32).reshape(shape))


def gaussian(name, shape, std=1.0, seed=0):
    """Box-Muller over two formula streams."""
    n = int(np.prod(shape))
    u1 = np.maximum(uniform01(name + "#a", n, seed), 1e-12)
    u2 = uniform01(name + "#b", n, seed)
    g = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return torch.from_numpy((g * std).astype(np.float32).reshape(shape))


def formula_tensor(name, ref, seed=0):
    """A deterministic value for state_dict entry `name` shaped/typed like `ref` (an existing tensor).
    Scales are chosen to keep 1-2 layer stacks numerically lively (non-trivial attention, biases and
    layer-scale all matter), not to imitate any trained checkpoint."""
    shape = tuple(ref.shape)
    leaf = name.split(".")[-1]
    if not ref.dtype.is_floating_point:
        return ref.clone()  # integer buffers (relative_position_index, position_ids) keep their built values
    if name == "temp":
        return torch.tensor(0.07, dtype=ref.dtype)
    if "gamma_" in leaf:
        return 0.1 + symmetric(name, shape, 0.03, seed)
    if "relative_position_bias_table" in leaf:
        return symmetric(name, shape, 0.5, seed)
    if leaf in ("cls_token", "mask_token"):
        return symmetric(name, shape, 0.5, seed)
    is_norm = any(t in name for t in ("LayerNorm", "layer_norm", "norm1", "norm2", "fc_norm")) or \
        (name.startswith(("itm_head.1", "bbox_head.1")))
    if is_norm and leaf == "weight":
        return 1.0 + symmetric(name, shape, 0.2, seed)
    if leaf in ("bias", "q_bias", "v_bias"):
        return symmetric(name, shape, 0.1, seed)
    if "embeddings" in name:
        return symmetric(name, shape, 0.1, seed)
    # dense / conv weights: uniform with std ~ 0.05 (xavier-ish for fan_in 768)
    return symmetric(name, shape, 0.05 * 1.7320508, seed)


def formula_state_dict(reference_state, seed=0):
    """Map every entry of an existing state_dict (shapes/dtypes only are used) to its formula value."""
    out = {}
    for k, v in reference_state.items():
        t = formula_tensor(k, v, seed)
        if k.endswith(("lm_head.decoder.bias", "lm_cap_head.decoder.bias", "predictions.decoder.bias")):
            # tied to `<head>.bias` (xroberta.py:1322-1323, xbert.py:690-691)
            t = formula_tensor(k[: -len("decoder.bias")] + "bias", v, seed)
        out[k] = t.to(v.dtype)
    return out


# ----------------------------------------------------------------------------------------------
# synthetic pre-training batch
# ----------------------------------------------------------------------------------------------
BOS, PAD, EOS, MASK_ID, VOCAB = 0, 1, 2, 50264, 50265


def pretrain_batch(batch_size, seed=1234, image_res=224, max_tokens=30, max_masks=15, min_len=8, vocab=VOCAB,
                   with_image=True):
    """image fp32 [B,3,R,R] ~ N(0,1); text_ids int64 [B,T] (<s> ... </s> pad); text_atts prefix ones;
    masked_pos int64 [B,M] distinct in [1,len) zero padded; masked_ids int64 [B,M] (-100 padded);
    text_ids_masked = ids with <mask> at masked_pos."""
    B, T, M = batch_size, max_tokens, max_masks
    tag = f"batch{seed}"
    out = {}
    if with_image:
        out["image"] = gaussian(tag + ".image", (B, 3, image_res, image_res), 1.0)
    lens = (min_len + np.floor(uniform01(tag + ".len", B) * (T - min_len + 1))).astype(np.int64)
    lens = np.clip(lens, min_len, T)
    tok = (3 + np.floor(uniform01(tag + ".tok", B * T) * (vocab - 1 - 3))).astype(np.int64).reshape(B, T)
    ids = np.full((B, T), PAD, dtype=np.int64)
    atts = np.zeros((B, T), dtype=np.int64)
    mpos = np.zeros((B, M), dtype=np.int64)
    mids = np.full((B, M), -100, dtype=np.int64)
    ids_masked = None
    order_u = uniform01(tag + ".perm", B * T).reshape(B, T)
    nm_u = uniform01(tag + ".nmask", B)
    for b in range(B):
        L = int(lens[b])
        ids[b, :L] = tok[b, :L]
        ids[b, 0] = BOS
        ids[b, L - 1] = EOS
        atts[b, :L] = 1
        cand = np.arange(1, L)  # positions [1, len)
        n = int(min(M, max(1, np.floor(nm_u[b] * min(M, L - 1)) + 1)))
        pick = cand[np.argsort(order_u[b, 1:L], kind="stable")[:n]]
        pick.sort()
        mpos[b, :n] = pick
        mids[b, :n] = ids[b, pick]
    ids_masked = ids.copy()
    for b in range(B):
        n = int((mids[b] != -100).sum())
        ids_masked[b, mpos[b, :n]] = MASK_ID if vocab == VOCAB else vocab - 1
    out.update(text_ids=torch.from_numpy(ids), text_atts=torch.from_numpy(atts),
               text_ids_masked=torch.from_numpy(ids_masked), masked_pos=torch.from_numpy(mpos),
               masked_ids=torch.from_numpy(mids))
    return out


def mim_block_mask(batch_size, grid=14, num_masking=75, seed=1234):
    """A deterministic stand-in for the MaskingGenerator draws (masking_generator.py:27-105): exactly
    `num_masking` of grid*grid patches per sample, as a few rectangular blocks topped up with singles.
    Used for parity fixtures and the synthetic benchmark; the product path draws its own masks."""
    B = batch_size
    u = uniform01(f"mim{seed}", B * 64).reshape(B, 64)
    out = np.zeros((B, grid, grid), dtype=bool)
    for b in range(B):
        k = 0
        while out[b].sum() < num_masking and k < 60:
            h = 2 + int(u[b, k] * 6); w = 2 + int(u[b, k + 1] * 6)
            y = int(u[b, k + 2] * (grid - h + 1)); x = int(u[b, k + 3] * (grid - w + 1))
            k += 4
            blk = np.zeros((grid, grid), dtype=bool)
            blk[y:y + h, x:x + w] = True
            if (out[b] | blk).sum() <= num_masking:
                out[b] |= blk
        flat = out[b].reshape(-1)
        need = num_masking - int(flat.sum())
        if need > 0:
            free = np.flatnonzero(~flat)
            flat[free[:need]] = True
    return torch.from_numpy(out.reshape(B, grid * grid))


def vqa_inputs(B=3, image_res=224):
    """VQA fixture inputs shared by the golden generator and the CPU / GPU parity tests: B images + questions, k[b] answers per
    question with annotator weights, and a candidate answer list for the inference-time ranking (top `topk`)."""
    from types import SimpleNamespace as NS
    b = pretrain_batch(B, seed=91, image_res=image_res)
    k = [2, 1, 3][:B]
    ans = pretrain_batch(sum(k), seed=92, max_tokens=7, min_len=3, with_image=False)
    cand = pretrain_batch(5, seed=93, max_tokens=6, min_len=3, with_image=False)
    weights = torch.tensor([0.6, 0.4, 1.0, 0.5, 0.3, 0.2][:sum(k)])
    return NS(image=b["image"], q_ids=b["text_ids"], q_atts=b["text_atts"], k=k, a_ids=ans["text_ids"], a_atts=ans["text_atts"],
              weights=weights, c_ids=cand["text_ids"], c_atts=cand["text_atts"], topk=3)


def retrieval_eval_inputs(n_img=5, n_txt=8):
    """Retrieval-evaluation fixture inputs: n_img images, n_txt captions (caption j describes image txt2img[j]), k_test = 3."""
    from types import SimpleNamespace as NS
    b = pretrain_batch(n_txt, seed=97)
    txt2img = [j % n_img for j in range(n_txt)]
    img2txt = [[j for j in range(n_txt) if txt2img[j] == i] for i in range(n_img)]
    return NS(image=b["image"][:n_img], text_ids=b["text_ids"], text_atts=b["text_atts"], k_test=3, txt2img=txt2img, img2txt=img2txt)


def vqa_batch(batch_size, seed=1234, image_res=480, max_tokens=40, max_answers=10, answer_len=8):
    """BASELINE configs[3] synthetic batch (the collate of dataset/vqa_dataset.py as VQA.py:45-52 consumes it): B images +
    questions of up to `max_tokens` tokens, k[b] ~ U[1, max_answers] answers per question (<s> ... </s>, up to `answer_len` tokens,
    pad = 1) and one annotator weight per answer (the weights of a question sum to 1)."""
    from types import SimpleNamespace as NS
    b = pretrain_batch(batch_size, seed=seed, image_res=image_res, max_tokens=max_tokens)
    k = [int(v) for v in (1 + np.floor(uniform01(f"vqa{seed}.k", batch_size) * max_answers)).clip(1, max_answers)]
    ans = pretrain_batch(sum(k), seed=seed + 1, max_tokens=answer_len, min_len=3, with_image=False)
    w = uniform01(f"vqa{seed}.w", sum(k)) + 0.1
    o = 0
    for n in k:
        w[o:o + n] /= w[o:o + n].sum()
        o += n
    return NS(image=b["image"], q_ids=b["text_ids"], q_atts=b["text_atts"], k=k, a_ids=ans["text_ids"], a_atts=ans["text_atts"],
              weights=torch.from_numpy(w.astype(np.float32)))


def region_case(n_images, grid=14):
    """Inputs of the vision tower's region call form (beit2.py:467-475): bs = n_images + 2 samples over n_images images
    (`idx_to_group_img` [bs], some images used twice) and a ragged region mask per sample (`image_atts` [bs, 1 + grid^2] of 0 / 1: a
    rectangle of patches, column 0 = the cls slot, always 1)."""
    bs = n_images + 2
    idx = torch.tensor([(3 * i + 1) % n_images for i in range(bs)], dtype=torch.long)
    atts = torch.zeros(bs, 1 + grid * grid, dtype=torch.long)
    atts[:, 0] = 1
    for i in range(bs):
        y0, x0 = (2 * i) % (grid - 4), (3 * i + 1) % (grid - 5)
        h, w = 3 + i % 4, 4 + (2 * i) % 5
        m = torch.zeros(grid, grid, dtype=torch.long)
        m[y0:y0 + h, x0:x0 + w] = 1
        atts[i, 1:] = m.reshape(-1)
    return idx, atts


def region_batch(batch_size, max_images, max_regions, seed=1234, image_res=224, patch_size=16, max_tokens=30, max_masks=15, vocab=VOCAB):
    """A region batch in the tuple layout that run_region_iter unpacks (Pretrain.py:94-99; the collate of the reference's region dataset):
    (image [n_img, 3, R, R], idx_to_group_img [bs], text_ids, text_atts, text_ids_masked, masked_pos, masked_ids [bs, ...],
    image_atts [bs, 1 + grid^2] of 0 / 1, target_bbox fp32 [bs, 4] as (cx, cy, w, h) in [0, 1], is_image [bs] of 0 / 1).
    bs = batch_size samples, image by image: every image carries 1..max_regions of them, at most max_images images.  A sample is either
    the whole image (is_image = 1: all patches, box (0.5, 0.5, 1, 1)) or a rectangle of patches with the box that bounds it -- every mask
    has at least one patch."""
    assert max_images * max_regions >= batch_size, "max_images * max_regions samples at the most"
    grid = image_res // patch_size
    tag = f"region{seed}"
    counts, left = [], batch_size
    draw = uniform01(tag + ".count", max_images)
    for i in range(max_images):
        if left == 0:
            break
        images_after = max_images - i - 1
        lo = max(1, left - images_after * max_regions)   # what this image must take for the rest to fit
        k = min(max(lo, 1 + int(draw[i] * max_regions)), max_regions, left)
        counts.append(k)
        left -= k
    n_img = len(counts)
    idx = np.repeat(np.arange(n_img), counts)
    u = uniform01(tag + ".box", batch_size * 5).reshape(batch_size, 5)
    atts = np.zeros((batch_size, 1 + grid * grid), dtype=np.int64)
    atts[:, 0] = 1
    target = np.zeros((batch_size, 4), dtype=np.float32)
    is_image = np.zeros(batch_size, dtype=np.int64)
    for s in range(batch_size):
        if s > 0 and u[s, 4] < 0.2:   # the whole image with its caption (never sample 0: the box losses divide by the number of regions)
            is_image[s] = 1
            y0, x0, h, w = 0, 0, grid, grid
        else:
            h, w = 1 + int(u[s, 0] * (grid - 1)), 1 + int(u[s, 1] * (grid - 1))
            y0, x0 = int(u[s, 2] * (grid - h + 1)), int(u[s, 3] * (grid - w + 1))
        m = np.zeros((grid, grid), dtype=np.int64)
        m[y0:y0 + h, x0:x0 + w] = 1
        atts[s, 1:] = m.reshape(-1)
        target[s] = [(x0 + 0.5 * w) / grid, (y0 + 0.5 * h) / grid, w / grid, h / grid]
    b = pretrain_batch(batch_size, seed=seed, image_res=image_res, max_tokens=max_tokens, max_masks=max_masks, vocab=vocab, with_image=False)
    image = gaussian(tag + ".image", (n_img, 3, image_res, image_res), 1.0)
    return (image, torch.from_numpy(idx), b["text_ids"], b["text_atts"], b["text_ids_masked"], b["masked_pos"], b["masked_ids"],
            torch.from_numpy(atts), torch.from_numpy(target), torch.from_numpy(is_image))


def imagenet_batch(batch_size, seed=1234, image_res=224, num_labels=1000):
    """(images fp32 [B, 3, res, res], labels int64 [B]) in the tuple layout of Imagenet.py:453's loader: formula images (unit Gaussian, what
    Normalize leaves) and formula labels in [0, num_labels), pure functions of (seed, index)."""
    image = gaussian(f"imagenet.image.{seed}", (batch_size, 3, image_res, image_res))
    u = uniform01("imagenet.label", batch_size, seed)
    labels = torch.from_numpy(np.minimum((u * num_labels).astype(np.int64), num_labels - 1))
    return image, labels


def vqa_answer_list(num_answers, seed=1234, answer_len=8, shared=2, vocab=VOCAB):
    """A synthetic candidate answer list in the layout VQA.py:87 tokenizes (`<s> ... </s>` rows, pad = 1): (ids int64 [A, answer_len],
    atts int64 [A, answer_len], names = the list of A answer strings).  Every first answer token is shared by `shared` candidates on
    average (first tokens are drawn from a pool of A / shared tokens), as in the real list, where "yes", "yes it is" ... start alike: the
    first-token probabilities of the ranking then carry ties."""
    b = pretrain_batch(num_answers, seed=seed, max_tokens=answer_len, min_len=3, vocab=vocab, with_image=False)
    ids = b["text_ids"].clone()
    pool = max(num_answers // max(shared, 1), 1)
    first = (3 + np.floor(uniform01(f"vqa_answers{seed}.pool", pool) * (vocab - 1 - 3))).astype(np.int64)
    pick = np.minimum((uniform01(f"vqa_answers{seed}.pick", num_answers) * pool).astype(np.int64), pool - 1)
    ids[:, 1] = torch.from_numpy(first[pick])
    return ids, b["text_atts"], [f"answer{i}" for i in range(num_answers)]


def vqa_eval_batch(batch_size, seed=1234, image_res=480, max_tokens=40, first_question_id=0):
    """One test batch in the tuple layout of VQA.py:89's loader, questions as token ids: (image fp32 [B, 3, res, res], (q_ids, q_atts)
    int64 [B, max_tokens], question_id int64 [B] = first_question_id + 0 .. B - 1)."""
    b = pretrain_batch(batch_size, seed=seed, image_res=image_res, max_tokens=max_tokens)
    return b["image"], (b["text_ids"], b["text_atts"]), torch.arange(first_question_id, first_question_id + batch_size)


def glue_batch(batch_size, seed=1234, max_length=128, min_len=8, vocab=VOCAB, pad_id=PAD, num_labels=2):
    """One GLUE batch as run_glue.py:283's collate emits it (`padding='longest'`): (input_ids int64 [B, T], attention_mask int64 [B, T],
    labels) with T the longest sequence of THIS batch (<= max_length), `<s> ... </s>` rows padded with pad_id.  Labels: int64 in
    [0, num_labels) for classification; for num_labels == 1 (STS-B) fp32 similarity scores on a 0.2 grid in [0, 5], so that the label
    ranks are full of ties."""
    b = pretrain_batch(batch_size, seed=seed, max_tokens=max_length, min_len=min(min_len, max_length), vocab=vocab, with_image=False)
    atts = b["text_atts"]
    T = int(atts.sum(1).max())
    ids, atts = b["text_ids"][:, :T].clone(), atts[:, :T].clone()
    ids[atts == 0] = pad_id
    u = uniform01("glue.label", batch_size, seed)
    if num_labels == 1:
        labels = torch.from_numpy((np.minimum(np.floor(u * 26.0), 25.0) / 5.0).astype(np.float32))
    else:
        labels = torch.from_numpy(np.minimum((u * num_labels).astype(np.int64), num_labels - 1))
    return ids, atts, labels


def _grounding_text(batch_size, seed, max_tokens, min_len, vocab):
    """Expressions as Grounding_bbox.py:52 tokenizes them (`padding='longest'`): ids / atts int64 [B, T], T the longest row of the batch."""
    b = pretrain_batch(batch_size, seed=seed, max_tokens=max_tokens, min_len=min(min_len, max_tokens), vocab=vocab, with_image=False)
    atts = b["text_atts"]
    T = int(atts.sum(1).max())
    return b["text_ids"][:, :T].clone(), atts[:, :T].clone()


def grounding_batch(batch_size, seed=1234, image_res=384, max_tokens=40, min_len=5, vocab=VOCAB):
    """One training batch in the tuple layout of Grounding_bbox.py:50's loader, expressions as token ids: (image fp32 [B, 3, res, res],
    (text_ids, text_atts) int64 [B, T], target_bbox fp32 [B, 4] = (cx, cy, w, h) in [0, 1], every box inside the image with w, h in
    [0.1, 0.6])."""
    image = gaussian(f"grounding.image.{seed}", (batch_size, 3, image_res, image_res))
    ids, atts = _grounding_text(batch_size, seed, max_tokens, min_len, vocab)
    u = uniform01("grounding.box", batch_size * 4, seed).reshape(batch_size, 4)
    w, h = 0.1 + 0.5 * u[:, 2], 0.1 + 0.5 * u[:, 3]
    cx, cy = w / 2 + u[:, 0] * (1.0 - w), h / 2 + u[:, 1] * (1.0 - h)
    return image, (ids, atts), torch.from_numpy(np.stack([cx, cy, w, h], axis=1).astype(np.float32))


def grounding_eval_batch(batch_size, seed=1234, image_res=384, max_tokens=40, min_len=5, first_ref_id=0, vocab=VOCAB):
    """One test batch in the tuple layout of Grounding_bbox.py:81's loader: (image, (text_ids, text_atts), ref_ids int64 [B] =
    first_ref_id + 0 .. B - 1)."""
    image = gaussian(f"grounding.eval_image.{seed}", (batch_size, 3, image_res, image_res))
    ids, atts = _grounding_text(batch_size, seed + 7919, max_tokens, min_len, vocab)
    return image, (ids, atts), torch.arange(first_ref_id, first_ref_id + batch_size)


def grounding_refs(num_refs, seed=1234, first_ref_id=0):
    """The ground truth the grounding evaluation reads (refer.Refs / refToAnn / Imgs of dataset/utils.py:276-279) as three tables and an
    index: ref_box fp32 [R, 4] = (x, y, w, h) in pixels, ref_size fp32 [R, 2] = (width, height), ref_split int32 [R] (0 val, 1 testA,
    2 testB: row r is split r % 3, so all three occur from R = 3), ref_index = {ref_id: row}.  Every box is valid: x, y >= 0, w, h > 0,
    inside its image; whole pixels, as the COCO annotations mostly are."""
    from types import SimpleNamespace as NS
    assert num_refs >= 3, "fewer than three refs cannot cover val, testA and testB"
    u = uniform01("grounding.refs", num_refs * 6, seed).reshape(num_refs, 6)
    W, H = np.floor(320 + 320 * u[:, 0]), np.floor(240 + 240 * u[:, 1])
    w, h = np.floor(W * (0.1 + 0.5 * u[:, 2])) + 1, np.floor(H * (0.1 + 0.5 * u[:, 3])) + 1
    x, y = np.floor(u[:, 4] * (W - w)), np.floor(u[:, 5] * (H - h))
    return NS(ref_box=torch.from_numpy(np.stack([x, y, w, h], axis=1).astype(np.float32)),
              ref_size=torch.from_numpy(np.stack([W, H], axis=1).astype(np.float32)),
              ref_split=torch.from_numpy((np.arange(num_refs) % 3).astype(np.int32)),
              ref_index={first_ref_id + r: r for r in range(num_refs)})


def grounding_dets(refs, seed=1234, min_boxes=3, max_boxes=8):
    """The detector boxes the mask-based grounding evaluation ranks (dets[str(image_id)] of dataset/utils.py:195), one fp64 [k, 4] array of
    (x, y, w, h) per row of `refs` (grounding_refs), k in [min_boxes, max_boxes]: box 0 is the ground-truth box moved by a few pixels (a
    detector usually proposes the object), the others are formula boxes inside the image; fractional coordinates, as detector output is."""
    size = refs.ref_size.double().numpy()
    box = refs.ref_box.double().numpy()
    R = size.shape[0]
    count = min_boxes + (uniform01("grounding.dets.count", R, seed) * (max_boxes - min_boxes + 1)).astype(np.int64).clip(0, max_boxes - min_boxes)
    u = uniform01("grounding.dets", R * max_boxes * 4, seed).reshape(R, max_boxes, 4)
    out = []
    for r in range(R):
        W, H = size[r]
        w, h = 8.0 + u[r, :, 2] * 0.5 * W, 8.0 + u[r, :, 3] * 0.5 * H
        x, y = u[r, :, 0] * (W - w), u[r, :, 1] * (H - h)
        d = np.stack([x, y, w, h], axis=1)[:count[r]]
        d[0] = (min(box[r, 0] + 1.5, W - 1.0), min(box[r, 1] + 0.75, H - 1.0), box[r, 2], box[r, 3])
        out.append(np.ascontiguousarray(d, dtype=np.float64))
    return out
