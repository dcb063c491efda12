"""The VQA fine-tune / evaluation task loop around the HIP step: the training epoch, the answer-ranking evaluation pass, the accuracy
and the per-epoch checkpoint / evaluation loop of VQA.py.

Mirrors (names, argument meaning, ordering):
  * train_one_epoch   VQA.py:35-72    (`train` there; `train` here is the epoch loop of main())
  * evaluation        VQA.py:75-100
  * calculate_acc     VQA.py:103-122
  * train             VQA.py:233-267
The optimizer (four AdamW groups, `lr_mult` on model.init_params) and the linear warm-up / decay schedule are the pre-training loop's
(pretrain_loop.create_optimizer / create_scheduler = optim.py / scheduler.py, which VQA.py:216-220 calls); the step runs through
RCCLDDPAccelerator on the transformers-rule xfm_adamw.
What differs, on purpose:
  * the batches carry TOKEN IDS -- a question / answer is an (input_ids, attention_mask) pair where the reference tokenizes strings
    (:48-49, :87, :91); there is no tokenizer and no dataset code on this path.  The test loader's `dataset` holds `answer_list` (the
    strings of the records) and `answer_input` (their ids and mask);
  * the reference reads the loss with `.item()` after every step (:66); here the loss tensors are parked (task.LossMeters) and
    read when a log line is due;
  * the reference reads two device values per QUESTION (:95-98: `.item()`, `.max()` indexing a Python list); here the model runs with
    `fused=True` -- xfm_answer_shortlist / xfm_answer_rerank -- and writes every question's winning candidate id into ONE device buffer
    that is read once per pass;
  * `accumulate_steps` > 1 (:53-57) is not built: every shipped config leaves it at 1."""
import json
import os

import torch

from .task import LossMeters, is_distributed, is_main_process, to_device, unwrap
from .task import read as _read  # the loop's single device-to-host read (evaluation calls it once per pass; the tests count its calls)


def _accumulate_steps(config):
    accumulate_steps = int(config.get('accumulate_steps', 1))
    if accumulate_steps > 1:
        raise NotImplementedError(f"accumulate_steps == {accumulate_steps} (VQA.py:53-57) is not built: every shipped config trains with 1")
    return accumulate_steps


def train_one_epoch(model, data_loader, optimizer, epoch, device, scheduler, config, accelerator, print_freq=50, log=None):
    """VQA.py:35-72 (`train`): per iteration -- upload, loss = model(image, question, answer, train=True, k=n, weights=weights), backward
    and step through the accelerator, scheduler.step().  A batch is (image, (q_ids, q_atts), (a_ids, a_atts), weights, n) with n the
    host-side list of answers per question.  Returns the epoch's meters formatted as the reference does (:72)."""
    _accumulate_steps(config)
    model.train()
    meters = LossMeters()
    for i, (image, question, answer, weights, n) in enumerate(data_loader):
        image, weights, question_input, answer_input = to_device(device, (image, weights, question, answer))
        loss = model(image, question_input, answer_input, train=True, k=n, weights=weights)
        meters.update(loss=loss, lr=optimizer.param_groups[0]["lr"])
        accelerator.backward_step(loss, optimizer)
        accelerator.optimizer_step(optimizer, model)   # i % accumulate_steps == 0 always: accumulate_steps is 1
        scheduler.step()
        optimizer.zero_grad()
        if i % print_freq == 0:
            meters.flush()
            if log is not None:
                log(epoch, i, meters.global_avg())
    avg = meters.global_avg()
    print("Averaged stats:", {k: round(v, 6) for k, v in avg.items()}, flush=True)
    return {k: "{:.5f}".format(v) for k, v in avg.items()}


@torch.no_grad()
def evaluation(model, data_loader, device, config):
    """VQA.py:75-100: rank the candidate answers for every test question, k_test re-ranked.  The candidate tensors are uploaded once;
    every batch writes its winners (candidate ids) behind the previous batch's in one int64 device buffer, read ONCE at the end.
    A batch is (image, (q_ids, q_atts), question_id).  Returns the reference's list of {"question_id", "answer"} records."""
    model.eval()
    answer_list = data_loader.dataset.answer_list
    answer_input = to_device(device, data_loader.dataset.answer_input)
    fused = answer_input[0].is_cuda   # (a CPU model path has no kernels to fuse onto)
    # one slot per question: len(loader) batches of at most batch_size_test (a larger batch fails the kernel wrapper's range check)
    winners = torch.zeros(len(data_loader) * config['batch_size_test'], dtype=torch.int64, device=device)
    question_ids, done = [], 0
    for image, question, question_id in data_loader:
        image, question_input = to_device(device, (image, question))
        n = image.size(0)
        if fused:
            model(image, question_input, answer_input, train=False, k=config['k_test'], fused=True, result=winners, result_offset=done)
        else:
            topk_ids, topk_probs = model(image, question_input, answer_input, train=False, k=config['k_test'])
            winners[done:done + n] = topk_ids.gather(1, topk_probs.argmax(dim=1, keepdim=True)).view(-1)   # :97 `topk_prob.max(dim=0)`
        question_ids.extend(int(q) for q in (question_id.tolist() if torch.is_tensor(question_id) else question_id))   # (host tensors)
        done += n
    picked = _read(winners[:done])
    return [{"question_id": ques_id, "answer": answer_list[a]} for ques_id, a in zip(question_ids, picked)]


def calculate_acc(result_rpath, test_dataset):
    """VQA.py:103-122: exact-match accuracy of a result file against the annotations that carry an answer; None (as the reference's bare
    `return`) when the split has none.  Prints the reference's two lines and returns n_correct / n."""
    gt = {}
    for ann in test_dataset.ann:
        if 'answer' in ann.keys():
            gt[ann['question_id']] = ann['answer'].strip()
        else:
            return None
    n = 0
    n_correct = 0
    with open(result_rpath, 'r') as f:
        for sample in json.load(f):
            n += 1
            index = sample['question_id']
            if sample['answer'].strip() == gt[index]:
                n_correct += 1
    print(f"n_questions: {n}, n_correct: {n_correct}", flush=True)
    if n > 0:
        print(f"acc: {n_correct / n}", flush=True)
        return n_correct / n
    return None


def save_result(result, result_dir, filename):
    """dataset/utils.py collect_result on one process: the records as <result_dir>/<filename>.json; returns the path."""
    os.makedirs(result_dir, exist_ok=True)
    path = os.path.join(result_dir, '%s.json' % filename)
    with open(path, 'w') as f:
        json.dump(result, f)
    return path


def train(model, train_loader, test_loader, optimizer, device, scheduler, config, accelerator, checkpointer, output_dir, result_dir,
          start_epoch=0, train_sampler=None, print_freq=50, log=None):
    """VQA.py:233-267: per epoch -- train, on the main process a log.txt line and a checkpoint through
    `checkpointer.save_checkpoint(model_state=..., epoch=..., training_states=...)` (optimizer.state_dict() carries the fused AdamW
    moments in torch's format), then from epoch `start_eval` an evaluation pass whose records go to
    <result_dir>/vqa_result_epoch<N>.json.  Returns the list of result files written."""
    _accumulate_steps(config)
    results = []
    max_epoch = config['schedular']['epochs']
    for epoch in range(start_epoch, max_epoch):
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        train_stats = train_one_epoch(model, train_loader, optimizer, epoch, device, scheduler, config, accelerator, print_freq=print_freq,
                                      log=log)
        if is_main_process():
            log_stats = {**{f'train_{k}': v for k, v in train_stats.items()}, 'epoch': epoch}
            with open(os.path.join(output_dir, "log.txt"), "a") as f:
                f.write(json.dumps(log_stats) + "\n")
            save_obj = {'model': unwrap(model).state_dict(), 'config': config}
            if checkpointer is not None:
                checkpointer.save_checkpoint(model_state=save_obj, epoch=epoch, training_states=optimizer.state_dict())
        if epoch >= config['start_eval']:
            vqa_result = evaluation(model, test_loader, device, config)
            if is_main_process():   # (one node: every rank ranks the whole synthetic test set; collect_result's gather is not needed)
                results.append(save_result(vqa_result, result_dir, 'vqa_result_epoch%d' % epoch))
        if is_distributed():
            torch.distributed.barrier()
    return results
