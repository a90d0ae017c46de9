"""`test` and `run_tester` of the reference (`core/tools/test.py:27-250`): same signatures, return values and log lines.
The batches are born on the device (no `TransferTensorDict`, no `tqdm` bar), `DeviceMetric` takes the place of `Metric`
(no synchronisation per batch), and `run_tester(..., *, prefetch=2)` reads each annotation file through a prefetching
`ClipLoader` over the CenterCrop pipeline the reference's tester composes (:136-171)."""
import contextlib
import json
import os
import time

import torch
import torch.distributed as dist

from ..dataset.dataset import Video_Dataset
from ..dataset.transform import get_transforms
from ..models import build_model
from ..utils import ClipLoader, DeviceMetric, get_time_diff, save_scores
from .train import QUIET, current_device, group_ranks, local_plans, sharded

LINE = "----------------------------------------------------------"


def test(cfg, model, data_loader, criterion, modality, logger, device=torch.device("cuda")):
    """reference :27-94 -> (test_loss, test_acc, conf_mat[, output]); the metrics are taken only for labelled data, and
    with `cfg.test.save_results` `output` is {"action_id": [per batch], head: [scores per batch]}.

    As one rank of several: this rank's shares through the bare module, no collective per batch (see `validate`); the
    metrics are merged and equal on every rank.  With `save_results` the ranks' ids and scores travel to rank 0 in ONE
    object gather after the loop (the shares' sizes differ) and are put back together per GLOBAL batch, shares in rank
    order: rank 0's `output` is the single process's, every uid once and in its order.  On the other ranks `output`
    holds that rank's own shares."""
    rank, world = group_ranks()
    no_batches = round(len(data_loader.dataset) / data_loader.batch_size)
    heads = list(cfg.model.num_classes.keys())
    if world > 1:
        sharded(data_loader, world, "test")
    metric = DeviceMetric(cfg, no_batches, device, process_group=dist.group.WORLD if world > 1 else None)
    model.eval()
    bare = getattr(model, "module", model) if world > 1 else model
    if cfg.test.save_results:
        output = {"action_id": []}
        for key in heads:
            output[key] = []
        rows = []               # the global batch number of every entry of `output`
    with torch.no_grad(), (local_plans(bare) if world > 1 else contextlib.nullcontext()):
        for data, target, action_id in data_loader:
            out = bare(data)
            if isinstance(target["class"], dict):
                loss, batch_size = bare.get_loss(criterion, target, out)
                if world > 1:
                    metric.set_metrics(out, target, batch_size, loss, share=data_loader.share, row=data_loader.batch_no)
                else:
                    metric.set_metrics(out, target, batch_size, loss)
            if cfg.test.save_results:
                output["action_id"].extend([action_id])
                for key in heads:
                    output[key].extend([out[key]])
                if world > 1:
                    rows.append(data_loader.batch_no)
    test_loss, test_acc, conf_mat = metric.get_metrics()
    if cfg.test.save_results:
        if world > 1:
            output = _gather_output(output, rows, heads, rank, world, device)
        return (test_loss, test_acc, conf_mat, output)
    return (test_loss, test_acc, conf_mat)


def _gather_output(output, rows, heads, rank, world, device):
    """every rank's (global batch number, ids, scores per head) to rank 0 -> there, the lists per global batch with the
    shares joined in rank order; elsewhere the rank's own `output`, untouched"""
    def host(x):
        return x.detach().cpu() if torch.is_tensor(x) else list(x)
    mine = [(no, host(output["action_id"][i]), {key: host(output[key][i]) for key in heads}) for i, no in enumerate(rows)]
    every = [None] * world if rank == 0 else None
    dist.gather_object(mine, every, dst=0)
    if rank != 0:
        return output
    shares = {}
    for part in every:                      # rank order
        for no, ids, scores in part:
            shares.setdefault(no, []).append((ids, scores))
    joined = {"action_id": []}
    for key in heads:
        joined[key] = []
    for no in sorted(shares):
        ids = [s[0] for s in shares[no]]
        if all(torch.is_tensor(u) for u in ids):
            joined["action_id"].append(torch.cat(ids).to(device))
        else:
            joined["action_id"].append([u for part in ids for u in (part.tolist() if torch.is_tensor(part) else part)])
        for key in heads:
            joined[key].append(torch.cat([s[1][key] for s in shares[no]]).to(device))
    return joined


def run_tester(cfg, logger, modality, *, prefetch=2):
    """reference :97-250: one dataset and loader per `cfg.test.annotation_file` entry.

    As one rank of several (default process group and current device set by the caller, as for `run_trainer`):
    `cfg.test.batch_size` is the global batch, every rank loads the weights and reads its shares, and rank 0 alone logs
    and writes the score files."""
    rank, world = group_ranks()
    device = current_device()
    if rank != 0:
        logger = QUIET
    logger.info("Initializing model...")
    model, criterion, num_gpus = build_model(cfg, modality, device)
    logger.info("Model initialized.")
    logger.info(model)
    logger.info(LINE)
    if not cfg.test.pre_trained:
        raise ValueError("No pre-trained weights exist. Please set the pre_trained parameter for test in config file.")
    pre_trained = cfg.test.pre_trained
    logger.info("Loading pre-trained weights {}...".format(pre_trained))
    data_dict = torch.load(pre_trained, map_location="cpu")
    (model.module if num_gpus > 1 and hasattr(model, "module") else model).load_state_dict(data_dict["model"])
    logger.info("Done.")
    logger.info(LINE)
    test_transforms = get_transforms(cfg, modality, mode="test", device=device,
                                     flow_length=2 * cfg.data.flow.win_length)
    annotation_files = cfg.test.annotation_file
    if isinstance(annotation_files, str):
        annotation_files = [annotation_files]
    logger.info("No of files to test: {}".format(len(annotation_files)))
    logger.info(LINE)
    if cfg.test.save_results:
        assert len(annotation_files) == len(cfg.test.results_file), \
            "Number of annotations files to test ({}) and number of result files ({}) do not match".format(
                len(annotation_files), len(cfg.test.results_file))
    start_time = time.time()
    for idx, annotation in enumerate(annotation_files):
        if cfg.test.vid_list:
            logger.info("Reading list of test videos...")
            file_dir = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            with open(os.path.join(file_dir, cfg.test.vid_list)) as f:
                test_list = [x.strip() for x in f.readlines() if len(x.strip()) > 0]
            logger.info("Done.")
            logger.info(LINE)
        else:
            test_list = None
        logger.info("Creating the dataset using {}...".format(annotation))
        test_dataset = Video_Dataset(cfg, test_list, annotation, modality, transform=test_transforms, mode="test",
                                     device=device)
        test_loader = ClipLoader(test_dataset, cfg.test.batch_size, shuffle=False, prefetch=prefetch,
                                 shard=(rank, world) if world > 1 else None, logger=logger)
        logger.info("Done.")
        logger.info(LINE)
        logger.info("{} action segments to be processed.".format(len(test_dataset)))
        logger.info("Inference in progress...")
        try:
            results = test(cfg, model, test_loader, criterion, modality, logger, device)
        finally:
            test_loader.close()
        logger.info(LINE)
        logger.info("Test_Loss: {}".format(results[0]))
        logger.info(LINE)
        logger.info("Accuracy Top {}:".format(cfg.val.topk))
        logger.info(json.dumps(results[1], indent=2))
        logger.info(LINE)
        if cfg.test.save_results and rank == 0:
            output_dict = results[3]
            if cfg.out_dir:
                out_file = os.path.join(cfg.out_dir, "inferences", cfg.test.results_file[idx])
            else:
                out_file = os.path.join("./inferences", cfg.test.results_file[idx])
            try:
                import pandas as pd
                action_names = pd.read_pickle(os.path.join(cfg.data_dir, "annotations", "action_id_to_name.pkl"))
                save_scores(output_dict, out_file, action_names)
                logger.info("Saved results to {}".format(out_file))
            except Exception as e:
                logger.exception(e)
    hours, minutes, seconds = get_time_diff(start_time, time.time())
    logger.info("Inference time: {} hours, {} minutes, {} seconds,".format(hours, minutes, seconds))
