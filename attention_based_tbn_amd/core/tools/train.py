"""`train`, `validate` and `run_trainer` of the reference (`core/tools/train.py:24-159,162-357`): same signatures, return
values, schedule, checkpoint file and log lines, joined from `build_model`, `build_optimizer`, `create_dataloader`,
`TrainStep`, `DeviceMetric`, `save_checkpoint` and `load_checkpoint`.

What differs, on purpose:
  * the batches are born on the device, so nothing is transferred (`TransferTensorDict`, :63,74) and no `tqdm` bar is drawn;
  * one iteration is `TrainStep.__call__` (the reference's :71-94 schedule, gradient accumulation included) and the
    metric is fed AFTER it, from `TrainStep.last_out` and the loss it returns -- the same tensors the reference feeds;
  * `DeviceMetric` takes the place of `Metric`: no synchronisation per batch.  The host waits for the device only at the
    progress lines, which read `DeviceMetric.running("total")`;
  * `log_interval = max(1, no_batches // 4)`: the reference's `no_batches // 4` (:62) divides by zero below four batches;
  * the reference logs "Clipping gradient: ..." in EVERY iteration whose norm exceeds the bound (:88-91), which costs one
    synchronisation per step; here the line is logged at the progress lines only, from `TrainStep.last_total_norm`;
  * `run_trainer(..., writer=None, *, prefetch=2)`: the loaders prefetch (`ClipLoader(prefetch=)`), and a `writer` is
    anything with `add_scalar(tag, value, epoch)` -- the reference's `Plotter` tags without a tensorboard import;
  * several GPUs are several processes (the reference: one process, `nn.DataParallel`).  When the caller has initialised
    the default `torch.distributed` group with more than one rank and set the current device, the loops here and in
    `test.py` run as ranks of one job: global batch sizes, sharded loaders, merged metrics, rank 0 the only writer.  A
    rank that raises leaves its peers in a collective until the group's timeout, which the caller chose.  Nothing is
    read from the environment.
"""
import contextlib
import json
import os
import time

import torch
import torch.distributed as dist

from ..models import build_model
from ..utils import (DeviceMetric, TrainStep, build_optimizer, create_dataloader, get_time_diff, load_checkpoint,
                     save_checkpoint)

LINE = "----------------------------------------------------------"


class _Quiet(object):
    """the logger of every rank but 0: takes any logging call and says nothing"""

    def __getattr__(self, name):
        return lambda *args, **kwargs: None


QUIET = _Quiet()


def group_ranks():
    """(rank, world) of the default process group the caller initialised; (0, 1) without one"""
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def current_device():
    """the device the loops run on: with several ranks the CURRENT device, which the caller set (one GPU per rank)"""
    if not torch.cuda.is_available():
        return torch.device("cpu")
    if group_ranks()[1] > 1:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cuda")


@contextlib.contextmanager
def local_plans(model):
    """a forward inside runs without the engine-plan exchange of `DataParallel` (`BNInception.plan_sync`, a collective at
    the first forward of a new shape that every rank must enter with the SAME shape): for the forwards whose shapes
    differ between the ranks (unequal shares of a batch) or that not every rank runs (an empty share in validation).
    Each rank then tunes such a shape for itself."""
    held = [(m, m.plan_sync) for m in model.modules() if getattr(m, "plan_sync", None) is not None]
    for m, _ in held:
        m.plan_sync = None
    try:
        yield
    finally:
        for m, sync in held:
            m.plan_sync = sync


def sharded(data_loader, world, who):
    """the loops' check that a job of `world` ranks reads through loaders sharded that way"""
    if getattr(data_loader, "world", 1) != world:
        raise ValueError(f"{who}: the process group has {world} ranks, so the loader must be "
                         f"ClipLoader(shard=(rank, {world})) (create_dataloader(shard=)); every rank would read every clip")


def train(cfg, model, data_loader, optimizer, scheduler, criterion, epoch, logger, device=torch.device("cuda")):
    """one epoch (reference :24-105) -> train_loss, the loss dictionary of `DeviceMetric.get_metrics`.

    As one rank of several (an initialised default process group): `data_loader` is this rank's `ClipLoader(shard=)`;
    every batch's share goes to `TrainStep` (the loss scale) and to the metric, which merges in `get_metrics` -- the
    returned dictionary is the global one, equal on every rank.  Only rank 0 logs; its progress lines show its own
    shares' running loss.  The gradient exchange inside backward is the only collective per batch."""
    rank, world = group_ranks()
    if world > 1:
        sharded(data_loader, world, "train")
        logger = logger if rank == 0 else QUIET
    no_batches = round(len(data_loader.dataset) / data_loader.batch_size)
    log_interval = max(1, no_batches // 4)
    metric = DeviceMetric(cfg, no_batches, device, process_group=dist.group.WORLD if world > 1 else None)
    step = TrainStep.from_config(cfg, model, optimizer, criterion)
    model.train()
    for iter_no, (data, target) in enumerate(data_loader):
        if world > 1:
            share = data_loader.share
            # unequal shares: the ranks' shapes differ, so each tunes this (tail) shape for itself
            with (local_plans(model) if share[0] * world != share[1] else contextlib.nullcontext()):
                loss, batch_size = step(iter_no, data, target, epoch, share=share)
            metric.set_metrics(step.last_out, target, batch_size, loss, share=share, row=data_loader.batch_no)
        else:
            loss, batch_size = step(iter_no, data, target, epoch)
            metric.set_metrics(step.last_out, target, batch_size, loss)
        if rank == 0 and (iter_no == 0 or (iter_no + 1) % log_interval == 0):
            if step.last_total_norm is not None:
                total_norm = float(step.last_total_norm)
                if total_norm > cfg.train.clip_grad:
                    logger.info(f"Clipping gradient: {total_norm} with coef {cfg.train.clip_grad / total_norm}")
            logger.info("Batch Progress: [{}/{}] || Train Loss: {:.5f}".format(
                (iter_no + 1), no_batches, metric.running("total") / (iter_no + 1)))
    train_loss, _, _ = metric.get_metrics()
    return train_loss


def validate(cfg, model, data_loader, criterion, modality, logger, device=torch.device("cuda")):
    """reference :108-159 -> (val_loss, val_acc, conf_mat).

    As one rank of several: this rank's shares through the BARE module (no wrapper, no plan exchange -- a rank whose
    share of a batch is empty runs no forward for it, so nothing in the loop may be a collective); the metric merges in
    `get_metrics`, the only place the ranks meet, and every rank returns the same global results.  The caller makes the
    BatchNorm buffers equal first (`DataParallel.broadcast_buffers`, `run_trainer` does)."""
    rank, world = group_ranks()
    no_batches = len(data_loader.dataset) // data_loader.batch_size
    if world == 1:
        metric = DeviceMetric(cfg, no_batches, device)
        model.eval()
        with torch.no_grad():
            for data, target, _ in data_loader:
                out = model(data)
                loss, batch_size = model.get_loss(criterion, target, out)
                metric.set_metrics(out, target, batch_size, loss)
        return metric.get_metrics()
    sharded(data_loader, world, "validate")
    metric = DeviceMetric(cfg, no_batches, device, process_group=dist.group.WORLD)
    model.eval()
    bare = getattr(model, "module", model)
    with torch.no_grad(), local_plans(bare):
        for data, target, _ in data_loader:
            out = bare(data)
            loss, batch_size = bare.get_loss(criterion, target, out)
            metric.set_metrics(out, target, batch_size, loss, share=data_loader.share, row=data_loader.batch_no)
    return metric.get_metrics()


def run_trainer(cfg, logger, modality, writer=None, *, prefetch=2):
    """reference :162-357: model, optimiser, resume, loaders, the epoch loop, one checkpoint per epoch.

    As one rank of several (the caller has initialised the default process group -- WITH the timeout after which a rank
    whose peer died gives up waiting in a collective -- and set the current device; nothing is read from the
    environment): cfg's batch sizes are GLOBAL and the loaders are sharded; every rank loads a checkpoint to resume from;
    after each epoch's training rank 0's BatchNorm buffers become everyone's (nn.DataParallel's rule that replica 0's
    running statistics are the model's), so validation and the checkpoint see one model; rank 0 alone logs, plots and
    writes the checkpoint, and a barrier follows the write.  The checkpoint is written under a temporary name and renamed."""
    rank, world = group_ranks()
    device = current_device()
    if rank != 0:
        logger, writer = QUIET, None
    epochs = cfg.train.epochs
    logger.info("Initializing model...")
    model, criterion, num_gpus = build_model(cfg, modality, device)
    logger.info("Model initialized.")
    logger.info(model)
    logger.info(LINE)
    optimizer, lr_scheduler, scheduler_warmup = build_optimizer(cfg, model)

    if cfg.train.pre_trained:
        logger.info("Loading pre-trained weights...")
        data_dict = load_checkpoint(cfg.train.pre_trained, model, optimizer, lr_scheduler, num_gpus)
        start_epoch = data_dict["epoch"] + 1
        epochs += start_epoch
        train_loss_hist = data_dict["train_loss"]
        val_loss_hist = data_dict["validation_loss"]
        val_acc_hist = data_dict["validation_accuracy"]
        logger.info(f"Model will continue training from epoch no {start_epoch + 1}")
        logger.info("Done.")
        logger.info(LINE)
    else:
        start_epoch = 0
        train_loss_hist, val_loss_hist = [], []
        val_acc_hist = {k: [] for k in cfg.model.num_classes.keys()}

    checkpoint_name = "tbn_{}_{}.pth".format(cfg.model.arch, "_".join(modality))
    if cfg.data.dataset:
        checkpoint_name = "_".join([cfg.data.dataset, checkpoint_name])
    checkpoint = os.path.join(cfg.out_dir, cfg.model.checkpoint_dir, cfg.exp_name, checkpoint_name)
    os.makedirs(os.path.split(checkpoint)[0], exist_ok=True)

    shard = (rank, world) if world > 1 else None
    train_loader = create_dataloader(cfg, logger, modality, mode="train", device=device, prefetch=prefetch, shard=shard)
    val_loader = create_dataloader(cfg, logger, modality, mode="val", device=device, prefetch=prefetch, shard=shard)

    def plot(value, epoch, tag):
        if writer is not None:
            writer.add_scalar(tag, value, epoch)

    logger.info("Training in progress...")
    start_time = time.time()
    try:
        for epoch in range(start_epoch, epochs, 1):
            epoch_start_time = time.time()
            train_loss = train(cfg, model, train_loader, optimizer, lr_scheduler, criterion, epoch, logger, device)
            train_loss_hist.append(train_loss)
            if world > 1 and hasattr(model, "broadcast_buffers"):
                model.broadcast_buffers()       # before validation and the checkpoint: replica 0's running statistics
            logger.info("Validation in progress...")
            if cfg.val.enable:
                val_loss, val_acc, confusion_matrix = validate(cfg, model, val_loader, criterion, modality, logger, device)
                val_loss_hist.append(val_loss)
                for k in val_acc_hist.keys():
                    val_acc_hist[k].append(val_acc[k])
            else:
                val_loss = val_acc = confusion_matrix = None
            if lr_scheduler:
                if cfg.train.warmup.enable:
                    scheduler_warmup.step(epoch + 1)
                else:
                    lr_scheduler.step()
            if rank == 0:
                save_checkpoint(model, optimizer, epoch, train_loss_hist, val_loss_hist, val_acc_hist, confusion_matrix,
                                num_gpus, scheduler=lr_scheduler, filename=checkpoint + ".tmp")
                os.replace(checkpoint + ".tmp", checkpoint)     # a reader sees the old file or the new one, never half of one
            if world > 1:
                dist.barrier()
            plot(optimizer.param_groups[0]["lr"], epoch, "train/learning_rate")
            for k in train_loss.keys():
                plot(train_loss[k], epoch, f"train/{k}_loss")
                if cfg.val.enable:
                    plot(val_loss[k], epoch, f"val/{k}_loss")
            if cfg.val.enable:
                for cls, acc in val_acc.items():
                    for k, v in enumerate(acc):
                        plot(v, epoch, f"val/accuracy/{cls}_top_{cfg.val.topk[k]}")
            hours, minutes, seconds = get_time_diff(epoch_start_time, time.time())
            logger.info(LINE)
            logger.info(f"Epoch: [{epoch + 1}/{epochs}] || Learning Rate: {optimizer.param_groups[0]['lr']}")
            logger.info(f"Train_loss: {train_loss}")
            logger.info(f"Val_Loss: {val_loss}")
            logger.info(LINE)
            logger.info(f"Epoch Time: {hours} hours, {minutes} minutes, {seconds} seconds")
            logger.info(LINE)
            logger.info(f"Accuracy Top {cfg.val.topk}:")
            logger.info(json.dumps(val_acc, indent=2))
            logger.info(LINE)
    finally:
        train_loader.close()
        val_loader.close()
    hours, minutes, seconds = get_time_diff(start_time, time.time())
    logger.info(f"Training completed. Total time taken: {hours} hours, {minutes} minutes, {seconds} seconds")
