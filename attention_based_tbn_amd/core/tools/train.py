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
    anything with `add_scalar(tag, value, epoch)` -- the reference's `Plotter` tags without a tensorboard import.
"""
import json
import os
import time

import torch

from ..models import build_model
from ..utils import (DeviceMetric, TrainStep, build_optimizer, create_dataloader, get_time_diff, load_checkpoint,
                     save_checkpoint)

LINE = "----------------------------------------------------------"


def train(cfg, model, data_loader, optimizer, scheduler, criterion, epoch, logger, device=torch.device("cuda")):
    """one epoch (reference :24-105) -> train_loss, the loss dictionary of `DeviceMetric.get_metrics`"""
    no_batches = round(len(data_loader.dataset) / data_loader.batch_size)
    log_interval = max(1, no_batches // 4)
    metric = DeviceMetric(cfg, no_batches, device)
    step = TrainStep.from_config(cfg, model, optimizer, criterion)
    model.train()
    for iter_no, (data, target) in enumerate(data_loader):
        loss, batch_size = step(iter_no, data, target, epoch)
        metric.set_metrics(step.last_out, target, batch_size, loss)
        if iter_no == 0 or (iter_no + 1) % log_interval == 0:
            if step.last_total_norm is not None:
                total_norm = float(step.last_total_norm)
                if total_norm > cfg.train.clip_grad:
                    logger.info(f"Clipping gradient: {total_norm} with coef {cfg.train.clip_grad / total_norm}")
            logger.info("Batch Progress: [{}/{}] || Train Loss: {:.5f}".format(
                (iter_no + 1), no_batches, metric.running("total") / (iter_no + 1)))
    train_loss, _, _ = metric.get_metrics()
    return train_loss


def validate(cfg, model, data_loader, criterion, modality, logger, device=torch.device("cuda")):
    """reference :108-159 -> (val_loss, val_acc, conf_mat)"""
    no_batches = len(data_loader.dataset) // data_loader.batch_size
    metric = DeviceMetric(cfg, no_batches, device)
    model.eval()
    with torch.no_grad():
        for data, target, _ in data_loader:
            out = model(data)
            loss, batch_size = model.get_loss(criterion, target, out)
            metric.set_metrics(out, target, batch_size, loss)
    return metric.get_metrics()


def run_trainer(cfg, logger, modality, writer=None, *, prefetch=2):
    """reference :162-357: model, optimiser, resume, loaders, the epoch loop, one checkpoint per epoch"""
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
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

    train_loader = create_dataloader(cfg, logger, modality, mode="train", device=device, prefetch=prefetch)
    val_loader = create_dataloader(cfg, logger, modality, mode="val", device=device, prefetch=prefetch)

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
            save_checkpoint(model, optimizer, epoch, train_loss_hist, val_loss_hist, val_acc_hist, confusion_matrix,
                            num_gpus, scheduler=lr_scheduler, filename=checkpoint)
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
