"""Evaluation metrics of the reference (`core/utils/metric.py:4-157`) with the per-batch top-k correctness and
confusion matrix computed by one HIP launch per class head (`tbn_topk_correct`) instead of `topk` + a Python loop
over the batch that indexes the device matrix element by element.

`DeviceMetric` is the same bookkeeping without the per-batch host round trips: one `tbn_metric_update` launch per batch
writes the batch's hit counts and loss terms into a device ring that the host reads once, in `get_metrics`."""
import ctypes

import numpy as np
import torch

from ..._lib import MetricHead, TbnHipError, call, ptr, stream_ptr


def get_correct_score(out, target, topk, device=None):
    """`Metric._get_correct_score` (reference metric.py:137-157): (correct (maxk, B) bool, conf_mat (C, C) float)"""
    if not out.is_cuda:
        raise TbnHipError("metrics: class scores must be on the GPU (no CPU fallback)")
    out = out.detach().float().contiguous()
    target = target.to(device=out.device, dtype=torch.long).contiguous().view(-1)
    B, Cn = out.shape
    maxk = max(topk)
    correct = torch.empty((maxk, B), dtype=torch.uint8, device=out.device)
    conf = torch.zeros((Cn, Cn), dtype=torch.float32, device=out.device)
    call("tbn_topk_correct", ptr(out), Cn, ptr(target), B, Cn, maxk, ptr(correct), 0, ptr(conf), stream_ptr())
    return correct.bool(), conf


class Metric(object):
    """Same constructor, `set_metrics` / `get_metrics` and rounding as the reference class."""

    def __init__(self, cfg, no_batches, device=torch.device("cuda")):
        self.cfg = cfg
        self.topk = list(cfg.val.topk)
        self.device = device
        self.no_batches = no_batches
        self.multi_class = len(list(cfg.model.num_classes.keys())) > 1
        self.loss, self.accuracy, self.conf_mat = {}, {}, {}
        for key, no_cls in cfg.model.num_classes.items():
            self.accuracy[key] = [0] * len(self.topk)
            self.conf_mat[key] = torch.zeros((no_cls, no_cls), device=device)
            self.loss[key] = 0
        if self.multi_class:
            self.loss["all_class"] = 0
            self.accuracy["all_class"] = [0] * len(self.topk)
        att = cfg.model.attention
        if att.enable and not att.use_fixed:
            if att.use_prior:
                self.loss["prior"] = 0
            if att.use_contrast:
                self.loss["contrast"] = 0
            if att.use_entropy:
                self.loss["entropy"] = 0
        self.loss["total"] = 0

    def set_metrics(self, out, target, batch_size, batch_loss):
        correct = {}
        if self.multi_class:
            correct["all_class"] = []
        for key in out.keys():
            if key == "weights":
                continue
            corr, cm = get_correct_score(out[key], target["class"][key], self.topk, self.device)
            self.conf_mat[key] += cm
            correct[key] = corr
            if self.multi_class:
                correct["all_class"].append(corr)
            self.loss[key] += batch_loss[key].item()
        if self.multi_class:
            self.loss["all_class"] += batch_loss["all_class"].item()
        att = self.cfg.model.attention
        if att.enable and not att.use_fixed:
            for k, on in (("prior", att.use_prior), ("contrast", att.use_contrast), ("entropy", att.use_entropy)):
                if on:
                    self.loss[k] += batch_loss[k].item()
        self.loss["total"] += batch_loss["total"].item()
        for key in self.accuracy.keys():
            for i, k in enumerate(self.topk):
                if key == "all_class":
                    c = correct[key][0][:k].sum(0)
                    for c2 in correct[key][1:]:
                        c = c * c2[:k].sum(0)   # a clip counts when every class head is right within its top k
                    acc = float(c.to(torch.float32).sum().mul_(100.0 / batch_size))
                else:
                    acc = float(correct[key][:k].reshape(-1).to(torch.float32).sum().mul_(100.0 / batch_size))
                self.accuracy[key][i] += acc

    def get_metrics(self):
        for key in self.accuracy.keys():
            self.accuracy[key] = [round(x / self.no_batches, 2) for x in self.accuracy[key]]
        for key in self.loss.keys():
            self.loss[key] = round(self.loss[key] / self.no_batches, 5)
        return self.loss, self.accuracy, self.conf_mat


class DeviceMetric(Metric):
    """`Metric` (same constructor, `set_metrics` / `get_metrics`, same values) whose `set_metrics` never makes the host
    wait for the device: ONE `tbn_metric_update` launch adds the batch's per-head and all-heads hit counts for every k
    into row i of a zero-initialised int32 ring and copies the loss terms (device scalars) into row i of a float ring;
    the per-head confusion matrices are updated by the same launch.  `get_metrics` copies the rings once and redoes the
    reference's arithmetic on the host, batch by batch in order: accuracy terms `float32(hits) * float32(100 / B)`
    summed as Python floats, loss terms as the float32 values summed as Python floats, then the reference's rounding.
    A ring of `max(8, no_batches + 1)` rows that fills up is folded into the host sums with one synchronisation and
    reused.  Loss entries that are Python numbers stay on the host.  `running(key)` (one synchronisation) serves
    progress lines."""

    def __init__(self, cfg, no_batches, device=torch.device("cuda")):
        super().__init__(cfg, no_batches, device)
        self._heads = list(cfg.model.num_classes.keys())
        self._loss_keys = list(self.loss.keys())
        self._nk = len(self.topk)
        self._topk = (ctypes.c_int * self._nk)(*[int(k) for k in self.topk])
        self._cap = max(8, int(no_batches) + 1)
        self._hits = torch.zeros((self._cap, (len(self._heads) + 1) * self._nk), dtype=torch.int32, device=device)
        self._loss_ring = torch.zeros((self._cap, max(1, len(self._loss_keys))), dtype=torch.float32, device=device)
        self._pending = []          # per ring row: (batch_size, keys of the device losses in column order, {key: host loss})
        self._acc = {key: [0] * self._nk for key in self.accuracy}
        self._loss_sum = {key: 0 for key in self.loss}

    def set_metrics(self, out, target, batch_size, batch_loss):
        keys = [k for k in out.keys() if k != "weights"]
        if keys != self._heads:
            raise ValueError(f"DeviceMetric: the model's class heads {keys} are not cfg.model.num_classes' {self._heads}")
        if len(self._pending) == self._cap:
            self._flush()
        row = len(self._pending)
        heads = (MetricHead * len(keys))()
        keep = []                   # converted copies live until the launch is queued
        for h, key in enumerate(keys):
            scores = out[key]
            if not scores.is_cuda:
                raise TbnHipError("metrics: class scores must be on the GPU (no CPU fallback)")
            scores = scores.detach()
            if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1 or scores.stride(0) < scores.shape[1]:
                scores = scores.float().reshape(scores.shape[0], -1).contiguous()
            tgt = target["class"][key].to(device=scores.device, dtype=torch.long).contiguous().view(-1)
            conf = self.conf_mat[key]
            if scores.shape[0] != tgt.numel() or tuple(conf.shape) != (scores.shape[1], scores.shape[1]):
                raise ValueError(f"DeviceMetric: head {key!r}: scores {tuple(scores.shape)}, {tgt.numel()} targets, "
                                 f"confusion matrix {tuple(conf.shape)}")
            keep += [scores, tgt]
            heads[h] = MetricHead(ptr(scores), scores.stride(0), scores.shape[1], ptr(tgt), ptr(conf))
        batch = keep[0].shape[0]
        if any(scores.shape[0] != batch for scores in keep[0::2]):
            raise ValueError("DeviceMetric: the heads' scores differ in batch size")
        on_device, on_host = [], {}
        for key in self._loss_keys:
            v = batch_loss[key]
            if isinstance(v, torch.Tensor):
                v = v.detach().reshape(-1)[:1].to(device=self._hits.device, dtype=torch.float32)
                keep.append(v)
                on_device.append(key)
            else:
                on_host[key] = float(v)
        ptrs = (ctypes.c_void_p * max(1, len(on_device)))(*[ptr(t) for t in keep[2 * len(keys):]])
        call("tbn_metric_update", heads, len(keys), batch, self._topk, self._nk, ptrs, len(on_device),
             ptr(self._hits[row]), ptr(self._loss_ring[row]), stream_ptr())
        self._pending.append((batch_size, on_device, on_host))

    def _fold(self, hits, losses):
        """the pending rows (host copies of the rings) into the host sums, in batch order"""
        for row, (batch_size, on_device, on_host) in enumerate(self._pending):
            scale = np.float32(100.0 / batch_size)
            groups = self._heads + ["all_class"]
            for g, key in enumerate(groups):
                if key in self._acc:
                    for j in range(self._nk):
                        self._acc[key][j] += float(np.float32(hits[row, g * self._nk + j]) * scale)
            for col, key in enumerate(on_device):
                self._loss_sum[key] += float(np.float32(losses[row, col]))
            for key, v in on_host.items():
                self._loss_sum[key] += v

    def _flush(self):
        n = len(self._pending)
        if n == 0:
            return
        # one copy, one synchronisation: the float ring travels as its bit patterns beside the counts
        both = torch.cat([self._hits[:n], self._loss_ring[:n].view(torch.int32)], 1).cpu()
        width = self._hits.shape[1]
        self._fold(both[:, :width].numpy(), both[:, width:].contiguous().view(torch.float32).numpy())
        self._pending = []
        self._hits.zero_()

    def running(self, key="total"):
        """the sum so far of one loss term (one synchronisation): what a progress line divides by its batch count"""
        total = self._loss_sum[key]
        n = len(self._pending)
        if n:
            losses = self._loss_ring[:n].cpu().numpy()
            for row, (_, on_device, on_host) in enumerate(self._pending):
                if key in on_host:
                    total += on_host[key]
                else:
                    total += float(np.float32(losses[row, on_device.index(key)]))
        return total

    def get_metrics(self):
        self._flush()
        self.accuracy = {key: [round(x / self.no_batches, 2) for x in acc] for key, acc in self._acc.items()}
        self.loss = {key: round(x / self.no_batches, 5) for key, x in self._loss_sum.items()}
        return self.loss, self.accuracy, self.conf_mat
