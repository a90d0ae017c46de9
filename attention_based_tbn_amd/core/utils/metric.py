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
    progress lines.

    `process_group=` (None: no merge, the class as above; `torch.distributed.group.WORLD` for the default group) makes
    the metric one of W, one per rank of a data-parallel job whose ranks each hold a share of every global batch
    (`ClipLoader(shard=)`).  `set_metrics(..., share=(n_r, n[, W]), row=i)` then files the batch under global batch i
    (`ClipLoader.batch_no`; default: the next row) with this rank's n_r of its n clips; a global batch this rank had no
    share of is simply never filed and counts as a zero row with n_r = 0.  `set_metrics` launches and synchronises
    exactly as without a group, and a ring flush stays local.  `get_metrics` merges, with THREE collectives however many
    batches there were (the row count by MAX; one float64 table of every row's hit counts, weighted loss terms and
    clip counts by SUM -- counts below 2^53 are exact there; the confusion matrices, concatenated, by SUM): per global
    batch the hit counts are summed as integers, each loss term is combined as sum_r (n_r / n) loss_r in float64 (the
    mean over the n clips of a term that is a mean over clips; a rank that holds the whole batch contributes its float32
    value exactly), and the reference's arithmetic is redone with n as the batch size: `float32(hits) * float32(100 / n)`
    and the loss terms summed as Python floats in batch order, then the rounding.  Every rank returns equal
    dictionaries and confusion matrices (fresh tensors; `self.conf_mat` stays this rank's own).  A prior term under
    `loss_reduction="sum"` is weighed like the others, so its entry is the clip-weighted mean of the ranks' sums, not
    their sum.  `running(key)` stays LOCAL: this rank's un-weighted sum, fit for a progress line and nothing else."""

    def __init__(self, cfg, no_batches, device=torch.device("cuda"), process_group=None):
        super().__init__(cfg, no_batches, device)
        self.process_group = process_group
        self._rows = {}             # merging only: global batch -> (n_r, n, int64 hit counts, {loss key: float})
        self._next_row = 0
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

    def set_metrics(self, out, target, batch_size, batch_loss, *, share=None, row=None):
        keys = [k for k in out.keys() if k != "weights"]
        if keys != self._heads:
            raise ValueError(f"DeviceMetric: the model's class heads {keys} are not cfg.model.num_classes' {self._heads}")
        where = None
        if self.process_group is not None:
            if share is None:
                raise ValueError("DeviceMetric: with a process group every batch needs share=(n_r, n)")
            n_r, n = int(share[0]), int(share[1])
            row = self._next_row if row is None else int(row)
            if not 0 < n_r <= n or row < self._next_row:
                raise ValueError(f"DeviceMetric: share {share!r} / row {row} (next row {self._next_row})")
            self._next_row = row + 1
            where = (row, n_r, n)
        elif share is not None and int(share[0]) != int(share[1]):
            raise ValueError(f"DeviceMetric: share {share!r} of a batch needs process_group= to be merged")
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
        self._pending.append((batch_size, on_device, on_host, where))

    def _fold(self, hits, losses):
        """the pending rows (host copies of the rings) into the host sums, in batch order"""
        for row, (batch_size, on_device, on_host, where) in enumerate(self._pending):
            if where is not None:       # kept row by row for the merge; the local sums below serve `running` only
                terms = {key: float(np.float32(losses[row, col])) for col, key in enumerate(on_device)}
                terms.update(on_host)
                self._rows[where[0]] = (where[1], where[2], hits[row].astype(np.int64), terms)
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
            for row, (_, on_device, on_host, _) in enumerate(self._pending):
                if key in on_host:
                    total += on_host[key]
                else:
                    total += float(np.float32(losses[row, on_device.index(key)]))
        return total

    def merge(self):
        """-> (accuracy sums, loss sums, confusion matrices) of the GLOBAL batches, equal on every rank: the three
        collectives of the class docstring.  Every rank of the group must call it (through `get_metrics`)."""
        import torch.distributed as dist
        group = self.process_group
        on_device = dist.get_backend(group) == "nccl"       # RCCL moves device tensors only

        def reduced(t, op):
            t = t.to(self._hits.device) if on_device else t
            dist.all_reduce(t, op=op, group=group)
            return t.cpu()

        rows = int(reduced(torch.tensor([max(self._rows) + 1 if self._rows else 0], dtype=torch.int64), dist.ReduceOp.MAX))
        nh, nl = self._hits.shape[1], len(self._loss_keys)
        acc = {key: [0] * self._nk for key in self._acc}
        loss_sum = {key: 0 for key in self._loss_sum}
        if rows:
            table = np.zeros((rows, nh + nl + 3), dtype=np.float64)     # hits | (n_r / n) loss | n_r, n, ranks with a share
            for row, (n_r, n, hits, terms) in self._rows.items():
                table[row, :nh] = hits
                table[row, nh:nh + nl] = [n_r / n * terms[key] for key in self._loss_keys]
                table[row, nh + nl:] = (n_r, n, 1)
            table = reduced(torch.from_numpy(table), dist.ReduceOp.SUM).numpy()
            groups = self._heads + ["all_class"]
            for row in range(rows):
                n_sum, n_times, holders = table[row, nh + nl:]
                if holders == 0:
                    continue            # a global batch nobody filed
                n = int(round(n_times / holders))
                if n * holders != n_times or n_sum != n:
                    raise RuntimeError(f"DeviceMetric.merge: global batch {row}: the ranks' shares add up to {int(n_sum)} "
                                       f"clips of {n_times / holders:g}")
                scale = np.float32(100.0 / n)
                for g, key in enumerate(groups):
                    if key in acc:
                        for j in range(self._nk):
                            acc[key][j] += float(np.float32(table[row, g * self._nk + j]) * scale)
                for col, key in enumerate(self._loss_keys):
                    loss_sum[key] += float(table[row, nh + col])
        keys = list(self.conf_mat.keys())
        flat = torch.cat([self.conf_mat[key].reshape(-1) for key in keys])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        conf, at = {}, 0
        for key in keys:
            size = self.conf_mat[key].numel()
            conf[key] = flat[at:at + size].view_as(self.conf_mat[key])
            at += size
        return acc, loss_sum, conf

    def get_metrics(self):
        self._flush()
        acc, loss_sum, conf = (self._acc, self._loss_sum, self.conf_mat) if self.process_group is None else self.merge()
        self.accuracy = {key: [round(x / self.no_batches, 2) for x in a] for key, a in acc.items()}
        self.loss = {key: round(x / self.no_batches, 5) for key, x in loss_sum.items()}
        return self.loss, self.accuracy, conf
