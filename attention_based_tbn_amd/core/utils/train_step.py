"""The body of the reference's training loop for ONE iteration, gradient accumulation included.

Reference: core/tools/train.py:66-94.  With `accumulator_step = k` (cfg.train.optim.accumulator_step) iteration
`it` of an epoch does, in this order,

    (it + 1) % k == 0        -> optimizer.zero_grad()                      (:71-72, BEFORE the forward)
    out = model(data); loss, B = model.get_loss(criterion, target, out, epoch)
    loss["total"] /= k                                                      (:79)
    loss["total"].backward()                                                (:81)
    cfg.train.clip_grad      -> clip_grad_norm_(model.parameters(), clip)   (:84-91, EVERY iteration, in place, on
                                                                             whatever has ACCUMULATED in .grad so far)
    (it + 1) % k == k - 1    -> optimizer.step()                            (:93-94)

so for k = 2 the optimiser steps after iterations 0, 2, 4, ... and the gradients are cleared in front of iterations
1, 3, 5, ... -- the very first step of an epoch is taken on one micro-batch, and a gradient that was clipped in
iteration i is clipped AGAIN (together with what iteration i + 1 added) before the step.  `TrainStep` reproduces exactly
that schedule; nothing is "fixed".

MI355X side: for k == 1 the clip is folded into the fused optimiser launch (`FusedSGD.step(clip_grad=)` and
`FusedAdam.step(clip_grad=)` alike: the gradients are read once and not rescaled in memory -- legal because the next thing
that happens to them is `zero_grad`); for k > 1 the
clipped gradients must persist into the next iteration, so the in-place multi-tensor `clip_grad_norm_` runs every
iteration and `step()` on the stepping ones.

Data parallel (`core.models.DataParallel`, one process per GPU): the reference's nn.DataParallel reduces the replicas'
gradients into the master copy on EVERY backward, and its per-iteration clip sees that global accumulated gradient.
  * clip_grad off: accumulation is linear, so the non-stepping iterations run under `DataParallel.no_sync()` and the
    stepping iteration's all-reduce averages the locally accumulated sums -- one gradient exchange per optimiser step.
    Parameters that a replica may leave without a gradient in some iteration (the audio branch under
    `data.audio.dropout > 0`, reference model.py:215-222) are part of that exchange with whatever each rank accumulated:
    `DataParallel.finish_gradient_sync` sends a rank's existing .grad (zeros where it has none) and only reports "no
    gradient" when NO rank holds one (tests/test_host_cpu.py::test_accumulation_with_optional_branch_gloo_world2);
  * clip_grad on: the clip coefficient is a function of the norm of the GLOBAL accumulated gradient, which no rank can
    form from local data, so every iteration synchronises (avg_r(G + g_r) = G + avg_r(g_r): the previously synchronised
    part G is identical on all ranks) -- identical to the reference, at the reference's own communication volume.
"""
import collections
import contextlib

import torch

from .optim import FusedAdam, FusedSGD, clip_grad_norm_


class TrainStep:
    def __init__(self, model, optimizer, criterion, accumulator_step=1, clip_grad=None):
        if int(accumulator_step) < 1:
            raise ValueError("TrainStep: accumulator_step must be >= 1")
        self.model = model
        self.optimizer = optimizer
        self.criterion = criterion
        self.k = int(accumulator_step)
        self.clip_grad = clip_grad if clip_grad else None    # reference: `if cfg.train.clip_grad:`
        self.last_total_norm = None     # 0-dim device tensor of the last clip (None when clipping is off)
        self.last_out = None            # the model's output dict of the last call (what a metric is fed with)
        self.last_scale = None          # (mean factor, sum factor) the last call applied for its share; see __call__
        self.last_scale_on = None       # "gradient" (DataParallel weighs the finished gradients) / "loss" / None
        # did the backward of the last iterations exchange gradients (data parallel only)?  Bounded: a run has millions
        self.synced = collections.deque(maxlen=64)

    @classmethod
    def from_config(cls, cfg, model, optimizer, criterion):
        return cls(model, optimizer, criterion, cfg.train.optim.accumulator_step, cfg.train.clip_grad)

    def zeroes(self, iter_no):
        return (iter_no + 1) % self.k == 0

    def steps(self, iter_no):
        return (iter_no + 1) % self.k == self.k - 1

    def _sync_context(self, iter_no):
        no_sync = getattr(self.model, "no_sync", None)
        if no_sync is None or self.clip_grad is not None or self.steps(iter_no):
            self.synced.append(True)
            return contextlib.nullcontext()
        self.synced.append(False)
        return no_sync()

    def _shared_total(self, loss, share, epoch):
        """what is back-propagated in place of loss["total"] when this rank holds `share = (n_r, n, W)` of a global batch:
        every term times the factor that makes `DataParallel`'s average of the ranks' gradients the gradient of the loss
        ONE process computes on the n clips.  `None` / W == 1 / nothing to scale -> loss["total"] itself (the same
        object: the step is bit-identical to the unshared one).  With k == 1 under an active `DataParallel` the mean
        factor is handed to the wrapper instead (`weigh_next_backward`: on the finished gradients, right before they are
        exchanged) and only what the sum term needs beyond it stays on the loss; `last_scale_on` says which."""
        self.last_scale, self.last_scale_on = None, None
        weigh = getattr(self.model, "weigh_next_backward", None) if getattr(self.model, "active", False) else None
        if weigh is not None:
            weigh(None)         # a weight left behind by a backward that never came
        if share is None:
            return loss["total"]
        n_r, n, world = (int(v) for v in share)
        if world < 1 or not 0 < n_r <= n:
            raise ValueError(f"TrainStep: share {share!r} is not (n_r, n, W) with 0 < n_r <= n")
        if world == 1:
            return loss["total"]
        mean = None if n_r * world == n else n_r * world / n      # equal shares: exactly 1, and not multiplied in
        bare = getattr(self.model, "module", self.model)
        att = bare.cfg.model.attention
        sum_term = None
        if (att.enable and not att.use_fixed and att.use_prior and att.loss_reduction == "sum"
                and torch.is_tensor(loss.get("prior"))):
            # the multiplier get_loss gave the prior term (model.py: 0 before decay_step while training)
            mult = 0 if (bare.training and epoch + 1 < att.decay_step) else att.wt_decay
            if mult:
                sum_term = mult * loss["prior"] / self.k
        self.last_scale = (mean, world if sum_term is not None else None)
        total = loss["total"]
        if weigh is not None and self.k == 1:
            # .grad holds nothing when this backward starts (zero_grad precedes every forward) and the backward is a
            # synchronised one: the wrapper multiplies the finished gradients by the mean factor, and the sum term gets
            # on the loss what it still lacks, W / mean in all
            self.last_scale_on = "gradient"
            weigh(mean)
            if sum_term is not None:
                total = total + (world / (1.0 if mean is None else mean) - 1.0) * sum_term
            return total
        self.last_scale_on = "loss"
        if mean is not None:
            total = total * mean
        if sum_term is not None:
            total = total + (world - (1.0 if mean is None else mean)) * sum_term
        return total

    def __call__(self, iter_no, data, target, epoch=0, share=None):
        """one iteration of the reference loop -> (loss dict, batch_size); loss["total"] is already divided by k, as the
        reference's metric bookkeeping sees it (train.py:79-80).

        `share=(n_r, n, W)` (`ClipLoader.share`; None: today's step): this rank's `data` is n_r clips of a global batch
        of n spread over W ranks.  `DataParallel` AVERAGES the ranks' gradients, so a term t whose reduction is a MEAN
        over clips has to enter the exchange with the factor `n_r W / n` -- avg_r of that is sum_r (n_r / n) grad t_r, the
        gradient of the mean over all n clips -- and a term reduced by a SUM over clips with `W` (avg_r W grad t_r =
        sum_r grad t_r).
        In `TBNModel.get_loss`:
          mean  every class head's cross entropy (nn.CrossEntropyLoss()); the entropy term (`.mean()` always); the contrast
                term (ContrastLoss "mean" / "batchmean": a mean over the b*n weight rows); the prior term under
                `loss_reduction` "mean" and "batchmean" (a sum divided by b*n*T or b*n);
          sum   the prior term under `loss_reduction="sum"` (ContrastLoss "sum" is an unreduced vector that cannot be
                back-propagated, here as in the reference).
        With equal shares (n_r W == n) the mean factor is exactly 1 and is NOT multiplied in: without a sum term
        loss["total"] itself is back-propagated and the step is bit-identical to the unshared one.
        Where the factor goes.  A factor on the loss that is no power of two makes every product of the backward pass
        round differently, and a gradient that is a small sum of large cancelling contributions shows it: measured on a
        1 + 2 split, `pe.2.bias` moved by 3e-5 ... 1e-4 of its max-norm on ONE rank, no exchange involved, every other
        tensor by less than 7e-6.  So with k == 1 under an active `DataParallel` -- `.grad` holds nothing when the
        backward starts -- the mean factor goes on the FINISHED gradients instead: `DataParallel.weigh_next_backward`
        multiplies each tensor once, right before its collective (buckets inside backward included); the backward pass is
        the unshared one bit for bit, and only the sum term keeps a factor on the loss, `W / mean` in all.  With k > 1 a
        micro-batch's gradient cannot be told from what has accumulated, and without the wrapper nothing is exchanged:
        there both factors go on loss["total"] before `backward()` (`last_scale_on`: "gradient" / "loss").
        The returned dictionary holds this rank's un-scaled terms (what the
        reference's bookkeeping sees; `DeviceMetric` weighs them by n_r / n when it merges).  `last_scale` =
        (mean factor or None, sum factor or None) of the last call, None without a share.
        Two things stay per replica, as under the reference's nn.DataParallel: BatchNorm's batch statistics, and -- unlike
        there, where the loss sees the gathered output -- the entropy term's switch-off below `entropy_thresh`, which
        looks at this rank's entropy."""
        if self.zeroes(iter_no):
            self.optimizer.zero_grad()
        with self._sync_context(iter_no):
            out = self.last_out = self.model(data)
            loss, batch_size = self.model.get_loss(self.criterion, target, out, epoch)
            loss["total"] = loss["total"] / self.k
            self._shared_total(loss, share, epoch).backward()
        fused = isinstance(self.optimizer, (FusedSGD, FusedAdam)) and self.k == 1 and self.clip_grad is not None
        if self.clip_grad is not None and not fused:
            params = [p for p in self.model.parameters() if p.grad is not None]
            if params and params[0].grad.is_cuda:
                self.last_total_norm = clip_grad_norm_(params, self.clip_grad)
            else:       # CPU rehearsals of the schedule (gloo tests): torch's own
                self.last_total_norm = torch.nn.utils.clip_grad_norm_(params, self.clip_grad)
        if self.steps(iter_no):
            if fused:
                self.optimizer.step(clip_grad=self.clip_grad, grads_consumed=True)
                self.last_total_norm = self.optimizer.last_total_norm
            else:
                self.optimizer.step()
        return loss, batch_size
