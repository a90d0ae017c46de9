"""Train-step shell on the MI355X: multi-tensor gradient clipping + SGD(momentum) or Adam in three launches.

Mirrors the reference loop body (core/tools/train.py:82-94) and its optimiser construction
(core/tools/train.py:190-202): `torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.train.clip_grad)`
followed by `optim.SGD(lr, momentum, weight_decay).step()`.  `FusedSGD` is a `torch.optim.Optimizer`, so
`MultiStepLR` / the warm-up scheduler of the reference drive it unchanged, and its `state_dict()` has torch's
layout (`momentum_buffer` per parameter).  No host synchronisation: the total norm and the clipping
coefficient stay on the device (`clip_grad_norm_` returns the norm as a 0-dim device tensor, like torch).
`FusedAdam` is the `optim.Adam` of the reference's other branch (core/tools/train.py:202-208) on the same launch scheme.
There is no CPU fallback: CPU tensors raise (`FusedAdam` over parameters that ALL live on the CPU is torch's Adam itself).
"""
import ctypes as C
import math

import torch

from ..._lib import AdamTensor, OptTensor, TbnHipError, call, lib, ptr, stream_ptr

MAX_TENSORS = 48   # TBN_OPT_MAX_TENSORS


def _check(p, g):
    if not (p.is_cuda and g.is_cuda):
        raise TbnHipError("fused optimiser: parameters and gradients must live on the GPU (no CPU fallback)")
    if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous() or not g.is_contiguous():
        raise TbnHipError("fused optimiser: contiguous fp32 parameters / gradients only")
    if g.is_sparse:
        raise TbnHipError("fused optimiser: sparse gradients are not supported")


def _entries(params, with_param, bufs=None):
    ents = []
    for i, p in enumerate(params):
        g = p.grad
        if g is None:
            continue
        _check(p, g)
        ents.append(OptTensor(ptr(p) if with_param else 0, ptr(g), ptr(bufs[i]) if bufs is not None else 0, p.numel()))
    return ents


def _chunks(ents, struct=OptTensor):
    for i in range(0, len(ents), MAX_TENSORS):
        part = ents[i:i + MAX_TENSORS]
        yield (struct * len(part))(*part), len(part)


def _sqnorm_coef(ents, max_norm, device):
    """-> (total_norm, coef) 1-element device tensors"""
    L = lib()
    arrs = list(_chunks(ents))
    counts = [L.tbn_opt_num_partials(a, n) for a, n in arrs]
    partials = torch.empty(max(1, sum(counts)), dtype=torch.float32, device=device)
    st, off = stream_ptr(), 0
    for (a, n), c in zip(arrs, counts):
        call("tbn_opt_sqnorm_partials", a, n, partials.data_ptr() + 4 * off, st)
        off += c
    out = torch.empty(2, dtype=torch.float32, device=device)
    call("tbn_opt_clip_coef", ptr(partials), off, float(max_norm), out.data_ptr(), out.data_ptr() + 4, st)
    return out[0], out[1:2]


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """Drop-in for `torch.nn.utils.clip_grad_norm_` (L2 only) on GPU gradients: scales them in place by
    min(1, max_norm / (total_norm + 1e-6)) and returns the total norm (0-dim device tensor, not synchronised)."""
    if float(norm_type) != 2.0:
        raise TbnHipError("clip_grad_norm_: only norm_type=2 is implemented on the HIP path")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    ents = _entries(params, False)
    total, coef = _sqnorm_coef(ents, max_norm, params[0].device)
    for a, n in _chunks(ents):
        call("tbn_opt_scale_grads", a, n, ptr(coef), stream_ptr())
    return total


class FusedSGD(torch.optim.Optimizer):
    """`torch.optim.SGD(params, lr, momentum, weight_decay)` (dampening 0, no Nesterov) as one multi-tensor HIP
    launch per step.  `step(clip_grad=max_norm)` additionally runs `clip_grad_norm_` (norm in `self.last_total_norm`,
    a device tensor) and is equivalent to the reference's `clip_grad_norm_(...)` + `optimizer.step()`
    (core/tools/train.py:84-94) in every schedule: the gradients are rescaled IN MEMORY, so what a later backward
    accumulates onto them (accumulator_step > 1, train.py:71-72) is what the reference accumulates onto.
    `step(clip_grad=max_norm, grads_consumed=True)` folds the clip coefficient into the update instead (gradients read
    once, NOT rescaled in memory: one launch and one pass over the gradients fewer) -- only for callers that clear the
    gradients before the next backward (accumulator_step == 1: `TrainStep`, `bench.py`); under accumulation it would
    silently differ from the reference, which is why it is opt-in."""

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedSGD: lr, momentum and weight_decay must be non-negative")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0,
                                      nesterov=False, maximize=False, foreach=None, differentiable=False,
                                      fused=None))
        self.last_total_norm = None

    @torch.no_grad()
    def step(self, closure=None, clip_grad=None, grads_consumed=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        gscale = None
        if clip_grad:
            allp = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
            if allp:
                ents = _entries(allp, False)
                self.last_total_norm, gscale = _sqnorm_coef(ents, clip_grad, allp[0].device)
                if not grads_consumed:
                    for a, n in _chunks(ents):
                        call("tbn_opt_scale_grads", a, n, ptr(gscale), stream_ptr())
                    gscale = None
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            mom = float(group["momentum"])
            bufs = None
            if mom != 0.0:
                bufs = []
                for p in params:
                    st = self.state[p]
                    if st.get("momentum_buffer") is None:
                        st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    bufs.append(st["momentum_buffer"])
            ents = _entries(params, True, bufs)
            for a, n in _chunks(ents):
                call("tbn_opt_sgd_step", a, n, float(group["lr"]), mom, float(group["weight_decay"]), ptr(gscale),
                     stream_ptr())
            # the kernel wrote the parameters (and momentum buffers) through raw pointers: tell autograd, as an in-place
            # torch op would have -- saved-tensor checks and every cache keyed on `_version` (the classifier's stacked
            # weight copy, core/models/model.py) rely on the counter
            torch.autograd.graph.increment_version(params)
            if bufs is not None:
                torch.autograd.graph.increment_version(bufs)
        return loss


class FusedAdam(torch.optim.Adam):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay)` (amsgrad off, coupled L2 decay: the reference's
    core/tools/train.py:202-208) as one multi-tensor HIP launch per step.  It IS a `torch.optim.Adam`: the per-parameter
    state is torch's (`step` a 0-dim float32 CPU tensor, `exp_avg` / `exp_avg_sq` zeros like the parameter), so
    `state_dict()` / `load_state_dict()` interchange with torch's optimiser in both directions.  `step` is counted per
    parameter as torch counts it: a parameter without a gradient is skipped and falls behind (Base_Audio under
    data.audio.dropout), and the two bias-correction factors go to the kernel per tensor, formed here in double.
    `step(clip_grad=, grads_consumed=)` has `FusedSGD.step`'s contract.  Nothing synchronises with the device: `step` lives
    on the host, the clip coefficient on the device.

    Parameters that ALL live on the CPU (the CPU rehearsals of `TrainStep`) take the base class's own step, after
    `torch.nn.utils.clip_grad_norm_` when `clip_grad` is set: that is torch's Adam, which this class is -- not a fallback to
    an oracle.  CPU parameters mixed with GPU ones raise, like every other tensor the kernel cannot take."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad=True is not implemented on the HIP path")
        if isinstance(lr, bool) or not isinstance(lr, (int, float)):
            raise ValueError("FusedAdam: lr must be a Python float (a tensor lr would be read back every step)")
        super().__init__(params, lr=float(lr), betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False)
        self.last_total_norm = None

    @torch.no_grad()
    def step(self, closure=None, clip_grad=None, grads_consumed=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        allp = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not allp:
            return loss
        if not any(p.is_cuda or p.grad.is_cuda for p in allp):
            if clip_grad:
                self.last_total_norm = torch.nn.utils.clip_grad_norm_(allp, clip_grad)
            super().step()
            return loss
        gscale = None
        if clip_grad:
            ents = _entries(allp, False)
            self.last_total_norm, gscale = _sqnorm_coef(ents, clip_grad, allp[0].device)
            if not grads_consumed:
                for a, n in _chunks(ents):
                    call("tbn_opt_scale_grads", a, n, ptr(gscale), stream_ptr())
                gscale = None
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            beta1, beta2 = (float(b) for b in group["betas"])
            lr = float(group["lr"])
            for p in params:      # refuse before any `step` advances
                _check(p, p.grad)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                _check(st["exp_avg"], st["exp_avg_sq"])
                if st["exp_avg"].shape != p.shape or st["exp_avg_sq"].shape != p.shape:
                    raise TbnHipError("FusedAdam: a loaded exp_avg / exp_avg_sq does not have its parameter's shape")
                if st["step"].is_cuda:
                    raise TbnHipError("FusedAdam: `step` lives on the device (a capturable / fused torch.optim.Adam state); "
                                      "reading it would synchronise every step")
            ents, moments = [], []
            for p in params:
                st = self.state[p]
                st["step"] += 1
                t = float(st["step"])
                ents.append(AdamTensor(ptr(p), ptr(p.grad), ptr(st["exp_avg"]), ptr(st["exp_avg_sq"]), p.numel(),
                                       lr / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t)))
                moments += [st["exp_avg"], st["exp_avg_sq"]]
            for a, n in _chunks(ents, AdamTensor):
                call("tbn_opt_adam_step", a, n, beta1, beta2, float(group["eps"]), float(group["weight_decay"]),
                     ptr(gscale), stream_ptr())
            # raw-pointer writes: tell autograd, as FusedSGD.step does
            torch.autograd.graph.increment_version(params)
            torch.autograd.graph.increment_version(moments)
        return loss
