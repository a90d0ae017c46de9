"""Operator-level autograd wrappers for conv / BatchNorm networks on NHWC tensors (HIP only -- no CPU fallback): what a
backbone the engine does not know is composed from (core/models/resnet.py, vgg.py, bn_inception_audio.py).

  fused units
    conv_bn_act         conv (1x1 / 3x3, stride 1 / 2, cin a multiple of 32) [+ bias] + BatchNorm + optional residual +
                        optional ReLU
    residual_block      a whole BasicBlock / Bottleneck as ONE autograd node: its backward pass lets the identity path and
                        conv1's data gradient meet in the block input's gradient buffer through the `accumulate` arguments
                        of tbn_bn_res_bwd / tbn_conv2d_dgrad instead of a separate add
    conv_bias_act       conv + bias + optional ReLU without BatchNorm
  stems and first layers (straight from NCHW frames, no input gradient)
    stem_bn_pool        7x7 / stride 2 / pad 3 conv + BatchNorm + ReLU + MaxPool(3, 2, 1)
    audio_stem_bn_pool  the separable 1x3 | 3x1 / stride 2 audio stem + two BatchNorms + ReLU + MaxPool(3, 2, ceil)
    first_conv3         3x3 / stride 1 / pad 1 conv to 64 channels, plain (bias + ReLU) or with BatchNorm
  pools
    maxpool3, avgpool3  the 3x3 pools of the inception blocks
    maxpool2            MaxPool2d(2, 2), optionally carrying the ReLU mask of the conv in front of it in its backward
    adaptive_avgpool7_flat  AdaptiveAvgPool2d((7, 7)) + flatten in the NCHW order a classifier's weight expects
  means
    global_mean         AdaptiveAvgPool2d(1) + flatten
    freq_mean           the mean over the frequency axis alone

Training: tbn_conv2d_fwd epilogue 1 (bias-free output + statistics partials), then tbn_bn_fwd_batch (no residual, ReLU,
at most 1024 channels) or tbn_bn_res_fwd (the join: residual and / or no ReLU and / or more channels).  Eval: running
statistics folded into the conv's epilogue 2, the join through epilogue 0 + tbn_bn_res_apply.  Everything launches on the
current stream.  Parameters keep torch's OIHW shape (checkpoints interchange); the kernels read [cout][k][k][cin], a copy
cached on the parameter's `_version`.
"""
import ctypes as C

import torch

from ._lib import BnBwdDesc, BnFwdDesc, BnSeg, call, lib, ptr, stream_ptr, TbnHipError

MOMENTUM = 0.1
EPS = 1e-5


class BnState:
    """what a unit needs beside its parameters: geometry, the BatchNorm buffers, and the two caches of the unit"""
    __slots__ = ("stride", "pad", "running_mean", "running_var", "wcache", "fcache")

    def __init__(self, stride, pad, running_mean, running_var):
        self.stride, self.pad = stride, pad
        self.running_mean, self.running_var = running_mean, running_var
        self.wcache, self.fcache = {}, {}      # kernel_weight / folded_bn


def _need_cuda(t, what):
    if not t.is_cuda:
        raise TbnHipError(f"{what}: tensor is on {t.device}; the TBN hot path only runs on an MI355X "
                          "(HIP) device -- there is no CPU fallback")


def _f32c(t):
    t = t.contiguous()
    return t if t.dtype == torch.float32 else t.float()


def _new(ref, *shape, dtype=torch.float32):
    return torch.empty(*shape, device=ref.device, dtype=dtype)


def _bias_f32(bias):
    return _f32c(bias.detach()) if bias is not None else None


def _zero_bias_grad(ref, c):
    """a per-channel constant in front of a batch-statistics BatchNorm has exactly zero gradient"""
    return torch.zeros(c, device=ref.device, dtype=torch.float32)


def _rows(stats):
    """the pointers of the four rows of a (4, c) statistics tensor: batch mean | 1/std | scale | shift"""
    return tuple(stats[i].data_ptr() for i in range(4))


def _wrote_running(state):
    """the kernels wrote the running buffers behind autograd's back: tell the caches keyed on `_version` (folded_bn)"""
    if state.running_mean is not None:
        torch.autograd.graph.increment_version((state.running_mean, state.running_var))


def _adopt_state(state, stride, pad, running=None):
    """a fresh BnState, or the caller's with the geometry (and the running buffers, when given) of this call"""
    if state is None:
        return BnState(stride, pad, *(running or (None, None)))
    state.stride, state.pad = stride, pad
    if running is not None:
        state.running_mean, state.running_var = running
    return state


def kernel_weight(weight, cache):
    """an OIHW conv weight in the kernels' [cout][k][k][cin] order.  k = 1 or cin = 1: the same memory, no copy.
    Otherwise a permuted copy kept in `cache` until the parameter changes (`_version`: optimiser steps bump it)."""
    cout, cin, k, _ = weight.shape
    w = weight.detach()
    if (k == 1 or cin == 1) and w.is_contiguous() and w.dtype == torch.float32:
        return w.view(cout, k, k, cin)
    key = (weight.data_ptr(), weight._version)
    if cache.get("key") != key:
        buf = cache.get("buf")
        if buf is None or tuple(buf.shape) != (cout, k, k, cin) or buf.device != w.device:
            buf = cache["buf"] = _new(w, cout, k, k, cin)
        buf.copy_(w.permute(0, 2, 3, 1))
        cache["key"] = key
    return cache["buf"]


def _oihw(dwk):
    """weight gradient [cout][k][k][cin] -> the parameter's OIHW shape (a view)"""
    return dwk.permute(0, 3, 1, 2)


def folded_bn(gamma, beta, state, bias=None):
    """(2, c): scale = gamma / sqrt(var + eps) | shift = beta - mean * scale (with a conv bias: beta + (bias - mean) *
    scale), folded once and kept until one of the tensors changes (`_version`)"""
    rm, rv = state.running_mean, state.running_var
    key = tuple((t.data_ptr(), t._version) for t in (gamma, beta, rm, rv) + (() if bias is None else (bias,)))
    cache = state.fcache
    if cache.get("key") != key:
        sc = gamma.detach().float() / torch.sqrt(rv.float() + EPS)
        mean = rm.float() if bias is None else rm.float() - bias.detach().float()
        cache["ss"] = torch.stack([sc, beta.detach().float() - mean * sc]).contiguous()
        cache["key"] = key
    return cache["ss"]


def _out_size(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def _check_conv(x, wk, what):
    cout, k, _, cin = wk.shape
    if x.dim() != 4 or x.shape[3] != cin:
        raise TbnHipError(f"{what}: input {tuple(x.shape)} is not NHWC with {cin} channels")
    if cin % 32 or cout % 32 or k not in (1, 3):
        raise TbnHipError(f"{what}: the HIP convolutions take 1x1 / 3x3 kernels with cin and cout multiples of 32 "
                          f"(got k = {k}, cin = {cin}, cout = {cout})")


# ---------------------------------------------------------------------------------------------- launches (no autograd)
def _conv_fwd(x, wk, stride, pad, epilogue, ss=None, partial=None, bias=None, flags=0):
    n, h, w, cin = x.shape
    cout, k = wk.shape[0], wk.shape[1]
    oh, ow = _out_size(h, w, k, stride, pad)
    y = _new(x, n, oh, ow, cout)
    call("tbn_conv2d_fwd", ptr(x), cin, ptr(wk), ptr(bias), ptr(y), cout, n, h, w, cin, cout, k, stride, pad, epilogue,
         flags, ss[0].data_ptr() if ss is not None else 0, ss[1].data_ptr() if ss is not None else 0, ptr(partial),
         stream_ptr())
    return y


_BIAS_AT_JOIN = ("{}: a conv bias in front of the BatchNorm of a join (residual, no ReLU, or more than 1024 channels) is "
                 "not implemented: only the tbn_bn_fwd_batch path carries the bias into the running mean")


def _bn_fwd_batch(y, partial, nparts, pld, gamma, beta, bias, state, z):
    """z = relu(bn(y)) with batch statistics from `nparts` rows of (sum, sumsq) partials of pitch `pld` -> the (4, c) stats.
    A conv `bias` cancels in the batch statistics: y and z do not see it, running_mean takes mean + bias"""
    c = y.shape[-1]
    stats = _new(y, 4, c)
    d = BnFwdDesc()
    d.y, d.y_ld, d.p, d.c = y.data_ptr(), c, y.numel() // c, c
    d.partial, d.pld, d.nparts = partial.data_ptr(), pld, nparts
    d.gamma, d.beta, d.conv_bias = gamma.data_ptr(), beta.data_ptr(), ptr(bias)
    d.running_mean, d.running_var = ptr(state.running_mean), ptr(state.running_var)
    d.save_mean, d.save_rstd, d.scale, d.shift = _rows(stats)
    d.seg[0] = BnSeg(z.data_ptr(), c, 0)
    d.nseg = 1
    call("tbn_bn_fwd_batch", C.byref(d), 1, MOMENTUM, EPS, stream_ptr())
    _wrote_running(state)
    return stats


def _unit_fwd_train(x, wk, gamma, beta, state, res, relu, bias=None):
    """-> (y, z, stats): bias-free conv output, block output, (4, c) rows batch mean | 1/std | scale | shift"""
    n, h, w, cin = x.shape
    cout, k = wk.shape[0], wk.shape[1]
    batched = res is None and relu and cout <= 1024
    if bias is not None and not batched:
        raise TbnHipError(_BIAS_AT_JOIN.format("conv_bn_act"))
    tiles = lib().tbn_conv2d_stat_tiles(n, h, w, cin, cout, k, state.stride, state.pad)
    partial = _new(x, tiles * 2 * cout)
    y = _conv_fwd(x, wk, state.stride, state.pad, 1, partial=partial)
    z = torch.empty_like(y)
    if batched:
        return y, z, _bn_fwd_batch(y, partial, tiles, cout, gamma, beta, bias, state, z)
    stats = _new(x, 4, cout)
    call("tbn_bn_res_fwd", ptr(y), cout, y.numel() // cout, cout, ptr(partial), cout, tiles, ptr(gamma), ptr(beta),
         ptr(state.running_mean), ptr(state.running_var), MOMENTUM, EPS, *_rows(stats), ptr(res), cout, int(relu), ptr(z),
         cout, stream_ptr())
    _wrote_running(state)
    return y, z, stats


def _unit_fwd_eval(x, wk, gamma, beta, state, res, relu, bias=None):
    ss = folded_bn(gamma, beta, state, bias)
    if res is None and relu:
        return _conv_fwd(x, wk, state.stride, state.pad, 2, ss=ss)
    z = _conv_fwd(x, wk, state.stride, state.pad, 0)
    cout = wk.shape[0]
    call("tbn_bn_res_apply", ptr(z), cout, z.numel() // cout, cout, ss[0].data_ptr(), ss[1].data_ptr(), ptr(res), cout,
         int(relu), ptr(z), cout, stream_ptr())
    return z


def _bn_bwd(dz, y, z, stats, had_res, relu, dres, need_affine):
    """-> (dy, dgamma, dbeta); `dres` (a (p, c) buffer or None) receives the gradient of the residual"""
    cout = y.shape[-1]
    p = y.numel() // cout
    dy = torch.empty_like(y)
    dgb = _new(y, 2, cout) if need_affine else None
    dg, db = (dgb[0].data_ptr(), dgb[1].data_ptr()) if need_affine else (0, 0)
    if not had_res and relu and cout <= 1024:
        scratch = _new(y, lib().tbn_bn_bwd_partial_floats(p, cout) + 3 * cout)
        d = BnBwdDesc()
        d.dz[0] = BnSeg(dz.data_ptr(), cout, 0)
        d.nseg = 1
        d.y, d.dy, d.y_ld, d.p, d.c = y.data_ptr(), dy.data_ptr(), cout, p, cout
        d.mean, d.rstd, d.scale, d.shift = _rows(stats)
        d.partial, d.ext_parts, d.coef = scratch.data_ptr(), 0, scratch.data_ptr() + 4 * (scratch.numel() - 3 * cout)
        d.dgamma, d.dbeta, d.dbias = dg, db, 0
        call("tbn_bn_bwd_batch", C.byref(d), 1, stream_ptr())
    else:
        ws = _new(y, lib().tbn_bn_res_bwd_workspace_floats(p, cout))
        call("tbn_bn_res_bwd", ptr(dz), cout, ptr(z) if relu else 0, cout, ptr(y), cout, p, cout, *_rows(stats)[:3],
             int(relu), ptr(dy), cout, ptr(dres), cout, 0, dg, db, ptr(ws), stream_ptr())
    return dy, (dgb[0] if need_affine else None), (dgb[1] if need_affine else None)


def _conv_wgrad(dy, x, wk, state):
    n, h, w, cin = x.shape
    cout, k = wk.shape[0], wk.shape[1]
    dwk = torch.empty_like(wk)
    nws = lib().tbn_conv2d_wgrad_workspace_floats(n, h, w, cin, cout, k, state.stride, state.pad)
    ws = _new(x, max(nws, 1))
    call("tbn_conv2d_wgrad", ptr(dy), cout, ptr(x), cin, ptr(dwk), n, h, w, cin, cout, k, state.stride, state.pad,
         ptr(ws), stream_ptr())
    return _oihw(dwk)


def _conv_dgrad(dy, wk, x_shape, state, dx=None):
    """data gradient into `dx`: a fresh buffer, or ADDED to the one given"""
    n, h, w, cin = x_shape
    cout, k = wk.shape[0], wk.shape[1]
    acc = dx is not None
    if dx is None:
        dx = _new(dy, x_shape)
    ws = _new(dy, wk.numel())
    call("tbn_conv2d_dgrad", ptr(dy), cout, ptr(wk), ptr(dx), cin, n, h, w, cin, cout, k, state.stride, state.pad,
         int(acc), ptr(ws), stream_ptr())
    return dx


_EVAL_BACKWARD = ("{}: backward through an eval-mode backbone (running-statistics BN) is not implemented; call .train() "
                  "for fine-tuning or wrap inference in torch.no_grad()")
_NO_INPUT_GRAD = ("{}: the gradient with respect to the input frames is not implemented (the first conv's data gradient "
                  "is never formed); detach the input")


def _dead_backward(ctx, who, slots, input_grad=True):
    """the opening of every backward with a BatchNorm in it -> None when the node saved what its backward needs (`ctx.live`),
    else the all-None result.  `slots`: the needs_input_grad entries that this operator can differentiate; with
    `input_grad` off (stems, first layers) entry 0, the frames, is not one of them and asking for it is refused."""
    need = ctx.needs_input_grad
    if not input_grad and need[0]:
        raise TbnHipError(_NO_INPUT_GRAD.format(who))
    if ctx.live:
        return None
    if ctx.eval_mode and any(need[i] for i in slots):
        raise TbnHipError(_EVAL_BACKWARD.format(who))
    return (None,) * len(need)


# ---------------------------------------------------------------------------------------------- one fused unit
class _ConvBnActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, state, relu, training, bias=None):
        _need_cuda(x, "conv_bn_act")
        x = _f32c(x)
        wk = kernel_weight(weight, state.wcache)
        _check_conv(x, wk, "conv_bn_act")
        res = _f32c(residual) if residual is not None else None
        cb = _bias_f32(bias)
        ctx.eval_mode = not training
        ctx.live = training and (any(ctx.needs_input_grad[:5]) or ctx.needs_input_grad[8])
        if not training:
            return _unit_fwd_eval(x, wk, gamma, beta, state, res, relu, cb)
        y, z, stats = _unit_fwd_train(x, wk, gamma, beta, state, res, relu, cb)
        if ctx.live:
            ctx.state, ctx.relu, ctx.had_res = state, relu, res is not None
            ctx.save_for_backward(x, wk, y, z, stats)
        return z

    @staticmethod
    def backward(ctx, dz):
        need = ctx.needs_input_grad
        dead = _dead_backward(ctx, "conv_bn_act", (0, 1, 2, 3, 4, 8))
        if dead:
            return dead
        x, wk, y, z, stats = ctx.saved_tensors
        dz = _f32c(dz)
        dres = torch.empty_like(y) if (ctx.had_res and need[4]) else None
        dy, dg, db = _bn_bwd(dz, y, z, stats, ctx.had_res, ctx.relu, dres, need[2] or need[3])
        dw = _conv_wgrad(dy, x, wk, ctx.state) if need[1] else None
        dx = _conv_dgrad(dy, wk, x.shape, ctx.state) if need[0] else None
        dbias = _zero_bias_grad(y, y.shape[-1]) if need[8] else None
        return dx, dw, dg if need[2] else None, db if need[3] else None, dres, None, None, None, dbias


def conv_bn_act(x, weight, gamma, beta, running_mean, running_var, stride, pad, residual=None, relu=True,
                training=True, state=None, bias=None):
    """act(bn(conv(x) + bias) + residual) on NHWC tensors: x (n, h, w, cin), weight OIHW, residual (n, oh, ow, cout) or
    None, act = ReLU or identity.  training: batch statistics, running_mean / running_var (may be None) updated with
    momentum 0.1; else the running statistics.  `state` (a BnState the caller keeps) carries the weight and fold caches
    from call to call; without one they are rebuilt per call.  `bias` (cout floats or None): in training it cancels in the
    batch statistics -- the output is bit-identical to the call without it, running_mean takes mean + bias, its gradient
    is zeros -- and is only taken where no residual joins (ReLU, at most 1024 channels); in eval it is folded into the
    shift."""
    state = _adopt_state(state, stride, pad, (running_mean, running_var))
    return _ConvBnActFn.apply(x, weight, gamma, beta, residual, state, bool(relu), bool(training), bias)


# ---------------------------------------------------------------------------------------------- a residual block
class _ResidualBlockFn(torch.autograd.Function):
    """x -> relu(bn_K(conv_K(... relu(bn_1(conv_1(x))))) + shortcut(x)), shortcut = identity or bn_d(conv_d(x)).
    params: (weight, gamma, beta) of the K main units, then of the downsample unit when `states` has K + 1 entries."""

    @staticmethod
    def forward(ctx, x, states, nmain, training, *params):
        _need_cuda(x, "residual_block")
        x = _f32c(x)
        units = [(kernel_weight(params[3 * i], s.wcache), params[3 * i + 1], params[3 * i + 2], s)
                 for i, s in enumerate(states)]
        has_ds = len(states) == nmain + 1
        _check_conv(x, units[0][0], "residual_block")
        fwd = _unit_fwd_train if training else _unit_fwd_eval
        ctx.eval_mode = not training
        ctx.live = training and (ctx.needs_input_grad[0] or any(ctx.needs_input_grad[4:]))
        saved = [x]
        res = x
        if has_ds:
            out = fwd(x, *units[nmain], None, False)
            res = out[1] if training else out
            if ctx.live:
                saved += [units[nmain][0], out[0], out[2]]        # wk, y, stats
        cur = x
        for i in range(nmain):
            last = i == nmain - 1
            out = fwd(cur, *units[i], res if last else None, True)
            cur = out[1] if training else out
            if ctx.live:
                saved += [units[i][0], out[0], out[1], out[2]]    # wk, y, z, stats
        if ctx.live:
            ctx.states, ctx.nmain, ctx.has_ds = states, nmain, has_ds
            ctx.save_for_backward(*saved)
        return cur

    @staticmethod
    def backward(ctx, dout):
        need = ctx.needs_input_grad
        dead = _dead_backward(ctx, "residual_block", (0, *range(4, len(need))))
        if dead:
            return dead
        saved = list(ctx.saved_tensors)
        states, nmain, has_ds = ctx.states, ctx.nmain, ctx.has_ds
        x = saved.pop(0)
        ds = None
        if has_ds:
            ds, saved = saved[:3], saved[3:]
        main = [saved[4 * i:4 * i + 4] for i in range(nmain)]
        grads = [None] * (3 * len(states))

        def pneed(u, j):                 # weight / gamma / beta of unit u
            return need[4 + 3 * u + j]

        dz = _f32c(dout)
        dx = None
        # the join: dres goes to the block input's gradient (identity shortcut) or to the downsample unit
        ds_live = has_ds and (need[0] or any(pneed(nmain, j) for j in range(3)))
        wk, y, z, stats = main[-1]
        if has_ds:
            dres = torch.empty_like(y) if ds_live else None
        else:
            dres = dx = torch.empty_like(x) if need[0] else None
        dy, dg, db = _bn_bwd(dz, y, z, stats, True, True, dres, pneed(nmain - 1, 1) or pneed(nmain - 1, 2))
        if ds_live:
            dwk, dyy, dstats = ds
            ddy, ddg, ddb = _bn_bwd(dres, dyy, None, dstats, True, False, None, pneed(nmain, 1) or pneed(nmain, 2))
            if pneed(nmain, 0):
                grads[3 * nmain] = _conv_wgrad(ddy, x, dwk, states[nmain])
            grads[3 * nmain + 1] = ddg if pneed(nmain, 1) else None
            grads[3 * nmain + 2] = ddb if pneed(nmain, 2) else None
            if need[0]:
                dx = _conv_dgrad(ddy, dwk, x.shape, states[nmain])
        for i in range(nmain - 1, -1, -1):
            wk = main[i][0]
            inp = x if i == 0 else main[i - 1][2]
            if i < nmain - 1:
                if not (need[0] or any(pneed(u, j) for u in range(i + 1) for j in range(3))):
                    break                # nothing from this unit down to the block input is differentiated
                _, y, z, stats = main[i]
                dy, dg, db = _bn_bwd(dz, y, z, stats, False, True, None, pneed(i, 1) or pneed(i, 2))
            if pneed(i, 0):
                grads[3 * i] = _conv_wgrad(dy, inp, wk, states[i])
            grads[3 * i + 1] = dg if pneed(i, 1) else None
            grads[3 * i + 2] = db if pneed(i, 2) else None
            if i > 0:
                if need[0] or any(pneed(u, j) for u in range(i) for j in range(3)):
                    dz = _conv_dgrad(dy, wk, inp.shape, states[i])
            elif need[0]:
                # the shortcut's gradient is already in dx: conv1's data gradient is accumulated into it
                dx = _conv_dgrad(dy, wk, x.shape, states[0], dx=dx)
        return (dx, None, None, None) + tuple(grads)


def residual_block(x, main, downsample=None, training=True):
    """torchvision's BasicBlock (two units) / Bottleneck (three) on NHWC x.  `main`: [(weight, gamma, beta, BnState)] in
    order, every unit followed by ReLU, the last one after the shortcut is added; `downsample`: the same tuple for the
    1x1 conv + BN of the shortcut (no ReLU), or None for the identity."""
    units = list(main) + ([downsample] if downsample is not None else [])
    params = [t for u in units for t in u[:3]]
    return _ResidualBlockFn.apply(x, [u[3] for u in units], len(main), bool(training), *params)


# ---------------------------------------------------------------------------------------------- global average pool
class _GlobalMeanFn(torch.autograd.Function):
    """NHWC (n, h, w, c) -> (n, c), or with `freq_only` the mean over h alone -> (n, w, c).  tbn_spatial_mean_fwd takes at
    most 1024 channels per call: wider maps (the 2048 of ResNet-50/101/152) go through it as column ranges of the same
    buffers (the entry reads and writes pitched rows)."""

    @staticmethod
    def forward(ctx, x, freq_only=False):
        _need_cuda(x, "freq_mean" if freq_only else "global_mean")
        x = _f32c(x)
        n, h, w, c = x.shape
        out = _new(x, (n, w, c) if freq_only else (n, c))
        for c0 in range(0, c, 1024):
            call("tbn_spatial_mean_fwd", x.data_ptr() + 4 * c0, c, out.data_ptr() + 4 * c0, c, n, h, w, min(1024, c - c0),
                 int(freq_only), stream_ptr())
        ctx.shape, ctx.freq_only = tuple(x.shape), freq_only
        return out

    @staticmethod
    def backward(ctx, dout):
        n, h, w, c = ctx.shape
        dout = _f32c(dout)
        dx = _new(dout, ctx.shape)
        call("tbn_spatial_mean_bwd", ptr(dout), c, ptr(dx), c, n, h, w, c, int(ctx.freq_only), stream_ptr())
        return dx, None


def global_mean(x_nhwc):
    """AdaptiveAvgPool2d(1) + flatten on an NHWC map of any width that is a multiple of 4"""
    return _GlobalMeanFn.apply(x_nhwc)


def freq_mean(x_nhwc):
    """the mean over the frequency axis alone, (n, h, w, c) -> (n, w, c): F.avg_pool2d(features, (h, 1)) of the attended
    audio trunk (reference bn_inception_audio.py:1012-1019) in the layout the attention heads read"""
    return _GlobalMeanFn.apply(x_nhwc, True)


# ---------------------------------------------------------------------------------------------- 3x3 pools
def pool_out_size(size, stride, pad, ceil_mode):
    """output length of a kernel-3 pool along one axis (torch's rule: in ceil mode the last window must start inside the
    input or its left padding)"""
    o = (size + 2 * pad - 3 + (stride - 1 if ceil_mode else 0)) // stride + 1
    if ceil_mode and (o - 1) * stride >= size + pad:
        o -= 1
    return o


def _check_pool(x, what):
    _need_cuda(x, what)
    if x.dim() != 4 or x.shape[3] % 4:
        raise TbnHipError(f"{what}: input {tuple(x.shape)} is not NHWC with a multiple of 4 channels")


class _MaxPool3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride, pad, ceil_mode):
        _check_pool(x, "maxpool3")
        x = _f32c(x)
        n, h, w, c = x.shape
        oh, ow = pool_out_size(h, stride, pad, ceil_mode), pool_out_size(w, stride, pad, ceil_mode)
        out = _new(x, n, oh, ow, c)
        live = ctx.needs_input_grad[0]
        argmax = _new(x, n, oh, ow, c, dtype=torch.uint8) if live else None
        call("tbn_maxpool3_fwd", ptr(x), c, ptr(out), c, ptr(argmax), n, h, w, c, oh, ow, stride, pad, stream_ptr())
        if live:
            ctx.geom = (n, h, w, c, oh, ow, stride, pad)
            ctx.save_for_backward(argmax)
        return out

    @staticmethod
    def backward(ctx, dout):
        (argmax,) = ctx.saved_tensors
        n, h, w, c, oh, ow, stride, pad = ctx.geom
        dout = _f32c(dout)
        dx = _new(dout, n, h, w, c)
        call("tbn_maxpool3_bwd", ptr(dout), c, ptr(argmax), ptr(dx), c, n, h, w, c, oh, ow, stride, pad, 0, stream_ptr())
        return dx, None, None, None


def maxpool3(x_nhwc, stride, pad, ceil_mode=False):
    """nn.MaxPool2d(3, stride, pad, ceil_mode=ceil_mode) on an NHWC map (channels a multiple of 4)"""
    return _MaxPool3Fn.apply(x_nhwc, int(stride), int(pad), bool(ceil_mode))


class _AvgPool3Fn(torch.autograd.Function):
    """tbn_avgpool3_fwd is self-adjoint: the same launch on the output's gradient is the backward"""

    @staticmethod
    def forward(ctx, x):
        _check_pool(x, "avgpool3")
        x = _f32c(x)
        n, h, w, c = x.shape
        out = torch.empty_like(x)
        call("tbn_avgpool3_fwd", ptr(x), c, ptr(out), c, n, h, w, c, 0, stream_ptr())
        return out

    @staticmethod
    def backward(ctx, dout):
        return _AvgPool3Fn.apply(dout)


def avgpool3(x_nhwc):
    """nn.AvgPool2d(3, stride 1, padding 1, count_include_pad=True) on an NHWC map (channels a multiple of 4)"""
    return _AvgPool3Fn.apply(x_nhwc)


# ---------------------------------------------------------------------------------------------- the stem
def _bn_pool_fwd(y, gamma, beta, rm, rv, pooled, argmax, pad):
    """pooled = MaxPool(3, 2, pad)(relu(bn(y))) with batch statistics, the running buffers rm / rv (may be None) updated
    -> the (4, c) stats"""
    n, oh, ow, c = y.shape
    stats = _new(y, 4, c)
    bnws = _new(y, lib().tbn_bn_workspace_floats(n * oh * ow, c))
    call("tbn_bn_relu_maxpool_train_fwd", ptr(y), n, oh, ow, c, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), MOMENTUM, EPS,
         *_rows(stats), ptr(pooled), c, ptr(argmax), pooled.shape[1], pooled.shape[2], 2, pad, ptr(bnws), stream_ptr())
    return stats


def _bn_pool_bwd(dpooled, argmax, y, stats, pad):
    """-> (dy, dgb): the gradient of the conv output and the (2, c) rows dgamma | dbeta"""
    n, oh, ow, c = y.shape
    dpooled = _f32c(dpooled)
    dy = torch.empty_like(y)
    dgb = _new(y, 2, c)
    bnws = _new(y, lib().tbn_bn_workspace_floats(n * oh * ow, c))
    call("tbn_bn_relu_maxpool_train_bwd", ptr(dpooled), c, ptr(argmax), ptr(y), n, oh, ow, c, argmax.shape[1],
         argmax.shape[2], 2, pad, *_rows(stats), ptr(dy), dgb[0].data_ptr(), dgb[1].data_ptr(), ptr(bnws), stream_ptr())
    return dy, dgb


class _StemFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, state, training, who):
        _need_cuda(x, who)
        x = _f32c(x)
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        if tuple(weight.shape[1:]) != (cin, 7, 7) or not 1 <= cin <= 16 or cout % 32:
            raise TbnHipError(f"{who}: the stem is a 7x7 / stride 2 / pad 3 conv of 1..16 input channels, got weight "
                              f"{tuple(weight.shape)} for input {tuple(x.shape)}")
        wk = kernel_weight(weight, state.wcache)
        st = stream_ptr()
        oh, ow = _out_size(h, w, 7, 2, 3)
        ph, pw = _out_size(oh, ow, 3, 2, 1)           # MaxPool2d(3, 2, 1), ceil_mode off
        ws = _new(x, lib().tbn_stem_workspace_floats(cin, h, w, 0, n, cout))
        y = _new(x, n, oh, ow, cout)
        pooled = _new(x, n, ph, pw, cout)
        argmax = _new(x, n, ph, pw, cout, dtype=torch.uint8)
        ctx.eval_mode = not training
        ctx.live = training and any(ctx.needs_input_grad[1:4])
        ctx.who = who
        if not training:
            ss = folded_bn(gamma, beta, state)
            call("tbn_stem_conv_fwd", ptr(x), ptr(wk), 0, ptr(y), cout, n, h, w, cin, cout, 0, 2, ss[0].data_ptr(),
                 ss[1].data_ptr(), 0, 0, 0, 0, ptr(ws), st)
            call("tbn_maxpool3_fwd", ptr(y), cout, ptr(pooled), cout, ptr(argmax), n, oh, ow, cout, ph, pw, 2, 1, st)
            return pooled
        # the heuristic picks the tile: statistics rows are per 128 * mt output rows, unwritten rows must read as zero
        partial = torch.zeros((n * oh * ow + 127) // 128 * 2 * cout, device=x.device, dtype=torch.float32)
        call("tbn_stem_conv_fwd", ptr(x), ptr(wk), 0, ptr(y), cout, n, h, w, cin, cout, 0, 1, 0, 0, ptr(partial), 0, 0, 0,
             ptr(ws), st)
        stats = _bn_pool_fwd(y, gamma, beta, state.running_mean, state.running_var, pooled, argmax, 1)
        _wrote_running(state)
        if ctx.live:
            ctx.save_for_backward(x, y, argmax, stats)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        need = ctx.needs_input_grad
        dead = _dead_backward(ctx, ctx.who, (1, 2, 3), input_grad=False)
        if dead:
            return dead
        x, y, argmax, stats = ctx.saved_tensors
        n, cin, h, w = x.shape
        cout = y.shape[-1]
        dy, dgb = _bn_pool_bwd(dpooled, argmax, y, stats, 1)
        dw = None
        if need[1]:
            ws = _new(x, lib().tbn_stem_workspace_floats(cin, h, w, 0, n, cout))
            dwk = _new(x, cout, 7, 7, cin)
            call("tbn_stem_conv_wgrad", ptr(dy), cout, ptr(x), ptr(dwk), n, h, w, cin, cout, 0, 0, 0, ptr(ws), stream_ptr())
            dw = _oihw(dwk)
        return None, dw, dgb[0] if need[2] else None, dgb[1] if need[3] else None, None, None, None


def stem_bn_pool(x_nchw, weight, gamma, beta, state, training=True, who="stem_bn_pool"):
    """MaxPool2d(3, 2, 1)(relu(bn(conv7x7_s2_p3(x)))): NCHW frames (n, cin <= 16, h, w) -> NHWC (n, ph, pw, cout).  No
    input gradient is formed: asking for one raises TbnHipError in backward."""
    return _StemFn.apply(x_nchw, weight, gamma, beta, state, bool(training), who)


# ---------------------------------------------------------------------------------------------- the separable audio stem
class _AudioStemFn(torch.autograd.Function):
    """params: the two conv weights, the two conv biases, then gamma / beta of the two BatchNorms"""

    @staticmethod
    def forward(ctx, x, wa, wb, ba, bb, ga, gb, bea, beb, bns, training):
        who = "audio_stem_bn_pool"
        _need_cuda(x, who)
        x = _f32c(x)
        if (x.dim() != 4 or x.shape[1] != 1 or tuple(wa.shape) != (32, 1, 3, 1) or tuple(wb.shape) != (32, 1, 1, 3)
                or any(t.numel() != 32 for t in (ba, bb, ga, gb, bea, beb))):
            raise TbnHipError(f"{who}: the audio stem is Conv2d(1, 32, (3, 1)) | Conv2d(1, 32, (1, 3)) with bias on a "
                              f"one-channel input, got weights {tuple(wa.shape)}, {tuple(wb.shape)} for input "
                              f"{tuple(x.shape)}")
        n, _, h, w = x.shape
        st = stream_ptr()
        cat = lambda a, b: torch.cat([a.detach().reshape(32, -1), b.detach().reshape(32, -1)]).float().contiguous()
        wk = cat(wa, wb)                                   # [64][3]
        bias, gamma, beta = cat(ba, bb).view(64), cat(ga, gb).view(64), cat(bea, beb).view(64)
        # two 32-channel BatchNorms over a concatenation are one 64-channel BatchNorm
        rm = torch.cat([bns[0].running_mean, bns[1].running_mean]).float()
        rv = torch.cat([bns[0].running_var, bns[1].running_var]).float()
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        ph, pw = pool_out_size(oh, 2, 0, True), pool_out_size(ow, 2, 0, True)      # MaxPool2d(3, 2, ceil_mode=True)
        y = _new(x, n, oh, ow, 64)
        pooled = _new(x, n, ph, pw, 64)
        ctx.eval_mode = not training
        ctx.live = training and any(ctx.needs_input_grad[1:9])
        if not training:
            sc = gamma / torch.sqrt(rv + EPS)
            sh = beta + (bias - rm) * sc
            call("tbn_audio_stem_fwd", ptr(x), ptr(wk), 0, ptr(y), 64, n, h, w, 2, 0, ptr(sc), ptr(sh), 0, st)
            call("tbn_maxpool3_fwd", ptr(y), 64, ptr(pooled), 64, 0, n, oh, ow, 64, ph, pw, 2, 0, st)
            return pooled
        argmax = _new(x, n, ph, pw, 64, dtype=torch.uint8)
        partial = _new(x, lib().tbn_audio_stem_stat_rows(n, h, w) * 128)
        call("tbn_audio_stem_fwd", ptr(x), ptr(wk), 0, ptr(y), 64, n, h, w, 1, 0, 0, 0, ptr(partial), st)
        stats = _bn_pool_fwd(y, gamma, beta, rm, rv, pooled, argmax, 0)
        # y is the bias-free conv output: the reference's BatchNorm sees conv + bias, its batch mean is larger by the bias
        rm += MOMENTUM * bias
        for i, bn in enumerate(bns):       # (copy_ bumps the buffers' `_version` for the caches keyed on it)
            bn.running_mean.copy_(rm[32 * i:32 * i + 32])
            bn.running_var.copy_(rv[32 * i:32 * i + 32])
        if ctx.live:
            ctx.save_for_backward(x, y, argmax, stats)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        need = ctx.needs_input_grad
        dead = _dead_backward(ctx, "audio_stem_bn_pool", range(1, 9), input_grad=False)
        if dead:
            return dead
        x, y, argmax, stats = ctx.saved_tensors
        n, _, h, w = x.shape
        dy, dgb = _bn_pool_bwd(dpooled, argmax, y, stats, 0)
        dwa = dwb = None
        if need[1] or need[2]:
            ws = _new(x, lib().tbn_audio_stem_wgrad_workspace_floats(n, h, w))
            dwk = _new(x, 64, 3)
            call("tbn_audio_stem_wgrad", ptr(dy), 64, ptr(x), ptr(dwk), n, h, w, ptr(ws), stream_ptr())
            dwa, dwb = dwk[:32].view(32, 1, 3, 1), dwk[32:].view(32, 1, 1, 3)
        return (None, dwa if need[1] else None, dwb if need[2] else None, _zero_bias_grad(x, 32) if need[3] else None,
                _zero_bias_grad(x, 32) if need[4] else None, dgb[0, :32] if need[5] else None, dgb[0, 32:] if need[6] else None,
                dgb[1, :32] if need[7] else None, dgb[1, 32:] if need[8] else None, None, None)


def audio_stem_bn_pool(x_nchw, conv_a, bn_a, conv_b, bn_b, training=True):
    """MaxPool2d(3, 2, ceil_mode=True)(cat(relu(bn_a(conv_a(x))), relu(bn_b(conv_b(x))))): a one-channel spectrogram
    (n, 1, h, w) -> NHWC (n, ph, pw, 64).  conv_a = Conv2d(1, 32, (3, 1), stride 2, padding (1, 0)), conv_b = Conv2d(1, 32,
    (1, 3), stride 2, padding (0, 1)), both with bias; the modules are parameter containers, in training their running
    statistics are updated in place.  No input gradient is formed: asking for one raises TbnHipError in backward."""
    return _AudioStemFn.apply(x_nchw, conv_a.weight, conv_b.weight, conv_a.bias, conv_b.bias, bn_a.weight, bn_b.weight,
                              bn_a.bias, bn_b.bias, (bn_a, bn_b), bool(training))


# ---------------------------------------------------------------------------------------------- conv + bias (+ ReLU), no BN
def _relu_mask(dz, z):
    g = torch.empty_like(dz)
    call("tbn_relu_mask_bwd", ptr(dz), ptr(z), 0, ptr(g), dz.numel(), stream_ptr())
    return g


def _colsum(g):
    """column sums of a (..., c) tensor seen as (rows, c): the bias gradient.  tbn_colsum runs c / 32 workgroups whatever the
    row count (it was written for the heads' few hundred rows; over the 4.8 M rows of a 96 x 224 x 224 map it took 70 % of a
    VGG16 step), so the rows are first folded into the per-chunk sums of tbn_bn_stats_partials at streaming rate (its sums
    of squares go unused) and tbn_colsum adds those few rows"""
    c = g.shape[-1]
    rows = g.numel() // c
    out = _new(g, c)
    if c > 1024:         # wider than the statistics kernel takes
        call("tbn_colsum", ptr(g), c, ptr(out), rows, c, stream_ptr())
        return out
    partial = _new(g, lib().tbn_bn_workspace_floats(rows, c))
    nparts = C.c_int(0)
    call("tbn_bn_stats_partials", ptr(g), c, rows, c, ptr(partial), C.byref(nparts), stream_ptr())
    call("tbn_colsum", ptr(partial), 2 * c, ptr(out), nparts.value, c, stream_ptr())
    return out


class _ConvBiasActFn(torch.autograd.Function):
    """Without BatchNorm train and eval are the same function: backward works in both."""

    @staticmethod
    def forward(ctx, x, weight, bias, state, relu, relu_in_pool):
        _need_cuda(x, "conv_bias_act")
        x = _f32c(x)
        wk = kernel_weight(weight, state.wcache)
        _check_conv(x, wk, "conv_bias_act")
        cb = _bias_f32(bias)
        z = _conv_fwd(x, wk, state.stride, state.pad, 0, bias=cb, flags=2 if relu else 0)
        if any(ctx.needs_input_grad[:3]):
            ctx.state, ctx.mask = state, relu and not relu_in_pool
            ctx.save_for_backward(x, wk, z if ctx.mask else None)
        return z

    @staticmethod
    def backward(ctx, dz):
        need = ctx.needs_input_grad
        x, wk, z = ctx.saved_tensors
        dy = _f32c(dz)
        if ctx.mask:
            dy = _relu_mask(dy, z)
        db = _colsum(dy) if need[2] else None
        dw = _conv_wgrad(dy, x, wk, ctx.state) if need[1] else None
        dx = _conv_dgrad(dy, wk, x.shape, ctx.state) if need[0] else None
        return dx, dw, db, None, None, None


def conv_bias_act(x, weight, bias, stride, pad, relu=True, relu_in_pool=False, state=None):
    """act(conv(x) + bias) on NHWC tensors, act = ReLU or identity: x (n, h, w, cin), weight OIHW (1x1 / 3x3, cin and cout
    multiples of 32), bias (cout floats or None).  `relu_in_pool`: the caller passes the output straight to
    maxpool2(..., relu_gate=True), whose backward applies this unit's ReLU mask -- the backward here then skips its own mask
    pass (the pair costs one pass over the map instead of two).  A frozen weight / bias costs no gradient launch.  `state`
    (a BnState the caller keeps) carries the kernel-layout weight copy from call to call."""
    state = _adopt_state(state, stride, pad)
    return _ConvBiasActFn.apply(x, weight, bias, state, bool(relu), bool(relu and relu_in_pool))


# ---------------------------------------------------------------------------------------------- the 3x3 first layer
class _FirstConv3Fn(torch.autograd.Function):
    """x NCHW frames; gamma is None: relu(conv + bias) (train = eval); else BatchNorm + ReLU behind the conv"""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, state, relu, training, relu_in_pool, who):
        _need_cuda(x, who)
        x = _f32c(x)
        if x.dim() != 4 or tuple(weight.shape) != (64, x.shape[1], 3, 3) or not 1 <= x.shape[1] <= 16:
            raise TbnHipError(f"{who}: the first layer is a 3x3 / stride 1 / pad 1 conv of 1..16 input channels to 64, got "
                              f"weight {tuple(weight.shape)} for input {tuple(x.shape)}")
        n, cin, h, w = x.shape
        wk = kernel_weight(weight, state.wcache)
        cb = _bias_f32(bias)
        st = stream_ptr()
        y = _new(x, n, h, w, 64)
        ctx.who, ctx.bn, ctx.eval_mode = who, gamma is not None, False
        if gamma is None:
            call("tbn_conv3_first_fwd", ptr(x), ptr(wk), ptr(cb), ptr(y), 64, n, h, w, cin, 64, 0, 2 if relu else 0, 0, 0,
                 0, st)
            ctx.live = any(ctx.needs_input_grad[1:3])
            if ctx.live:
                ctx.mask = relu and not relu_in_pool
                ctx.save_for_backward(x, y if ctx.mask else None)
            return y
        if not relu:
            raise TbnHipError(f"{who}: the BatchNorm form of the first layer is always followed by ReLU")
        ctx.eval_mode = not training
        ctx.live = training and any(ctx.needs_input_grad[1:5])
        if not training:
            ss = folded_bn(gamma, beta, state, cb)
            call("tbn_conv3_first_fwd", ptr(x), ptr(wk), 0, ptr(y), 64, n, h, w, cin, 64, 2, 0, ss[0].data_ptr(),
                 ss[1].data_ptr(), 0, st)
            return y
        rows = lib().tbn_conv3_first_stat_rows(n, cin, h, w)
        partial = _new(x, rows * 128)
        call("tbn_conv3_first_fwd", ptr(x), ptr(wk), 0, ptr(y), 64, n, h, w, cin, 64, 1, 0, 0, 0, ptr(partial), st)
        z = torch.empty_like(y)
        stats = _bn_fwd_batch(y, partial, rows, 64, gamma, beta, cb, state, z)
        if ctx.live:
            ctx.save_for_backward(x, y, z, stats)
        return z

    @staticmethod
    def backward(ctx, dz):
        need = ctx.needs_input_grad
        dead = _dead_backward(ctx, ctx.who, (1, 2, 3, 4), input_grad=False)
        if dead:
            return dead
        dy = _f32c(dz)
        dg = dbeta = db = None
        if ctx.bn:
            x, y, z, stats = ctx.saved_tensors
            dy, dg, dbeta = _bn_bwd(dy, y, z, stats, False, True, None, need[3] or need[4])
            db = _zero_bias_grad(x, 64) if need[2] else None
        else:
            x, z = ctx.saved_tensors
            if ctx.mask:
                dy = _relu_mask(dy, z)
            db = _colsum(dy) if need[2] else None
        dw = None
        if need[1]:
            n, cin, h, w = x.shape
            ws = _new(x, max(lib().tbn_conv3_first_wgrad_workspace_floats(n, cin, h, w), 1))
            dwk = _new(x, 64, 3, 3, cin)
            call("tbn_conv3_first_wgrad", ptr(dy), 64, ptr(x), ptr(dwk), n, h, w, cin, 64, ptr(ws), stream_ptr())
            dw = _oihw(dwk)
        return (None, dw, db, dg if need[3] else None, dbeta if need[4] else None, None, None, None, None, None)


def first_conv3(x_nchw, weight, bias, gamma=None, beta=None, state=None, relu=True, training=True, relu_in_pool=False,
                who="first_conv3"):
    """The 3x3 / stride 1 / pad 1 first layer straight from NCHW frames (n, cin <= 16, h, w) -> NHWC (n, h, w, 64).
    Plain form (gamma is None): act(conv + bias), the same function in train and eval; `relu_in_pool` as in conv_bias_act.
    BatchNorm form (gamma, beta and a BnState with the running statistics): relu(bn(conv + bias)); in training the bias
    cancels in the batch statistics and only enters the running mean, as conv_bn_act(bias=) does it, in eval it is folded
    into the shift.  No input gradient is formed: asking for one raises TbnHipError in backward."""
    if state is None:
        state = BnState(1, 1, None, None)
    return _FirstConv3Fn.apply(x_nchw, weight, bias, gamma, beta, state, bool(relu), bool(training),
                               bool(relu and relu_in_pool and gamma is None), who)


# ---------------------------------------------------------------------------------------------- the pools of a VGG
class _MaxPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, relu_gate):
        _check_pool(x, "maxpool2")
        x = _f32c(x)
        n, h, w, c = x.shape
        out = _new(x, n, h // 2, w // 2, c)
        live = ctx.needs_input_grad[0]
        argmax = _new(x, n, h // 2, w // 2, c, dtype=torch.uint8) if live else None
        call("tbn_maxpool2_fwd", ptr(x), c, ptr(out), c, ptr(argmax), n, h, w, c, stream_ptr())
        if live:
            ctx.shape = (n, h, w, c)
            ctx.save_for_backward(argmax, x if relu_gate else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        argmax, z = ctx.saved_tensors
        n, h, w, c = ctx.shape
        dout = _f32c(dout)
        dx = _new(dout, n, h, w, c)
        call("tbn_maxpool2_bwd", ptr(dout), c, ptr(argmax), ptr(z), c, ptr(dx), c, n, h, w, c, 0, stream_ptr())
        return dx, None


def maxpool2(x_nhwc, relu_gate=None):
    """nn.MaxPool2d(2, 2) on an NHWC map (channels a multiple of 4, h and w at least 2; a trailing odd row / column is
    dropped).  `relu_gate` true: x is the output of a ReLU whose own backward mask was left out (conv_bias_act /
    first_conv3 with relu_in_pool) -- the gradient written is additionally gated by x > 0."""
    return _MaxPool2Fn.apply(x_nhwc, bool(relu_gate))


class _AdaptiveAvgPool7Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _check_pool(x, "adaptive_avgpool7_flat")
        x = _f32c(x)
        n, h, w, c = x.shape
        out = _new(x, n, c * 49)
        call("tbn_adaptive_avgpool7_fwd", ptr(x), c, ptr(out), n, h, w, c, stream_ptr())
        ctx.shape = (n, h, w, c)
        return out

    @staticmethod
    def backward(ctx, dout):
        n, h, w, c = ctx.shape
        dout = _f32c(dout)
        dx = _new(dout, n, h, w, c)
        call("tbn_adaptive_avgpool7_bwd", ptr(dout), ptr(dx), c, n, h, w, c, 0, stream_ptr())
        return dx


def adaptive_avgpool7_flat(x_nhwc):
    """torch.flatten(nn.AdaptiveAvgPool2d((7, 7))(x), 1) of an NHWC map (n, h, w, c) -> (n, c * 49) in the NCHW order
    (column = ch * 49 + oy * 7 + ox): a checkpoint's classifier.0.weight multiplies it as it is"""
    return _AdaptiveAvgPool7Fn.apply(x_nhwc)
