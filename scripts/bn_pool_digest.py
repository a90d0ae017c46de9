"""Digests of what the BN / pool kernel family computes, for comparing two builds of the library bit for bit.

The kernels of csrc/bn.hip, bn_multi.hip, bn_res.hip and pool.hip use no atomics and sum in fixed order, so a run repeats
exactly; a change to them that claims to leave results alone must leave every line of this script's output alone.  One
process, inputs from a seeded CPU generator, no retries.  One line per case:

    <case> <sha256 over every output buffer of the case, in a fixed order>

Operator cases: every C entry point of the family (tbn_bn_relu_train_*, tbn_bn_stats_partials, tbn_bn_fwd_batch /
tbn_bn_bwd_batch with one, two and three segments, pitched buffers and external partials, tbn_bn_relu_maxpool_train_* at
3x3 / 2 / 0 and 3x3 / 1 / 1, tbn_bn_res_* in every template arm at c = 64 and 2048, tbn_maxpool3_*, tbn_avgpool3_fwd,
tbn_spatial_mean_*) on maps of 5x5 and 7x6, C in {8, 64, 1024} and row counts that leave a partial last chunk and a
partial four-row group (P = 1, 67, 4 RP + 1 with RP = 256 / (C / 4) row lanes).  Engine cases: one training forward +
backward of BNInception per input-channel count 3, 10 and 1 (2 frames of 64 x 64, no autotuning, riders on and off):
features, every gradient and the running buffers.

    TBN_LIB=<library> python scripts/bn_pool_digest.py [--out file] [--no-engine]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from attention_based_tbn_amd._lib import BnBwdDesc, BnFwdDesc, BnSeg, call, lib  # noqa: E402

DEV = torch.device("cuda")
RNG = np.random.default_rng(20240611)
LINES = []


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def randn(*shape, std=1.0):
    return dev(RNG.standard_normal(shape) * std)


def uniform(*shape, lo=0.5, hi=1.5):
    return dev(RNG.uniform(lo, hi, shape))


def halves(*shape):
    """values on a grid of 0.5: a 3x3 window then holds ties, which the first-maximum rule decides"""
    return dev(np.round(RNG.standard_normal(shape) * 2.0) / 2.0)


def filled(*shape, dtype=torch.float32):
    """an output buffer with a known fill: bytes a kernel leaves alone are hashed too"""
    return torch.full(shape, 3, dtype=dtype, device=DEV)


def emit(case, tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    LINES.append("%-44s %s" % (case, h.hexdigest()))


def row_counts(c):
    return (1, 67, 4 * (256 // (c // 4)) + 1)


def bn_params(c):
    return uniform(c), randn(c, std=0.1), randn(c, std=0.1), uniform(c)   # gamma, beta, running mean, running var


# ---------------------------------------------------------------- single-layer BN
def bn_relu_train(p, c):
    y, dz = randn(p, c), randn(p, c + 12)
    gamma, beta, rm, rv = bn_params(c)
    mean, rstd, scale, shift, dgamma, dbeta = (filled(c) for _ in range(6))
    z, dy = filled(p, c + 8), filled(p, c)
    ws = filled(lib().tbn_bn_workspace_floats(p, c))
    call("tbn_bn_relu_train_fwd", y.data_ptr(), p, c, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1,
         1e-5, mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), z.data_ptr() + 16, c + 8,
         ws.data_ptr(), st())
    call("tbn_bn_relu_train_bwd", dz.data_ptr() + 32, c + 12, y.data_ptr(), p, c, mean.data_ptr(), rstd.data_ptr(),
         scale.data_ptr(), shift.data_ptr(), dy.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), st())
    emit("bn_relu_train p%d c%d" % (p, c), [z, mean, rstd, scale, shift, rm, rv, dy, dgamma, dbeta])


def stats_partials(y, p, c):
    """partials of the column slice y (p, c) of a pitched buffer"""
    partial = filled(lib().tbn_bn_workspace_floats(p, c))
    n = C.c_int(-1)
    call("tbn_bn_stats_partials", y.data_ptr(), y.stride(0), p, c, partial.data_ptr(), C.byref(n), st())
    return partial, n.value


def bn_stats(p, c):
    buf = randn(p, c + 24)
    partial, n = stats_partials(buf[:, 8:8 + c], p, c)
    emit("bn_stats_partials p%d c%d parts%d" % (p, c, n), [partial])


# ---------------------------------------------------------------- batched BN
def seg3(views):
    arr = (BnSeg * 3)()
    for i, (v, col) in enumerate(views):
        arr[i] = BnSeg(v.data_ptr(), v.stride(0), col)
    return arr


def split_cols(c, nseg):
    """first columns of nseg column ranges, multiples of 4, unequal widths"""
    return [0, c // 4 // 3 * 4 or 4, c // 4 * 3 // 4 * 4][:nseg] if nseg > 1 else [0]


class Member:
    def __init__(self, p, c, nseg, ext):
        self.p, self.c = p, c
        self.ybuf = randn(p, c + 24)
        self.y = self.ybuf[:, 8:8 + c]
        cols = split_cols(c, nseg)
        ends = cols[1:] + [c]
        self.zbufs = [filled(p, e - b + 8 * (i + 1)) for i, (b, e) in enumerate(zip(cols, ends))]
        self.zsegs = [(buf[:, 4:4 + e - b], b) for buf, b, e in zip(self.zbufs, cols, ends)]
        self.dzbufs = [randn(p, e - b + 4 * (i + 1)) for i, (b, e) in enumerate(zip(cols, ends))]
        self.dzsegs = [(buf[:, 4:4 + e - b], b) for buf, b, e in zip(self.dzbufs, cols, ends)]
        self.gamma, self.beta, self.rm, self.rv = bn_params(c)
        self.bias = randn(c, std=0.1)
        self.vec = [filled(c) for _ in range(7)]   # mean rstd scale shift dgamma dbeta dbias
        self.coef = filled(3 * c)
        if ext:       # partials made by the caller, with a pitch of their own (forward) / a part count of their own (backward)
            parts = 3
            self.pld, self.nparts = c + 4, parts
            rows = np.array_split(self.y.cpu().numpy().astype(np.float64), parts)
            part = np.zeros((parts, 2, c + 4), np.float32)
            for i, r in enumerate(rows):
                part[i, 0, :c], part[i, 1, :c] = r.sum(0), (r * r).sum(0)
            self.partial = dev(part)
            self.ext_parts = parts
            self.bpartial = randn(parts, 2, c, std=float(p) ** 0.5 / parts)
        else:
            self.partial, self.nparts = stats_partials(self.y, p, c)
            self.pld, self.ext_parts = c, 0
            self.bpartial = filled(max(1, lib().tbn_bn_bwd_partial_floats(p, c)))

    def fwd_desc(self):
        d = BnFwdDesc()
        d.y, d.y_ld, d.p, d.c = self.y.data_ptr(), self.y.stride(0), self.p, self.c
        d.partial, d.pld, d.nparts = self.partial.data_ptr(), self.pld, self.nparts
        d.gamma, d.beta, d.conv_bias = self.gamma.data_ptr(), self.beta.data_ptr(), self.bias.data_ptr()
        d.running_mean, d.running_var = self.rm.data_ptr(), self.rv.data_ptr()
        d.save_mean, d.save_rstd, d.scale, d.shift = (v.data_ptr() for v in self.vec[:4])
        d.seg, d.nseg = seg3(self.zsegs), len(self.zsegs)
        return d

    def bwd_desc(self):
        d = BnBwdDesc()
        d.dz, d.nseg = seg3(self.dzsegs), len(self.dzsegs)
        d.y, d.dy, d.y_ld, d.p, d.c = self.y.data_ptr(), self.y.data_ptr(), self.y.stride(0), self.p, self.c   # in place
        d.scale, d.shift, d.mean, d.rstd = (self.vec[i].data_ptr() for i in (2, 3, 0, 1))
        d.partial, d.ext_parts, d.coef = self.bpartial.data_ptr(), self.ext_parts, self.coef.data_ptr()
        d.dgamma, d.dbeta, d.dbias = (v.data_ptr() for v in self.vec[4:])
        return d

    def outputs(self):
        return self.zbufs + self.vec + [self.rm, self.rv, self.coef, self.ybuf] + ([] if self.ext_parts else [self.bpartial])


def bn_batch(p, c):
    nsegs = [n for n in (1, 2, 3) if n <= c // 4]
    members = [Member(p, c, n, ext=False) for n in nsegs] + [Member(p, c, nsegs[-1], ext=True)]
    fwd = (BnFwdDesc * len(members))(*[m.fwd_desc() for m in members])
    call("tbn_bn_fwd_batch", fwd, len(members), 0.1, 1e-5, st())
    bwd = (BnBwdDesc * len(members))(*[m.bwd_desc() for m in members])
    call("tbn_bn_bwd_batch", bwd, len(members), st())
    emit("bn_batch p%d c%d segs%s+ext" % (p, c, "".join(map(str, nsegs))), [t for m in members for t in m.outputs()])


# ---------------------------------------------------------------- BN fused with a 3x3 max pool
def pool_out(size, s, p):
    o = -(-(size + 2 * p - 3) // s) + 1
    return o - 1 if (o - 1) * s >= size + p else o


def bn_maxpool(h, w, c, s, p):
    n, oh, ow = 2, pool_out(h, s, p), pool_out(w, s, p)
    y = halves(n, h, w, c)
    gamma, beta, rm, rv = bn_params(c)
    mean, rstd, scale, shift, dgamma, dbeta = (filled(c) for _ in range(6))
    pooled, am = filled(n, oh, ow, c + 8), filled(n, oh, ow, c, dtype=torch.uint8)
    dpool, dy = randn(n, oh, ow, c + 4), filled(n, h, w, c)
    ws = filled(lib().tbn_bn_workspace_floats(n * h * w, c))
    call("tbn_bn_relu_maxpool_train_fwd", y.data_ptr(), n, h, w, c, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
         rv.data_ptr(), 0.1, 1e-5, mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(),
         pooled.data_ptr() + 16, c + 8, am.data_ptr(), oh, ow, s, p, ws.data_ptr(), st())
    call("tbn_bn_relu_maxpool_train_bwd", dpool.data_ptr(), c + 4, am.data_ptr(), y.data_ptr(), n, h, w, c, oh, ow, s, p,
         mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), dy.data_ptr(), dgamma.data_ptr(),
         dbeta.data_ptr(), ws.data_ptr(), st())
    emit("bn_relu_maxpool %dx%d c%d s%dp%d" % (h, w, c, s, p), [pooled, am, mean, rstd, scale, shift, rm, rv, dy, dgamma, dbeta])


# ---------------------------------------------------------------- the residual join
def bn_res(p, c):
    y, res, dz = randn(p, c + 8), randn(p, c + 4), randn(p, c + 12)
    gamma, beta, rm, rv = bn_params(c)
    rows = np.array_split(y[:, :c].cpu().numpy().astype(np.float64), 2)
    partial = dev(np.stack([np.stack([r.sum(0), (r * r).sum(0)]) for r in rows]))
    mean, rstd, scale, shift = (filled(c) for _ in range(4))
    out = []
    for has_res in (0, 1):
        for relu in (0, 1):
            z = filled(p, c + 16)
            call("tbn_bn_res_fwd", y.data_ptr(), c + 8, p, c, partial.data_ptr(), c, 2, gamma.data_ptr(), beta.data_ptr(),
                 rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(),
                 shift.data_ptr(), res.data_ptr() if has_res else 0, c + 4, relu, z.data_ptr(), c + 16, st())
            z2 = filled(p, c + 16)
            call("tbn_bn_res_apply", y.data_ptr(), c + 8, p, c, scale.data_ptr(), shift.data_ptr(),
                 res.data_ptr() if has_res else 0, c + 4, relu, z2.data_ptr(), c + 16, st())
            out += [z, z2, mean.clone(), rstd.clone(), scale.clone(), shift.clone(), rm.clone(), rv.clone()]
            ws = filled(lib().tbn_bn_res_bwd_workspace_floats(p, c))
            for dres_mode in ((0, 0), (1, 0), (1, 1)):        # no dres, dres written, dres accumulated
                dy, dres, dgamma, dbeta = filled(p, c + 20), randn(p, c + 4), filled(c), filled(c)
                call("tbn_bn_res_bwd", dz.data_ptr(), c + 12, z.data_ptr(), c + 16, y.data_ptr(), c + 8, p, c,
                     mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), relu, dy.data_ptr(), c + 20,
                     dres.data_ptr() if dres_mode[0] else 0, c + 4, dres_mode[1], dgamma.data_ptr(), dbeta.data_ptr(),
                     ws.data_ptr(), st())
                out += [dy, dres, dgamma, dbeta]
    emit("bn_res p%d c%d" % (p, c), out)


# ---------------------------------------------------------------- pools
def maxpool3(h, w, c, s, p):
    n, oh, ow = 2, pool_out(h, s, p), pool_out(w, s, p)
    x, out, am = halves(n, h, w, c + 4), filled(n, oh, ow, c + 8), filled(n, oh, ow, c, dtype=torch.uint8)
    call("tbn_maxpool3_fwd", x.data_ptr(), c + 4, out.data_ptr() + 16, c + 8, am.data_ptr(), n, h, w, c, oh, ow, s, p, st())
    dout, dins = randn(n, oh, ow, c + 8), []
    for accumulate in (0, 1):
        din = randn(n, h, w, c + 4)
        call("tbn_maxpool3_bwd", dout.data_ptr(), c + 8, am.data_ptr(), din.data_ptr(), c + 4, n, h, w, c, oh, ow, s, p,
             accumulate, st())
        dins.append(din)
    emit("maxpool3 %dx%d c%d s%dp%d" % (h, w, c, s, p), [out, am] + dins)


def avgpool3(h, w, c):
    n = 2
    x, outs = randn(n, h, w, c + 4), []
    for accumulate in (0, 1):
        out = randn(n, h, w, c + 8)
        call("tbn_avgpool3_fwd", x.data_ptr(), c + 4, out.data_ptr(), c + 8, n, h, w, c, accumulate, st())
        outs.append(out)
    emit("avgpool3 %dx%d c%d" % (h, w, c), outs)


def spatial_mean(h, w, c):
    n, outs = 2, []
    x = randn(n, h, w, c + 4)
    for freq_only in (0, 1):
        rows = n * w if freq_only else n
        out, dout, din = filled(rows, c + 8), randn(rows, c + 8), filled(n, h, w, c + 4)
        call("tbn_spatial_mean_fwd", x.data_ptr(), c + 4, out.data_ptr(), c + 8, n, h, w, c, freq_only, st())
        call("tbn_spatial_mean_bwd", dout.data_ptr(), c + 8, din.data_ptr(), c + 4, n, h, w, c, freq_only, st())
        outs += [out, din]
    emit("spatial_mean %dx%d c%d" % (h, w, c), outs)


# ---------------------------------------------------------------- the engine
def engine(cin, riders):
    from attention_based_tbn_amd.core.models.bn_inception import BNInception
    torch.manual_seed(100 + cin)
    net = BNInception(1000, cin)
    with torch.no_grad():
        net.running_var.copy_(torch.from_numpy(RNG.uniform(0.5, 1.5, net.running_var.shape).astype(np.float32)))
        net.running_mean.copy_(torch.from_numpy((RNG.standard_normal(net.running_mean.shape) * 0.1).astype(np.float32)))
    net = net.to(DEV)
    net.set_bn_trainable(True, True)
    net.autotune, net.use_riders = False, riders
    x = randn(2, cin, 64, 64)
    net.train()
    out = net(x)
    (out * randn(*out.shape)).sum().backward()
    grads = [p.grad if p.grad is not None else torch.zeros(1) for _, p in net.named_parameters()]
    emit("BNInception cin%d riders%d" % (cin, riders), [out] + grads + [b for _, b in net.named_buffers()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    for c in (8, 64, 1024):
        for p in row_counts(c):
            bn_relu_train(p, c)
            bn_stats(p, c)
            bn_batch(p, c)
        for h, w in ((5, 5), (7, 6)):
            for s, p in ((2, 0), (1, 1)):
                bn_maxpool(h, w, c, s, p)
                maxpool3(h, w, c, s, p)
            avgpool3(h, w, c)
            spatial_mean(h, w, c)
    for c in (64, 2048):
        bn_res(67, c)
    if not a.no_engine:
        for cin in (3, 10, 1):
            for riders in (True, False):
                engine(cin, riders)
    text = "\n".join(LINES) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
