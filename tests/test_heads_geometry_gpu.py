"""The fusion-head operators (csrc/heads.hip), the pooled means (csrc/pool.hip) and the metrics / loss kernels beyond the one
geometry the rest of the suite runs them at: every loop trip count, lane count and kernel switch of the L_q = 1 attention
core and of GroupNorm, GroupNorm on inputs with a large common offset, MultiheadedAttention calls outside the kernel's
domain, and the pitch / accumulate / NULL-able arguments of the C-ABI with sentinel-filled guard columns.

References are plain fp64 torch on the CPU from seeded CPU generators; `relerr` is relative to the reference's max.
Tolerances are the suite's own: 1e-4 for outputs of reduction / GEMM-type operators, 2e-4 for their gradients, 1e-6 for
elementwise / averaging operators, exact equality where an operator only copies, selects or multiplies by 0 / 2."""
import ctypes
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import TbnHipError, call, lib, ptr  # noqa: E402

DEV = "cuda"
TOL = 1e-4      # outputs of reduction / GEMM-type operators
GTOL = 2e-4     # their gradients
ETOL = 1e-6     # elementwise / averaging operators
NAN = float("nan")


def st():
    return torch.cuda.current_stream().cuda_stream


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def g(seed):
    return torch.Generator().manual_seed(seed)


def last_error():
    return lib().tbn_last_error() or b""


def wide(lead, c, ld, off, fill=3.0, data=None):
    """a (lead..., ld) device buffer filled with `fill` whose columns [off, off + c) are the operand (`data` if given):
    returns (buffer, address of the slice's first float, view of the slice)"""
    buf = torch.full(tuple(lead) + (ld,), fill, dtype=torch.float32)
    if data is not None:
        buf[..., off:off + c] = data
    buf = buf.to(DEV)
    return buf, buf.data_ptr() + 4 * off, buf[..., off:off + c]


def guards_ok(buf, off, c, fill=3.0):
    """every column outside [off, off + c) still holds the fill value"""
    gd = torch.cat([buf[..., :off].reshape(-1), buf[..., off + c:].reshape(-1)]).cpu()
    return bool(torch.isnan(gd).all()) if fill != fill else bool((gd == fill).all())


def tailed(count, fill=3.0, tail=64):
    """a flat device buffer of count + tail floats (the tail is a guard behind a contiguous output)"""
    return torch.full((count + tail,), fill, dtype=torch.float32, device=DEV)


def tail_ok(buf, count, fill=3.0):
    t = buf[count:].cpu()
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


# ---------------------------------------------------------------------------------------------------------------- 1. mha_q1
MHA_GEOMS = [
    # R, T, E, heads
    (3, 1, 64, 4),       # d = 16: four active lanes; T = 1: softmax is 1, dq and dk are exactly 0
    (5, 16, 128, 4),     # d = 32, last T of the <16> instantiation
    (5, 17, 128, 4),     # first T of <32>
    (7, 8, 96, 3),       # 21 waves: ragged last workgroup, odd head count
    (3, 13, 1024, 4),    # the shape of the rest of the suite, as an anchor
    (2, 32, 2048, 4),    # d = 512: two trips of the lane loop, T at the limit
    (1, 25, 1536, 2),    # d = 768: three trips
]


def mha_ref(q, kv, mask, heads):
    R, E = q.shape
    T, d = kv.shape[1], E // heads
    qh = q.view(R, heads, d)
    k = kv[..., :E].reshape(R, T, heads, d)
    v = kv[..., E:].reshape(R, T, heads, d)
    s = torch.einsum("rhd,rthd->rht", qh, k) * float(d) ** -0.5
    p = torch.softmax(s, -1)
    pd = p if mask is None else p * mask
    ctx = torch.einsum("rht,rthd->rhd", pd, v).reshape(R, E)
    return ctx, pd.mean(1), s


@functools.lru_cache(maxsize=None)
def _mha_case(geom, masked, qscale=1.0):
    """inputs and the fp64 forward / autograd backward for the three upstream-gradient patterns, computed once"""
    R, T, E, H = geom
    q = torch.randn(R, E, generator=g(1)) * qscale
    kv = torch.randn(R, T, 2 * E, generator=g(2))
    mask = None
    if masked:
        mask = (torch.rand(R, H, T, generator=g(3)) >= 0.5).float() * 2.0     # p = 0.5: 0 or 1 / (1 - p)
        mask[R - 1, H - 1] = 0.0                                              # one (r, h) row dropped entirely
    dctx = torch.randn(R, E, generator=g(4))
    davg = torch.randn(R, T, generator=g(5))
    ref = {}
    for up in ("both", "ctx", "avg"):
        qr, kvr = q.double().requires_grad_(), kv.double().requires_grad_()
        c, a, s = mha_ref(qr, kvr, None if mask is None else mask.double(), H)
        loss = 0.0
        if up != "avg":
            loss = loss + (c * dctx.double()).sum()
        if up != "ctx":
            loss = loss + (a * davg.double()).sum()
        loss.backward()
        ref[up] = (c.detach(), a.detach(), qr.grad, kvr.grad, s.detach())
    return q, kv, mask, dctx, davg, ref


def _run_mha(geom, masked, upstream, qscale=1.0):
    from attention_based_tbn_amd import ops
    R, T, E, H = geom
    d = E // H
    q, kv, mask, dctx, davg, ref = _mha_case(geom, masked, qscale)
    c_ref, a_ref, dq_ref, dkv_ref, s_ref = ref[upstream]
    qd, kvd = q.to(DEV).requires_grad_(), kv.to(DEV).requires_grad_()
    md = None if mask is None else mask.to(DEV)
    dctx_d, davg_d = dctx.to(DEV), davg.to(DEV)
    ctx, avg = ops.mha_q1(qd, kvd, md, H)
    loss = 0.0
    if upstream != "avg":
        loss = loss + (ctx * dctx_d).sum()
    if upstream != "ctx":
        loss = loss + (avg * davg_d).sum()
    loss.backward()
    dq, dk, dv = qd.grad, kvd.grad[..., :E], kvd.grad[..., E:]
    errs = {"ctx": relerr(ctx, c_ref), "avg": relerr(avg, a_ref), "dq": relerr(dq, dq_ref),
            "dk": relerr(dk, dkv_ref[..., :E]), "dv": relerr(dv, dkv_ref[..., E:])}
    print("mha_q1", geom, "mask" if masked else "nomask", upstream, errs)
    assert bool(torch.isfinite(ctx).all() and torch.isfinite(avg).all() and torch.isfinite(qd.grad).all()
                and torch.isfinite(kvd.grad).all())
    assert errs["ctx"] < TOL and errs["avg"] < TOL, errs
    assert errs["dq"] < GTOL and errs["dk"] < GTOL and errs["dv"] < GTOL, errs
    if T == 1:      # a one-key softmax is the constant 1: nothing flows back into the scores
        assert float(dq.abs().max()) == 0.0 and float(dk.abs().max()) == 0.0
    if masked:      # the fully dropped (r, h) row: no context, no score gradient
        sl = slice((H - 1) * d, H * d)
        assert float(ctx[R - 1, sl].abs().max()) == 0.0
        assert float(dq[R - 1, sl].abs().max()) == 0.0 and float(dk[R - 1, :, sl].abs().max()) == 0.0

    # the same backward through the raw C-ABI with the pointers the autograd wrapper never passes as NULL / None
    # (autograd materialises the gradient of an unused output as zeros)
    scale = float(d) ** -0.5
    out = torch.empty(R, E, device=DEV)
    probs = torch.empty(2, R, H, T, device=DEV)
    avg2 = torch.empty(R, T, device=DEV)
    qn, kvn = qd.detach(), kvd.detach()
    call("tbn_mha_q1_fwd", ptr(qn), ptr(kvn), ptr(md), ptr(out), ptr(probs), ptr(avg2), R, T, E, H, scale, st())
    assert torch.equal(out, ctx.detach()) and torch.equal(avg2, avg.detach())
    if upstream == "ctx":       # davg_w == NULL
        dq2, dkv2 = torch.full_like(qn, NAN), torch.full_like(kvn, NAN)
        call("tbn_mha_q1_bwd", ptr(dctx_d), 0, ptr(qn), ptr(kvn), ptr(probs), ptr(md), ptr(dq2), ptr(dkv2), R, T, E, H,
             scale, st())
        assert torch.equal(dq2, qd.grad) and torch.equal(dkv2, kvd.grad)
    if upstream == "avg":       # dctx is None in ops._MHAq1Fn.backward
        fake = types.SimpleNamespace(saved_tensors=(qn, kvn, probs, md), heads=H, scale=scale)
        dq3, dkv3, _, _ = ops._MHAq1Fn.backward(fake, None, davg_d)
        assert torch.equal(dq3, qd.grad) and torch.equal(dkv3, kvd.grad)
    return s_ref


@pytest.mark.parametrize("upstream", ["both", "ctx", "avg"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("geom", MHA_GEOMS)
def test_mha_q1_geometry(geom, masked, upstream):
    """ops.mha_q1 forward and backward against fp64 autograd of scores -> softmax -> dropout mask -> context / head mean:
    partly idle waves (d < 256), several trips (d > 256), both sides of the MAXT switch, T = 1 and 32, a ragged last
    workgroup, with and without a dropout mask, with a gradient into both outputs or only one of them"""
    _run_mha(geom, masked, upstream)


def test_mha_q1_large_scores_stay_finite():
    """q scaled so that the scores span about +-80: the softmax subtracts the row maximum, so nothing overflows and the
    project's tolerances still hold"""
    s = _run_mha((5, 16, 128, 4), True, "both", qscale=20.0)
    assert float(s.max()) > 60.0 and float(s.min()) < -60.0, (float(s.min()), float(s.max()))


@pytest.mark.parametrize("rteh", [(2, 33, 64, 4), (2, 0, 64, 4), (2, 8, 24, 4), (2, 8, 130, 4)])
def test_mha_q1_refuses_outside_its_domain(rteh):
    """T = 33, T = 0, head_dim = 6 and e % heads != 0: a negative code and a message naming mha_q1, forward and backward,
    before any launch"""
    R, T, E, H = rteh
    buf = torch.zeros(1 << 16, device=DEV)
    p = ptr(buf)
    rc = lib().tbn_mha_q1_fwd(p, p, None, p, p, p, R, T, E, H, 0.5, st())
    assert rc < 0 and b"mha_q1" in last_error()
    rc = lib().tbn_mha_q1_bwd(p, p, p, p, p, None, p, p, R, T, E, H, 0.5, st())
    assert rc < 0 and b"mha_q1" in last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ------------------------------------------------------------------------- 2. MultiheadedAttention outside the kernel's domain
@pytest.mark.parametrize("teh", [(40, 128, 4), (8, 100, 4)])
def test_mha_module_single_query_outside_kernel_domain(teh):
    """one query per sample, key is value, but more than 32 keys / head_dim 25: torch.nn.MultiheadAttention takes both, so
    forward must compute them (general path) -- outputs, head-averaged weights, input and parameter gradients against
    torch's module in fp64 with the same parameters -- while attend(), the kernel's own entry, keeps refusing"""
    from attention_based_tbn_amd.core.models import MultiheadedAttention
    T, E, H = teh
    R = 3
    torch.manual_seed(4)
    m = MultiheadedAttention(E, H, dropout=0.0).to(DEV).eval()
    with torch.no_grad():
        m.attention_layer.in_proj_bias.normal_(0, 0.1)
        m.attention_layer.out_proj.bias.normal_(0, 0.1)
    ref = torch.nn.MultiheadAttention(E, H, dropout=0.0, bias=True).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in m.attention_layer.state_dict().items()})
    q0 = torch.randn(1, R, E, generator=g(1))
    kv0 = torch.randn(T, R, E, generator=g(2))
    dout = torch.randn(1, R, E, generator=g(3))
    dw = torch.randn(R, 1, T, generator=g(4))
    q, kv = q0.to(DEV).requires_grad_(), kv0.to(DEV).requires_grad_()
    out, w = m(q, kv, kv)
    ((out * dout.to(DEV)).sum() + (w * dw.to(DEV)).sum()).backward()
    qr, kvr = q0.double().requires_grad_(), kv0.double().requires_grad_()
    oref, wref = ref(qr, kvr, kvr)
    ((oref * dout.double()).sum() + (wref * dw.double()).sum()).backward()
    assert tuple(out.shape) == (1, R, E) and tuple(w.shape) == (R, 1, T)
    a = m.attention_layer
    errs = {"out": relerr(out, oref), "w": relerr(w, wref), "dq": relerr(q.grad, qr.grad), "dkv": relerr(kv.grad, kvr.grad),
            "in_w": relerr(a.in_proj_weight.grad, ref.in_proj_weight.grad),
            "in_b": relerr(a.in_proj_bias.grad, ref.in_proj_bias.grad),
            "out_w": relerr(a.out_proj.weight.grad, ref.out_proj.weight.grad),
            "out_b": relerr(a.out_proj.bias.grad, ref.out_proj.bias.grad)}
    print("mha module", teh, errs)
    assert errs["out"] < TOL and errs["w"] < TOL, errs
    assert all(errs[k] < GTOL for k in ("dq", "dkv", "in_w", "in_b", "out_w", "out_b")), errs
    with pytest.raises(TbnHipError, match="mha_q1"):
        m.attend(q0[0].to(DEV), kv0.transpose(0, 1).contiguous().to(DEV))


def test_mha_module_in_domain_call_keeps_the_kernel_path(monkeypatch):
    """the TBN's own call shape (T <= 32, head_dim % 4 == 0) still runs on the wavefront kernel, not on the general path"""
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd.core.models import MultiheadedAttention
    calls = []
    real = ops.mha_q1
    monkeypatch.setattr(ops, "mha_q1", lambda *a: (calls.append(1), real(*a))[1])
    m = MultiheadedAttention(128, 4, dropout=0.0).to(DEV).eval()
    for T in (1, 32):
        kv = torch.randn(T, 2, 128, generator=g(T)).to(DEV)
        out, w = m(torch.randn(1, 2, 128, generator=g(9)).to(DEV), kv, kv)
        assert tuple(out.shape) == (1, 2, 128) and tuple(w.shape) == (2, 1, T)
    assert len(calls) == 2


# ------------------------------------------------------------------------------------------------------------- 3. GroupNorm
GN_GEOMS = [
    # R, T, C, groups
    (2, 1, 16, 4),         # 1 lane per group (no shuffle), T = 1
    (1, 32, 512, 128),     # 1 lane per group, two waves idle
    (3, 8, 96, 3),         # 8 lanes per group, 24 active threads
    (40, 3, 64, 4),        # R = 40: the gamma / beta reduction (tbn_colsum) takes its unrolled 32-row loop plus tail
    (4, 25, 1280, 80),     # ragged second c += 1024 trip
    (2, 13, 2048, 8),      # 64 lanes per group (a whole wave), two full trips
]
GN_CASES = [(geom, 0.0) for geom in GN_GEOMS] + [(geom, off) for geom in GN_GEOMS[4:] for off in (16.0, 64.0)]


@pytest.mark.parametrize("geom,offset", GN_CASES)
def test_groupnorm_geometry_and_offset(geom, offset):
    """ops.group_norm forward and backward (x, gamma, beta gradients) against F.group_norm in fp64, for every lanes-per-group
    count and trip count of the kernel, and for x = offset + randn: nn.GroupNorm, which the operator replaces, loses nothing
    to a common offset, so the bounds are the project's 1e-4 / 2e-4 at every offset.
    torch's own fp32 CPU F.group_norm against the same fp64 reference at offset 64 (measured, same inputs):
      (4, 25, 1280, 80): y 2.4e-6  dx 1.3e-6  dgamma 6.9e-6  dbeta 1.0e-7
      (2, 13, 2048, 8):  y 2.2e-6  dx 2.9e-7  dgamma 6.6e-6  dbeta 8.9e-8
    i.e. more than an order of magnitude inside the bounds, while the one-pass fp32 formula var = E[x^2] - mean^2 on the
    same inputs gives y 7.0e-4 / 3.2e-4 (CPU emulation; on the MI355X a one-pass kernel measured y 5.0e-4 / 3.4e-4,
    dx 6.2e-4 / 5.2e-4 at offset 64, the mean-then-centred-variance kernel y 2.4e-6 / 1.8e-6, dx 5.4e-7 / 1.3e-7)."""
    from attention_based_tbn_amd import ops
    R, T, C, G = geom
    cpg = C // G
    x = offset + torch.randn(R, T, C, generator=g(1))
    gamma = torch.rand(C, generator=g(2)) + 0.5
    beta = torch.randn(C, generator=g(3))
    dy = torch.randn(R, T, C, generator=g(4))
    xr, gr, br = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    yr = F.group_norm(xr.permute(0, 2, 1), G, gr, br, 1e-5).permute(0, 2, 1)
    yr.backward(dy.double())
    xd, gd, bd = x.to(DEV).requires_grad_(), gamma.to(DEV).requires_grad_(), beta.to(DEV).requires_grad_()
    y = ops.group_norm(xd, gd, bd, G)
    y.backward(dy.to(DEV))
    # the saved statistics through the raw C-ABI: group mean and 1 / sqrt(biased variance + eps); same y bit for bit
    y2 = torch.full((R, T, C), NAN, device=DEV)
    mean, rstd = torch.full((R * G,), NAN, device=DEV), torch.full((R * G,), NAN, device=DEV)
    xn, gn, bn = xd.detach(), gd.detach(), bd.detach()
    call("tbn_groupnorm_fwd", ptr(xn), ptr(y2), ptr(gn), ptr(bn), ptr(mean), ptr(rstd), R, T, C, G, 1e-5, st())
    xg = x.double().view(R, T, G, cpg)
    mref = xg.mean((1, 3))
    rref = (((xg - mref.view(R, 1, G, 1)) ** 2).mean((1, 3)) + 1e-5).rsqrt()
    errs = {"y": relerr(y, yr), "dx": relerr(xd.grad, xr.grad), "dgamma": relerr(gd.grad, gr.grad),
            "dbeta": relerr(bd.grad, br.grad), "mean": relerr(mean.view(R, G), mref), "rstd": relerr(rstd.view(R, G), rref)}
    print("groupnorm", geom, offset, errs)
    assert torch.equal(y2, y.detach())
    assert errs["y"] < TOL and errs["mean"] < TOL and errs["rstd"] < TOL, errs
    assert errs["dx"] < GTOL and errs["dgamma"] < GTOL and errs["dbeta"] < GTOL, errs


@pytest.mark.parametrize("c_groups", [(48, 4), (1024, 2), (100, 3)])
def test_groupnorm_refuses_outside_its_domain(c_groups):
    """12 and 512 channels per group and C % groups != 0: a negative code and a message naming groupnorm"""
    C, G = c_groups
    buf = torch.zeros(1 << 14, device=DEV)
    p = ptr(buf)
    rc = lib().tbn_groupnorm_fwd(p, p, p, p, p, p, 2, 3, C, G, 1e-5, st())
    assert rc < 0 and b"groupnorm" in last_error()
    rc = lib().tbn_groupnorm_bwd(p, p, p, p, p, p, p, p, 2, 3, C, G, st())
    assert rc < 0 and b"groupnorm" in last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ------------------------------------------------------------------------- 4. pitches, accumulate and NULL-able arguments
@pytest.mark.parametrize("T", [1, 25])
@pytest.mark.parametrize("c", [96, 1024])
def test_pe_concat_pitched(c, T):
    """feat read from a channel slice of a wider buffer (feat_ld > c), out_ld == c + pe_dim and out_ld > c + pe_dim: the
    operator only copies, so everything is exact; pad columns are 0 over a NaN pre-fill; nothing behind the buffer moves"""
    from attention_based_tbn_amd import ops
    R, PD = 3, 10
    feat = torch.randn(R, T, c, generator=g(1))
    pe = torch.randn(PD, T, generator=g(2))
    fbuf, fptr, _ = wide((R, T), c, c + 8, 4, fill=NAN, data=feat)
    ped = pe.to(DEV)
    for out_ld in (c + PD, (c + PD + 31) // 32 * 32):
        n = R * T * out_ld
        flat = tailed(n, NAN)
        call("tbn_pe_concat_fwd", fptr, c + 8, ptr(ped), ptr(flat), out_ld, R, T, c, PD, st())
        out = flat[:n].view(R, T, out_ld).cpu()
        assert torch.equal(out[..., :c], feat)
        assert torch.equal(out[..., c:c + PD], pe.t().unsqueeze(0).expand(R, T, PD))
        assert bool((out[..., c + PD:] == 0).all()) and tail_ok(flat, n, NAN)
        # backward through the autograd wrapper: exactly the first c columns of the upstream gradient
        fd = feat.to(DEV).requires_grad_()
        dout = torch.randn(R, T, out_ld, generator=g(3))
        o2 = ops.pe_concat(fd, ped, out_ld)
        assert torch.equal(o2.detach().cpu(), out)
        o2.backward(dout.to(DEV))
        assert torch.equal(fd.grad.cpu(), dout[..., :c])
    flat = tailed(R * T * (c + PD), NAN)
    rc = lib().tbn_pe_concat_fwd(fptr, c + 8, ptr(ped), ptr(flat), c + PD - 1, R, T, c, PD, st())
    assert rc < 0 and b"pe_concat" in last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat).all())


@pytest.mark.parametrize("rtc", [(5, 1, 100), (3, 7, 100), (2, 8, 1024)])
def test_weighted_sum_pitched_and_weight_gradient(rtc):
    """tbn_weighted_sum_fwd / _bwd with out_ld / dout_ld > c (odd pitch, odd offset: the kernels are scalar), C not a multiple
    of 4, T = 1; the w.requires_grad branch of ops.weighted_sum against fp64 autograd"""
    from attention_based_tbn_amd import ops
    R, T, Cc = rtc
    ld, off = Cc + 13, 5
    f = torch.randn(R, T, Cc, generator=g(1))
    w = torch.rand(R, T, generator=g(2))
    dout = torch.randn(R, Cc, generator=g(3))
    fr, wr = f.double().requires_grad_(), w.double().requires_grad_()
    ref = (fr * wr.unsqueeze(2)).sum(1)
    ref.backward(dout.double())
    fd, wd = f.to(DEV), w.to(DEV)
    obuf, optr, oview = wide((R,), Cc, ld, off)
    call("tbn_weighted_sum_fwd", ptr(fd), ptr(wd), optr, ld, R, T, Cc, st())
    assert relerr(oview, ref) < ETOL and guards_ok(obuf, off, Cc)
    dbuf, dptr, _ = wide((R,), Cc, ld, off, fill=NAN, data=dout)
    n = R * T * Cc
    df = tailed(n)
    call("tbn_weighted_sum_bwd", dptr, ld, ptr(wd), ptr(df), R, T, Cc, st())
    assert relerr(df[:n].view(R, T, Cc), fr.grad) < ETOL and tail_ok(df, n)
    fd2, wd2 = f.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    o2 = ops.weighted_sum(fd2, wd2)
    o2.backward(dout.to(DEV))
    assert relerr(o2, ref) < ETOL and relerr(fd2.grad, fr.grad) < ETOL
    assert relerr(wd2.grad, wr.grad) < GTOL          # a sum over C channels: the reduction-gradient bound


LINEAR_MKN = [(1, 32, 32), (33, 96, 160), (96, 1056, 64)]     # both sides of the k >= 256 switch to the split-K tile kernel


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mkn", LINEAR_MKN)
def test_linear_fwd_pitched(mkn, relu):
    """tbn_linear_fwd reading x from and writing out into channel slices 32 floats narrower than their buffers (NaN in the
    input's pad columns, sentinel guards around the output), with and without ReLU"""
    m, k, n = mkn
    x = torch.randn(m, k, generator=g(1))
    w = torch.randn(n, k, generator=g(2)) / k ** 0.5
    b = torch.randn(n, generator=g(3))
    ref = F.linear(x.double(), w.double(), b.double())
    ref = F.relu(ref) if relu else ref
    xbuf, xptr, _ = wide((m,), k, k + 32, 16, fill=NAN, data=x)
    obuf, optr, oview = wide((m,), n, n + 32, 16)
    wd, bd = w.to(DEV), b.to(DEV)
    call("tbn_linear_fwd", xptr, k + 32, ptr(wd), ptr(bd), optr, n + 32, m, k, n, relu, st())
    assert relerr(oview, ref) < TOL and guards_ok(obuf, 16, n)


@pytest.mark.parametrize("mkn", LINEAR_MKN)
def test_linear_grads_pitched_accumulate_null_dbias(mkn):
    """tbn_linear_dgrad with pitched dy / dx and accumulate = 1 over a non-zero dx; tbn_linear_wgrad with pitched dy / x,
    with and without dbias"""
    m, k, n = mkn
    x = torch.randn(m, k, generator=g(1))
    w = torch.randn(n, k, generator=g(2)) / k ** 0.5
    dy = torch.randn(m, n, generator=g(4))
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    F.linear(xr, wr).backward(dy.double())
    xbuf, xptr, _ = wide((m,), k, k + 32, 16, fill=NAN, data=x)
    ybuf, yptr, _ = wide((m,), n, n + 32, 16, fill=NAN, data=dy)
    wd = w.to(DEV)
    dxbuf, dxptr, dxview = wide((m,), k, k + 32, 16)
    ws = torch.full((n * k,), NAN, device=DEV)
    call("tbn_linear_dgrad", yptr, n + 32, ptr(wd), dxptr, k + 32, m, k, n, 0, ptr(ws), st())
    assert relerr(dxview, xr.grad) < TOL and guards_ok(dxbuf, 16, k)
    call("tbn_linear_dgrad", yptr, n + 32, ptr(wd), dxptr, k + 32, m, k, n, 1, ptr(ws), st())
    assert relerr(dxview, 2 * xr.grad) < TOL and guards_ok(dxbuf, 16, k)
    nws = lib().tbn_linear_wgrad_workspace_floats(m, k, n)
    ws2 = torch.full((max(nws, 1),), NAN, device=DEV)
    dw = tailed(n * k)
    call("tbn_linear_wgrad", yptr, n + 32, xptr, k + 32, ptr(dw), 0, m, k, n, ptr(ws2), st())       # dbias == NULL
    assert relerr(dw[:n * k].view(n, k), wr.grad) < TOL and tail_ok(dw, n * k)
    dw2, db = tailed(n * k), tailed(n)
    ws2.fill_(NAN)
    call("tbn_linear_wgrad", yptr, n + 32, xptr, k + 32, ptr(dw2), ptr(db), m, k, n, ptr(ws2), st())
    assert torch.equal(dw2, dw)
    assert relerr(db[:n], dy.double().sum(0)) < TOL and tail_ok(db, n)


@pytest.mark.parametrize("rows", [1, 7, 8, 25, 57])
def test_colsum_pitched(rows):
    """tbn_colsum over a column slice (x_ld > cols, ragged last 32-column workgroup): fewer rows than row lanes, exactly
    eight, the unrolled 32-row loop with and without a tail"""
    cols, ld, off = 100, 136, 4
    x = torch.randn(rows, cols, generator=g(rows))
    xbuf, xptr, _ = wide((rows,), cols, ld, off, fill=NAN, data=x)
    obuf, optr, oview = wide((), cols, cols + 8, 4)
    call("tbn_colsum", xptr, ld, optr, rows, cols, st())
    assert relerr(oview, x.double().sum(0)) < TOL and guards_ok(obuf, 4, cols)


@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (2, 8)])
@pytest.mark.parametrize("c", [4, 96, 352, 1024])
def test_spatial_mean_pitched(c, hw):
    """tbn_spatial_mean_fwd / _bwd in both modes on channel slices: C / 4 = 1, C / 4 not a power of two (idle tail threads),
    C / 4 = 88 (ragged second grid row), C = 1024; one pixel, fewer pixels than pixel lanes, more"""
    n, (h, w) = 2, hw
    ld, off = c + 8, 4
    x = torch.randn(n, h, w, c, generator=g(1))
    xbuf, xptr, _ = wide((n, h, w), c, ld, off, fill=NAN, data=x)
    for freq in (0, 1):
        lead = (n, w) if freq else (n,)
        obuf, optr, oview = wide(lead, c, ld, off)
        call("tbn_spatial_mean_fwd", xptr, ld, optr, ld, n, h, w, c, freq, st())
        ref = x.double().mean(1) if freq else x.double().mean((1, 2))
        assert relerr(oview, ref) < ETOL and guards_ok(obuf, off, c), freq
        do = torch.randn(lead + (c,), generator=g(2))
        dbuf, dptr, _ = wide(lead, c, ld, off, fill=NAN, data=do)
        ibuf, iptr, iview = wide((n, h, w), c, ld, off)
        call("tbn_spatial_mean_bwd", dptr, ld, iptr, ld, n, h, w, c, freq, st())
        if freq:
            ref = (do.double() / h).unsqueeze(1).expand(n, h, w, c)
        else:
            ref = (do.double() / (h * w)).view(n, 1, 1, c).expand(n, h, w, c)
        assert relerr(iview, ref) < ETOL and guards_ok(ibuf, off, c), freq


def test_spatial_mean_refuses_more_than_1024_channels():
    buf = torch.zeros(2 * 2 * 1028, device=DEV)
    out = torch.zeros(1028, device=DEV)
    rc = lib().tbn_spatial_mean_fwd(ptr(buf), 1028, ptr(out), 1028, 1, 2, 2, 1028, 0, st())
    assert rc < 0 and b"spatial_mean" in last_error()


def test_avgpool3_pitched_and_accumulate():
    """tbn_avgpool3_fwd between channel slices, then accumulate = 1 over the (non-zero) result"""
    n, h, w, c = 2, 5, 7, 36
    ld, off = c + 8, 4
    x = torch.randn(n, h, w, c, generator=g(1))
    ref = F.avg_pool2d(x.double().permute(0, 3, 1, 2), 3, 1, 1, count_include_pad=True).permute(0, 2, 3, 1)
    xbuf, xptr, _ = wide((n, h, w), c, ld, off, fill=NAN, data=x)
    obuf, optr, oview = wide((n, h, w), c, ld, off)
    call("tbn_avgpool3_fwd", xptr, ld, optr, ld, n, h, w, c, 0, st())
    assert relerr(oview, ref) < ETOL and guards_ok(obuf, off, c)
    call("tbn_avgpool3_fwd", xptr, ld, optr, ld, n, h, w, c, 1, st())
    assert relerr(oview, 2 * ref) < ETOL and guards_ok(obuf, off, c)


@pytest.mark.parametrize("s_p", [(2, 0), (1, 1)])
def test_maxpool3_propagates_nan_like_torch(s_p):
    """a NaN inside a window gives NaN in exactly the outputs F.max_pool2d gives it; argmax == NULL is accepted and changes
    nothing"""
    s, p = s_p
    n, c, h, w = 1, 8, 6, 7
    x = torch.randn(n, c, h, w, generator=g(1))
    x[0, 1, 2, 3] = NAN
    x[0, 5, 0, 0] = NAN
    x[0, 6, 5, 6] = NAN
    ref = F.max_pool2d(x, 3, s, p, ceil_mode=True)
    oh, ow = ref.shape[2:]
    ref = ref.permute(0, 2, 3, 1)
    assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref[..., 0]).any())
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    outs = []
    for with_argmax in (True, False):
        y = torch.full((n, oh, ow, c), 3.0, device=DEV)
        am = torch.zeros(n * oh * ow * c, dtype=torch.uint8, device=DEV)
        call("tbn_maxpool3_fwd", ptr(xd), c, ptr(y), c, ptr(am) if with_argmax else 0, n, h, w, c, oh, ow, s, p, st())
        outs.append(y.cpu())
    assert torch.equal(torch.isnan(outs[0]), torch.isnan(ref))
    assert torch.equal(torch.nan_to_num(outs[0], nan=0.0), torch.nan_to_num(ref, nan=0.0))
    assert torch.equal(torch.nan_to_num(outs[0], nan=0.0), torch.nan_to_num(outs[1], nan=0.0))
    assert torch.equal(torch.isnan(outs[0]), torch.isnan(outs[1]))


@pytest.mark.parametrize("count", [1, 1000, 1_048_576 + 77])
def test_elementwise_kernels_counts_null_mask_in_place(count):
    """tbn_mul_mask (also in place), tbn_relu_mask_bwd (also mask == NULL) and tbn_dropout_fwd at one element, at a count that
    is no multiple of 256 and past the 4096-workgroup grid cap (a second grid-stride trip): they only select or multiply by
    0 / 2, so results are exact, and the floats behind the end stay untouched"""
    x = torch.randn(count, generator=g(1))
    m = (torch.rand(count, generator=g(2)) >= 0.5).float() * 2.0
    xd, md = x.to(DEV), m.to(DEV)
    y = tailed(count)
    call("tbn_mul_mask", ptr(xd), ptr(md), ptr(y), count, st())
    assert torch.equal(y[:count].cpu(), x * m) and tail_ok(y, count)
    z = tailed(count)
    z[:count] = xd
    call("tbn_mul_mask", ptr(z), ptr(md), ptr(z), count, st())            # in place
    assert torch.equal(z[:count].cpu(), x * m) and tail_ok(z, count)
    act = F.relu(torch.randn(count, generator=g(3)))                      # about half the activations are exactly 0
    actd = act.to(DEV)
    for mask in (md, None):
        dx = tailed(count)
        call("tbn_relu_mask_bwd", ptr(xd), ptr(actd), ptr(mask), ptr(dx), count, st())
        want = torch.where(act > 0, x, torch.zeros_like(x)) * (m if mask is not None else 1.0)
        assert torch.equal(dx[:count].cpu(), want) and tail_ok(dx, count)
        assert float(dx[:count][actd == 0].abs().max() if bool((actd == 0).any()) else 0.0) == 0.0
    rnd = torch.rand(count, generator=g(4))
    rd = rnd.to(DEV)
    yo, mo = tailed(count), tailed(count)
    call("tbn_dropout_fwd", ptr(xd), ptr(rd), 0.5, ptr(yo), ptr(mo), count, st())
    keep = (rnd >= 0.5).float() * 2.0
    assert torch.equal(mo[:count].cpu(), keep) and torch.equal(yo[:count].cpu(), x * keep)
    assert tail_ok(yo, count) and tail_ok(mo, count)


def test_broadcast_backwards_take_a_second_grid_trip():
    """tbn_weighted_sum_bwd at (9, 8, 16384) and tbn_segment_mean_bwd at (3, 25, 16384): more than 1 048 576 elements, so the
    capped grid loops; one multiplication per element"""
    R, T, Cc = 9, 8, 16384
    dout = torch.randn(R, Cc, generator=g(1))
    w = torch.rand(R, T, generator=g(2))
    dd, wd = dout.to(DEV), w.to(DEV)
    n = R * T * Cc
    df = tailed(n)
    call("tbn_weighted_sum_bwd", ptr(dd), Cc, ptr(wd), ptr(df), R, T, Cc, st())
    assert relerr(df[:n].view(R, T, Cc), dout.double().unsqueeze(1) * w.double().unsqueeze(2)) < ETOL and tail_ok(df, n)
    B, N = 3, 25
    do = torch.randn(B, Cc, generator=g(3))
    dod = do.to(DEV)
    n = B * N * Cc
    dx = tailed(n)
    call("tbn_segment_mean_bwd", ptr(dod), ptr(dx), B, N, Cc, st())
    assert relerr(dx[:n].view(B, N, Cc), (do.double() / N).unsqueeze(1).expand(B, N, Cc)) < ETOL and tail_ok(dx, n)


@pytest.mark.parametrize("b_c_k_ld", [(7, 13, 13, 20), (5, 100, 5, 128), (4, 64, 64, 67)])
def test_topk_correct_pitched_full_k_infinities(b_c_k_ld):
    """tbn_topk_correct with scores_ld > classes and values in the pad columns that would win every rank if read, k == classes,
    rows holding -inf and +inf: ranked classes, hit flags and the confusion matrix against torch.topk on distinct values"""
    B, Cc, K, ld = b_c_k_ld
    gen = g(B)
    base = torch.stack([torch.randperm(Cc, generator=gen) for _ in range(B)]).float() * 0.37 - 3.0
    base[0, 2] = -math.inf
    base[1, 5] = math.inf
    base[2, 1], base[2, 4] = math.inf, -math.inf
    target = torch.randint(0, Cc, (B,), generator=gen)
    target[1] = 5
    scores = torch.full((B, ld), 1e30)
    scores[:, :Cc] = base
    want = torch.topk(base, K, dim=1).indices.t().contiguous()           # (K, B)
    sd, td = scores.to(DEV), target.to(DEV)
    correct = torch.full((K * B + 16,), 7, dtype=torch.uint8, device=DEV)
    pred = torch.full((K * B + 16,), -7, dtype=torch.int64, device=DEV)
    conf = torch.zeros(Cc, Cc, device=DEV)
    call("tbn_topk_correct", ptr(sd), ld, ptr(td), B, Cc, K, ptr(correct), ptr(pred), ptr(conf), st())
    assert torch.equal(pred[:K * B].view(K, B).cpu(), want)
    assert torch.equal(correct[:K * B].view(K, B).cpu(), (want == target.unsqueeze(0)).to(torch.uint8))
    assert bool((pred[K * B:] == -7).all()) and bool((correct[K * B:] == 7).all())
    cref = torch.zeros(Cc, Cc)
    for b in range(B):
        cref[target[b], want[0, b]] += 1
    assert torch.equal(conf.cpu(), cref)
    correct2 = torch.full((K * B,), 7, dtype=torch.uint8, device=DEV)
    call("tbn_topk_correct", ptr(sd), ld, ptr(td), B, Cc, K, ptr(correct2), 0, 0, st())     # pred / conf_mat == NULL
    assert torch.equal(correct2, correct[:K * B])


def test_ce_heads_wide_spread_single_class_head_and_head_limit():
    """logits spread over about 200 stay finite and inside the existing 2e-6 / 1e-6 bounds (the kernel subtracts the row
    maximum); a head with a single class has loss 0 and gradient 0; four heads are accepted, five refused"""
    from attention_based_tbn_amd import ops
    B, ld = 9, 192
    heads = [(0, 125), (125, 1), (128, 40), (170, 7)]
    gen = g(7)
    raw = torch.randn(B, ld, generator=gen) * 30.0
    assert float(raw.max() - raw.min()) > 150.0
    scores = raw.to(DEV).requires_grad_()
    labels = [torch.randint(0, n, (B,), generator=gen).to(DEV) for _, n in heads]
    wts = [0.5 + 0.7 * i for i in range(len(heads))]
    losses = ops.cross_entropy_heads(scores, heads, labels)
    sum(w * l for w, l in zip(wts, losses)).backward()
    ref = raw.double().requires_grad_()
    rl = [F.cross_entropy(ref[:, o:o + n], lab.cpu()) for (o, n), lab in zip(heads, labels)]
    sum(w * l for w, l in zip(wts, rl)).backward()
    for a, b in zip(losses, rl):
        assert math.isfinite(float(a)) and abs(float(a) - float(b)) <= 2e-6 * max(1.0, abs(float(b))), (float(a), float(b))
    got, want = scores.grad.double().cpu(), ref.grad
    assert bool(torch.isfinite(got).all())
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()), float((got - want).abs().max())
    assert float(losses[1]) == 0.0 and float(got[:, 125].abs().max()) == 0.0
    covered = torch.zeros(ld, dtype=torch.bool)
    for o, n in heads:
        covered[o:o + n] = True
    assert float(got[:, ~covered].abs().max()) == 0.0
    # five heads through the raw C-ABI
    H = 5
    col0 = (ctypes.c_int * H)(0, 10, 20, 30, 40)
    ncls = (ctypes.c_int * H)(10, 10, 10, 10, 10)
    lab = torch.zeros(B, dtype=torch.int64, device=DEV)
    lptr = (ctypes.c_void_p * H)(*[lab.data_ptr()] * H)
    rowloss, loss, dsc = torch.zeros(H * B, device=DEV), torch.zeros(H, device=DEV), torch.zeros(B, ld, device=DEV)
    sd = scores.detach()
    rc = lib().tbn_ce_heads_fwd(ptr(sd), ld, B, H, col0, ncls, lptr, ptr(rowloss), ptr(loss), ptr(dsc), st())
    assert rc < 0 and b"ce_heads" in last_error()
    rc = lib().tbn_ce_heads_fwd(ptr(sd), ld, B, 4, col0, ncls, lptr, ptr(rowloss), ptr(loss), ptr(dsc), st())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss[:4]).all())
