"""The attention heads that used to leave the library: the general multi-head attention core (tbn_mha_fwd / tbn_mha_bwd,
ops.mha_core) and the attention-weight softmax of the learnt variants (tbn_attn_weights_fwd / _bwd, ops.attn_weights),
through the C-ABI, the autograd wrappers and the modules of core/models/attention.py.

References are plain fp64 torch on the CPU from seeded CPU generators; `relerr` is relative to the reference's max.  The
bounds are the suite's own, restated from tests/test_heads_geometry_gpu.py: TOL for outputs of reduction / GEMM-type
operators, GTOL for their gradients, ETOL for weights that sum to 1."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import lib, ptr  # noqa: E402

DEV = "cuda"
TOL = 1e-4      # tests/test_heads_geometry_gpu.py: outputs of reduction / GEMM-type operators
GTOL = 2e-4     # ... their gradients
ETOL = 1e-6     # ... elementwise / averaging operators, weights that sum to 1
FILL = 3.0


def st():
    return torch.cuda.current_stream().cuda_stream


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def g(seed):
    return torch.Generator().manual_seed(seed)


def last_error():
    return lib().tbn_last_error() or b""


def wide(rows, c, ld, off, data=None):
    """a (rows, ld) device buffer filled with FILL whose columns [off, off + c) are the operand: (buffer, address of the
    slice's first float, view of the slice)"""
    buf = torch.full((rows, ld), FILL, dtype=torch.float32)
    if data is not None:
        buf[:, off:off + c] = data
    buf = buf.to(DEV)
    return buf, buf.data_ptr() + 4 * off, buf[:, off:off + c]


def guards_ok(buf, off, c):
    gd = torch.cat([buf[:, :off].reshape(-1), buf[:, off + c:].reshape(-1)]).cpu()
    return bool((gd == FILL).all())


def tailed(count, tail=64):
    return torch.full((count + tail,), FILL, dtype=torch.float32, device=DEV)


def tail_ok(buf, count):
    return bool((buf[count:].cpu() == FILL).all())


# ------------------------------------------------------------------------------------------------ 1. tbn_mha_fwd / _bwd
MHA_SHAPES = [
    # L, T, R, E, heads
    (1, 1, 1, 4, 1),        # smallest case: a one-key softmax is the constant 1
    (2, 5, 6, 128, 4),      # ordinary multi-query case
    (3, 33, 2, 100, 4),     # head_dim 25 (no float4), first T past the q1 limit
    (1, 40, 3, 128, 4),     # more than 32 keys
    (2, 257, 1, 64, 2),     # T past one wave-wide chunk of 64 and past 256
    (5, 64, 2, 6, 6),       # head_dim 1
    (1, 1024, 1, 32, 1),    # the domain edge
]


def mha_ref(q, k, v, mask, L, T, R, H):
    """q (L*R, E), k / v (T*R, E) -> ctx (L*R, E), avg (R, L, T), pre-dropout probs (R, H, L, T)"""
    E = q.shape[1]
    d = E // H
    s = torch.einsum("lrhd,trhd->rhlt", q.view(L, R, H, d), k.view(T, R, H, d)) * float(d) ** -0.5
    p = torch.softmax(s, -1)
    pd = p if mask is None else p * mask
    ctx = torch.einsum("rhlt,trhd->lrhd", pd, v.view(T, R, H, d)).reshape(L * R, E)
    return ctx, pd.mean(1), p


@functools.lru_cache(maxsize=None)
def _mha_case(shape, masked):
    """inputs and the fp64 forward / autograd backward, computed once; masked = a 0 / 2.0 dropout mask and a gradient into
    the returned weights, unmasked = both NULL"""
    L, T, R, E, H = shape
    q = torch.randn(L * R, E, generator=g(1))
    k = torch.randn(T * R, E, generator=g(2))
    v = torch.randn(T * R, E, generator=g(3))
    dctx = torch.randn(L * R, E, generator=g(4))
    mask = davg = None
    if masked:
        mask = (torch.rand(R, H, L, T, generator=g(5)) >= 0.5).float() * 2.0      # p = 0.5: 0 or 1 / (1 - p)
        davg = torch.randn(R, L, T, generator=g(6))
    qr, kr, vr = (x.double().requires_grad_() for x in (q, k, v))
    c, a, p = mha_ref(qr, kr, vr, None if mask is None else mask.double(), L, T, R, H)
    loss = (c * dctx.double()).sum()
    if masked:
        loss = loss + (a * davg.double()).sum()
    loss.backward()
    return q, k, v, dctx, mask, davg, (c.detach(), a.detach(), p.detach(), qr.grad, kr.grad, vr.grad)


def _mha_run(shape, masked):
    L, T, R, E, H = shape
    q, k, v, dctx, mask, davg, _ = _mha_case(shape, masked)
    scale = float(E // H) ** -0.5
    n = R * H * L * T
    # odd pitches and offsets: no row is 16-byte aligned; k and v are two column ranges of ONE buffer
    qb, qp, _ = wide(L * R, E, E + 7, 3, q)
    kvb = torch.full((T * R, 2 * E + 11), FILL)
    kvb[:, 3:3 + E] = k
    kvb[:, E + 6:2 * E + 6] = v
    kvb = kvb.to(DEV)
    kp, vp, kv_ld = kvb.data_ptr() + 4 * 3, kvb.data_ptr() + 4 * (E + 6), 2 * E + 11
    dcb, dcp, _ = wide(L * R, E, E + 5, 1, dctx)
    cb, cp, cv = wide(L * R, E, E + 9, 5)
    dqb, dqp, dqv = wide(L * R, E, E + 3, 2)
    dkvb = torch.full((T * R, 2 * E + 13), FILL, device=DEV)         # dk and dv: two column ranges of one buffer too
    dkp, dvp, dkv_ld = dkvb.data_ptr() + 4 * 1, dkvb.data_ptr() + 4 * (E + 7), 2 * E + 13
    probs, avg, ds = tailed(2 * n), tailed(R * L * T), tailed(n)
    md = None if mask is None else mask.to(DEV)
    dad = None if davg is None else davg.to(DEV)
    rc = lib().tbn_mha_fwd(qp, E + 7, kp, kv_ld, vp, kv_ld, ptr(md), cp, E + 9, ptr(probs), ptr(avg), L, T, R, E, H, scale,
                           st())
    assert rc == 0, last_error()
    rc = lib().tbn_mha_bwd(dcp, E + 5, ptr(dad), qp, E + 7, kp, kv_ld, vp, kv_ld, ptr(probs), ptr(md), ptr(ds), dqp, E + 3,
                           dkp, dkv_ld, dvp, dkv_ld, L, T, R, E, H, scale, st())
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert guards_ok(cb, 5, E) and guards_ok(dqb, 2, E), "ctx / dq guard columns overwritten"
    gd = torch.cat([dkvb[:, :1], dkvb[:, 1 + E:E + 7], dkvb[:, 2 * E + 7:]], 1).cpu()
    assert bool((gd == FILL).all()), "dk / dv guard columns overwritten"
    assert tail_ok(probs, 2 * n) and tail_ok(avg, R * L * T) and tail_ok(ds, n), "a contiguous output ran past its end"
    assert bool((qb.cpu()[:, 3:3 + E] == q).all()) and guards_ok(qb, 3, E) and guards_ok(dcb, 1, E)
    return {"ctx": cv.cpu().clone(), "avg": avg[:R * L * T].view(R, L, T).cpu().clone(),
            "probs": probs[:2 * n].view(2, R, H, L, T).cpu().clone(), "dq": dqv.cpu().clone(),
            "dk": dkvb[:, 1:1 + E].cpu().clone(), "dv": dkvb[:, E + 7:2 * E + 7].cpu().clone()}


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", MHA_SHAPES)
def test_mha_core_c_abi_against_fp64(shape, masked):
    """tbn_mha_fwd / tbn_mha_bwd through ctypes, pitched operands with guard columns, against fp64 autograd of
    scores -> softmax -> dropout mask -> context / head mean; with a 0 / 2.0 mask and a gradient into avg_w, and with both
    NULL; a second run must give the same bits (dk / dv sum over the queries in a fixed order)"""
    L, T, R, E, H = shape
    *_, mask, _, ref = _mha_case(shape, masked)
    c_ref, a_ref, p_ref, dq_ref, dk_ref, dv_ref = ref
    out = _mha_run(shape, masked)
    errs = {"ctx": relerr(out["ctx"], c_ref), "avg": relerr(out["avg"], a_ref), "probs": relerr(out["probs"][0], p_ref),
            "dq": relerr(out["dq"], dq_ref), "dk": relerr(out["dk"], dk_ref), "dv": relerr(out["dv"], dv_ref)}
    rowsum = float((out["probs"][0].double().sum(-1) - 1.0).abs().max())
    print("mha", shape, "mask" if masked else "nomask", errs, "rowsum", rowsum)
    assert all(bool(torch.isfinite(x).all()) for x in out.values())
    assert errs["ctx"] < TOL and errs["avg"] < TOL and errs["probs"] < TOL, errs
    assert errs["dq"] < GTOL and errs["dk"] < GTOL and errs["dv"] < GTOL, errs
    assert rowsum < ETOL, rowsum
    if masked:
        assert torch.equal(out["probs"][1], out["probs"][0] * mask)
    else:
        assert torch.equal(out["probs"][1], out["probs"][0])
        assert float((out["avg"].double().sum(-1) - 1.0).abs().max()) < ETOL
    if T == 1:      # nothing flows back into the scores of a one-key softmax
        assert float(out["dq"].abs().max()) == 0.0 and float(out["dk"].abs().max()) == 0.0
    again = _mha_run(shape, masked)
    for name in out:
        assert torch.equal(out[name], again[name]), name + " differs between two runs"


def test_mha_core_op_matches_the_c_abi():
    """ops.mha_core (autograd wrapper) on column slices of padded buffers gives the bits of the raw entries, with and
    without a gradient into the weights"""
    from attention_based_tbn_amd import ops
    shape = (3, 33, 2, 100, 4)
    L, T, R, E, H = shape
    for masked in (True, False):
        q, k, v, dctx, mask, davg, _ = _mha_case(shape, masked)
        raw = _mha_run(shape, masked)
        qd = wide(L * R, E, 128, 0, q)[2].requires_grad_()
        kd = wide(T * R, E, 128, 0, k)[2].requires_grad_()
        vd = wide(T * R, E, 128, 0, v)[2].requires_grad_()
        ctx, avg = ops.mha_core(qd, kd, vd, None if mask is None else mask.to(DEV), H, L, T, R)
        loss = (ctx * dctx.to(DEV)).sum()
        if masked:
            loss = loss + (avg * davg.to(DEV)).sum()
        loss.backward()
        assert tuple(ctx.shape) == (L * R, E) and tuple(avg.shape) == (R, L, T)
        assert torch.equal(ctx.detach().cpu(), raw["ctx"]) and torch.equal(avg.detach().cpu(), raw["avg"])
        assert torch.equal(qd.grad.cpu(), raw["dq"]) and torch.equal(kd.grad.cpu(), raw["dk"])
        assert torch.equal(vd.grad.cpu(), raw["dv"])


# --------------------------------------------------------------------------------------- 2. tbn_attn_weights_fwd / _bwd
AW_SHAPES = [(1, 1, 1), (3, 3, 8), (5, 13, 13), (2, 65, 7), (2, 1024, 3)]     # r, k, t


@functools.lru_cache(maxsize=None)
def _aw_inputs(shape, tau):
    """logits, Exp(1) noise, prototypes and the upstream gradients from the first seed whose rows are free of near-ties:
    the top-2 gap of (logits + g) / tau, in fp64, exceeds 1e-3 in every row (a precondition of the hard cases: a one-hot
    that may fall either way under fp32 rounding checks nothing)"""
    r, k, t = shape
    for seed in range(100, 164):
        gen = g(seed)
        logits = torch.randn(r, k, generator=gen) * 2.0
        noise = torch.empty(r, k).exponential_(generator=gen)
        z = (logits.double() - noise.double().log()) / tau
        if k == 1:
            break
        top = z.topk(2, dim=1).values
        if float((top[:, 0] - top[:, 1]).min()) > 1e-3 and float(noise.min()) > 0.0:
            break
    else:
        raise AssertionError("no seed gives tie-free rows")
    if k > 1:
        top = z.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-3
    protos = torch.rand(k, t, generator=gen)
    return logits, noise, protos, torch.randn(r, t, generator=gen), torch.randn(r, k, generator=gen)


def aw_ref(logits, noise, tau, hard, protos, dw):
    """fp64 forward and the straight-through gradient of F.gumbel_softmax"""
    lg = logits.double().requires_grad_()
    z = lg if noise is None else lg - noise.double().log()
    soft = torch.softmax(z / tau, 1)
    onehot = None
    m = soft
    if hard:
        onehot = torch.zeros_like(soft).scatter_(1, soft.argmax(1, keepdim=True), 1.0)
        m = (onehot - soft.detach()) + soft
    w = m if protos is None else m @ protos.double()
    (w * dw.double()).sum().backward()
    return soft.detach(), w.detach(), lg.grad, onehot


@pytest.mark.parametrize("mode", ["softmax", "gumbel_soft", "gumbel_hard"])
@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("shape", AW_SHAPES)
def test_attn_weights_c_abi_against_fp64(shape, tau, mode):
    """tbn_attn_weights_fwd / _bwd through ctypes, logits pitched with guard columns, with and without prototypes: soft and
    w against fp64, the hard value bit for bit (onehot - soft) + soft in fp32 on the kernel's own soft, dlogits against the
    fp64 straight-through gradient"""
    r, k, t = shape
    logits, noise, protos, dw_t, dw_k = _aw_inputs(shape, tau)
    hard = mode == "gumbel_hard"
    nz = None if mode == "softmax" else noise
    for with_protos in (False, True):
        pr = protos if with_protos else None
        dw = dw_t if with_protos else dw_k
        cols = t if with_protos else k
        soft_ref, w_ref, dl_ref, onehot = aw_ref(logits, nz, tau, hard, pr, dw)
        lb, lp, _ = wide(r, k, k + 5, 2, logits)
        nd = None if nz is None else nz.to(DEV)
        pd = None if pr is None else pr.to(DEV)
        soft, w, dl = tailed(r * k), tailed(r * cols), tailed(r * k)
        rc = lib().tbn_attn_weights_fwd(lp, k + 5, ptr(nd), tau, int(hard), ptr(pd), ptr(soft), ptr(w), r, k, t, st())
        assert rc == 0, last_error()
        rc = lib().tbn_attn_weights_bwd(ptr(dw.to(DEV)), ptr(soft), ptr(pd), tau, ptr(dl), r, k, t, st())
        assert rc == 0, last_error()
        torch.cuda.synchronize()
        assert tail_ok(soft, r * k) and tail_ok(w, r * cols) and tail_ok(dl, r * k) and guards_ok(lb, 2, k)
        soft_c, w_c, dl_c = soft[:r * k].view(r, k).cpu(), w[:r * cols].view(r, cols).cpu(), dl[:r * k].view(r, k).cpu()
        errs = {"soft": relerr(soft_c, soft_ref), "w": relerr(w_c, w_ref), "dlogits": relerr(dl_c, dl_ref)}
        rowsum = float((soft_c.double().sum(1) - 1.0).abs().max())
        print("attn_weights", shape, tau, mode, "protos" if with_protos else "plain", errs, "rowsum", rowsum)
        assert errs["soft"] < TOL and errs["w"] < TOL, errs
        assert rowsum < ETOL, rowsum
        if k == 1:      # a one-entry softmax is the constant 1: no gradient
            assert float(dl_c.abs().max()) == 0.0
        else:
            assert errs["dlogits"] < GTOL, errs
        if hard:
            m32 = (onehot.float() - soft_c) + soft_c        # fp32, the order F.gumbel_softmax(hard=True) evaluates
            if with_protos:
                assert relerr(w_c, m32.double() @ pr.double()) < TOL
            else:
                assert torch.equal(w_c, m32)
        elif not with_protos:
            assert torch.equal(w_c, soft_c)


def test_attn_weights_first_index_wins_a_tie():
    """equal logits, no noise: every soft value is the same and the one-hot goes to index 0, as max(dim) does"""
    r, k = 2, 70
    logits = torch.zeros(r, k, device=DEV)
    soft, w = torch.empty(r, k, device=DEV), torch.empty(r, k, device=DEV)
    rc = lib().tbn_attn_weights_fwd(ptr(logits), k, None, 1.0, 1, None, ptr(soft), ptr(w), r, k, 0, st())
    assert rc == 0, last_error()
    s = soft.cpu()
    onehot = torch.zeros(r, k)
    onehot[:, 0] = 1.0
    assert torch.equal(w.cpu(), (onehot - s) + s)


# ------------------------------------------------------------------------------------------------------- 3. module level
def _uni(T, C, one_hot, tau):
    from attention_based_tbn_amd.core.models.attention import UniModalAttention
    torch.manual_seed(11)
    return UniModalAttention(C, T, hidden_size=32, use_gumbel=True, temperature=tau, one_hot=one_hot).to(DEV)


def _proto(T, C, tau):
    from attention_based_tbn_amd.core.models.attention import PrototypeAttention
    torch.manual_seed(12)
    return PrototypeAttention(C, T, hidden_size=32, use_gumbel=True, temperature=tau).to(DEV)


def _logits(m, vis):
    from attention_based_tbn_amd import ops
    h = ops.linear(vis, m.seq[0].weight, m.seq[0].bias, relu=True)
    return ops.linear(h, m.seq[2].weight, m.seq[2].bias)


def _grads(m):
    out = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return out


MODULES = [("uni_hard", lambda: _uni(13, 64, True, 1.0)), ("uni_soft", lambda: _uni(13, 64, False, 0.5)),
           ("proto", lambda: _proto(13, 64, 1.0)), ("proto_tau", lambda: _proto(25, 64, 0.5))]


@pytest.mark.parametrize("name,make", MODULES)
def test_modules_train_keep_the_rng_stream(name, make):
    """UniModalAttention / PrototypeAttention in train mode with gumbel noise: the same seed gives the weights, the attended
    feature and the parameter gradients that F.gumbel_softmax (+ torch.matmul for the prototypes) give on the same
    device, so the modules still consume torch's RNG stream exactly as they did"""
    m = make().train()
    R, C = 5, 64
    T = m.seq[2].out_features if name.startswith("uni") else m.win_size
    vis = torch.randn(R, C, generator=g(1)).to(DEV)
    seq = torch.randn(R, T, C, generator=g(2)).to(DEV)
    dout = torch.randn(R, C, generator=g(3)).to(DEV)
    dw = torch.randn(R, T, generator=g(4)).to(DEV)
    torch.manual_seed(77)
    att, w = m.attend(vis, seq)
    ((att * dout).sum() + (w * dw).sum()).backward()
    got = _grads(m)
    torch.manual_seed(77)
    logits = _logits(m, vis)
    if name.startswith("uni"):
        w_ref = F.gumbel_softmax(logits, tau=m.temperature, hard=m.one_hot)
    else:
        w_ref = torch.matmul(F.gumbel_softmax(logits, tau=m.temperature, hard=True), m.prototype_wts)
    att_ref = (seq * w_ref.unsqueeze(2)).sum(1)
    ((att_ref * dout).sum() + (w_ref * dw).sum()).backward()
    ref = _grads(m)
    assert tuple(w.shape) == (R, T) and tuple(att.shape) == (R, C)
    errs = {"w": relerr(w, w_ref), "att": relerr(att, att_ref)}
    gerrs = {n: relerr(got[n], ref[n]) for n in ref}
    print("module train", name, errs, gerrs)
    assert errs["w"] < TOL and errs["att"] < TOL, errs
    assert all(e < GTOL for e in gerrs.values()), gerrs
    assert all(float(ref[n].abs().max()) > 0.0 for n in ref)


@pytest.mark.parametrize("name,make", MODULES[::2])
def test_modules_eval_against_fp64_softmax(name, make):
    m = make().eval()
    R, C = 5, 64
    T = m.seq[2].out_features if name.startswith("uni") else m.win_size
    vis = torch.randn(R, C, generator=g(1))
    seq = torch.randn(R, T, C, generator=g(2))
    att, w = m.attend(vis.to(DEV), seq.to(DEV))
    p = {n: t.detach().double().cpu() for n, t in m.state_dict().items()}
    h = torch.relu(vis.double() @ p["seq.0.weight"].T + p["seq.0.bias"])
    w_ref = torch.softmax(h @ p["seq.2.weight"].T + p["seq.2.bias"], 1)
    if not name.startswith("uni"):
        w_ref = w_ref @ p["prototype_wts"]
    att_ref = (seq.double() * w_ref.unsqueeze(2)).sum(1)
    errs = {"w": relerr(w, w_ref), "att": relerr(att, att_ref)}
    print("module eval", name, errs)
    assert tuple(w.shape) == (R, T)
    assert errs["w"] < TOL and errs["att"] < TOL, errs


@pytest.mark.parametrize("T", [5, 40])
def test_mha_module_general_path_train_dropout(T, monkeypatch):
    """MultiheadedAttention.forward, L = 2, key is not value, dropout 0.5 in train mode: the returned weights are the head
    mean of 0 / 2-scaled softmax rows, and out is out_proj of the context of exactly the weights the op saved"""
    from attention_based_tbn_amd import ops
    from attention_based_tbn_amd.core.models import MultiheadedAttention
    L, R, E, H, p = 2, 3, 128, 4, 0.5
    d = E // H
    torch.manual_seed(5)
    m = MultiheadedAttention(E, H, dropout=p).to(DEV).train()
    seen = []
    real = ops.mha_core
    monkeypatch.setattr(ops, "mha_core", lambda *a: (seen.append(real(*a)), seen[-1])[1])
    query = torch.randn(L, R, E, generator=g(1)).to(DEV).requires_grad_()
    key = torch.randn(T, R, E, generator=g(2)).to(DEV).requires_grad_()
    value = torch.randn(T, R, E, generator=g(3)).to(DEV).requires_grad_()
    out, w = m(query, key, value)
    assert len(seen) == 1 and tuple(out.shape) == (L, R, E) and tuple(w.shape) == (R, L, T)
    q_s, k_s, v_s, probs, mask = seen[0][0].grad_fn.saved_tensors       # before backward frees them
    (out.sum() + w.sum()).backward()
    assert sorted(set(mask.cpu().flatten().tolist())) == [0.0, 2.0] and tuple(mask.shape) == (R, H, L, T)
    assert torch.equal(probs[1], probs[0] * mask)
    assert float(w.sum(-1).max()) <= 1.0 / (1.0 - p) + ETOL and float(w.min()) >= 0.0
    assert relerr(w, probs[1].mean(1)) < ETOL
    s = torch.einsum("lrhd,trhd->rhlt", q_s.double().cpu().view(L, R, H, d), k_s.double().cpu().view(T, R, H, d))
    assert relerr(probs[0], torch.softmax(s * float(d) ** -0.5, -1)) < TOL
    ctx = torch.einsum("rhlt,trhd->lrhd", probs[1].double().cpu(), v_s.double().cpu().view(T, R, H, d)).reshape(L * R, E)
    a = m.attention_layer
    out_ref = ctx @ a.out_proj.weight.detach().double().cpu().T + a.out_proj.bias.detach().double().cpu()
    err = relerr(out.reshape(L * R, E), out_ref)
    print("mha module train T", T, err)
    assert err < TOL, err
    for t in (query, key, value, a.in_proj_weight, a.in_proj_bias):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------- 4. no vendor dispatch
def test_attention_modules_dispatch_no_vendor_op(monkeypatch):
    """with torch's bmm / matmul / softmax / gumbel_softmax / dropout made to raise, the general-shape MHA call and both
    learnt-weight modules still run forward and backward, in train and eval mode: their math is the library's"""
    from attention_based_tbn_amd.core.models import MultiheadedAttention

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(name + " was dispatched from core/models/attention.py")
        return f

    for mod, name in ((torch, "bmm"), (torch, "matmul"), (torch, "softmax"), (F, "softmax"), (F, "gumbel_softmax"),
                      (F, "dropout")):
        monkeypatch.setattr(mod, name, refuse(name))
    E, H = 128, 4
    torch.manual_seed(3)
    mha = MultiheadedAttention(E, H, dropout=0.5).to(DEV)
    for train in (True, False):
        mha.train(train)
        for L, T in ((2, 5), (1, 40)):
            query = torch.randn(L, 3, E, generator=g(1)).to(DEV).requires_grad_()
            key = torch.randn(T, 3, E, generator=g(2)).to(DEV).requires_grad_()
            value = torch.randn(T, 3, E, generator=g(3)).to(DEV).requires_grad_()
            out, w = mha(query, key, value)
            (out.sum() + (w * w).sum()).backward()
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(key.grad).all())
        for make in (MODULES[0][1], MODULES[2][1]):
            m = make().train(train)
            vis = torch.randn(5, 64, generator=g(4)).to(DEV)
            seq = torch.randn(5, 13, 64, generator=g(5)).to(DEV).requires_grad_()
            att, w = m.attend(vis, seq)
            ((att * att).sum() + (w * w).sum()).backward()
            assert bool(torch.isfinite(att).all()) and bool(torch.isfinite(seq.grad).all())
            assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("ltreh", [(1, 1025, 1, 32, 1), (1, 0, 1, 32, 1), (2, 5, 3, 130, 4), (0, 5, 3, 128, 4),
                                   (2, 5, 3, 128, 0)])
def test_mha_core_refuses_outside_its_domain(ltreh):
    """T = 1025, T = 0, e % heads != 0, L = 0, heads = 0: a negative code and a message naming mha, forward and backward,
    before any launch"""
    L, T, R, E, H = ltreh
    buf = torch.zeros(1 << 16, device=DEV)
    p = ptr(buf)
    rc = lib().tbn_mha_fwd(p, E, p, E, p, E, None, p, E, p, p, L, T, R, E, H, 0.5, st())
    assert rc < 0 and b"mha" in last_error()
    rc = lib().tbn_mha_bwd(p, E, None, p, E, p, E, p, E, p, None, p, p, E, p, E, p, E, L, T, R, E, H, 0.5, st())
    assert rc < 0 and b"mha" in last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


def test_mha_core_refuses_null_pointers_and_short_pitches():
    buf = torch.zeros(1 << 16, device=DEV)
    p = ptr(buf)
    L, T, R, E, H = 2, 5, 3, 128, 4
    fwd = [p, E, p, E, p, E, None, p, E, p, p, L, T, R, E, H, 0.5, st()]
    for i in (0, 2, 4, 7, 9, 10):                       # q, k, v, ctx, probs, avg_w
        a = list(fwd)
        a[i] = None
        assert lib().tbn_mha_fwd(*a) < 0 and b"mha" in last_error(), i
    for i in (1, 3, 5, 8):                              # a leading dimension below E
        a = list(fwd)
        a[i] = E - 1
        assert lib().tbn_mha_fwd(*a) < 0 and b"mha" in last_error(), i
    bwd = [p, E, None, p, E, p, E, p, E, p, None, p, p, E, p, E, p, E, L, T, R, E, H, 0.5, st()]
    for i in (0, 3, 5, 7, 9, 11, 12, 14, 16):           # dctx, q, k, v, probs, dscores, dq, dk, dv
        a = list(bwd)
        a[i] = None
        assert lib().tbn_mha_bwd(*a) < 0 and b"mha" in last_error(), i
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


@pytest.mark.parametrize("rkt", [(2, 0, 3), (2, 1025, 3), (0, 3, 3), (2, 3, 0), (2, 3, 1025)])
def test_attn_weights_refuses_outside_its_domain(rkt):
    """k = 0, k = 1025, r = 0, and with prototypes t = 0 / 1025: a negative code and a message naming attn_weights"""
    r, k, t = rkt
    buf = torch.zeros(1 << 16, device=DEV)
    p = ptr(buf)
    rc = lib().tbn_attn_weights_fwd(p, max(k, 1), None, 1.0, 0, p, p, p, r, k, t, st())
    assert rc < 0 and b"attn_weights" in last_error()
    rc = lib().tbn_attn_weights_bwd(p, p, p, 1.0, p, r, k, t, st())
    assert rc < 0 and b"attn_weights" in last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


def test_attn_weights_refuses_null_pointers_and_bad_tau():
    buf = torch.zeros(1 << 16, device=DEV)
    p = ptr(buf)
    fwd = [p, 3, None, 1.0, 0, None, p, p, 2, 3, 0, st()]
    for i in (0, 6, 7):                                 # logits, soft, w
        a = list(fwd)
        a[i] = None
        assert lib().tbn_attn_weights_fwd(*a) < 0 and b"attn_weights" in last_error(), i
    a = list(fwd)
    a[3] = 0.0
    assert lib().tbn_attn_weights_fwd(*a) < 0 and b"attn_weights" in last_error()
    a = list(fwd)
    a[1] = 2                                            # leading dimension below k
    assert lib().tbn_attn_weights_fwd(*a) < 0 and b"attn_weights" in last_error()
    bwd = [p, p, None, 1.0, p, 2, 3, 0, st()]
    for i in (0, 1, 4):                                 # dw, soft, dlogits
        a = list(bwd)
        a[i] = None
        assert lib().tbn_attn_weights_bwd(*a) < 0 and b"attn_weights" in last_error(), i
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
