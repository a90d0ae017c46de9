"""Training BatchNorm + ReLU at operator level: the multi-scale input generator, the float64 reference, the per-channel
checker and an fp32 emulation of the kernels' sum / sum-of-squares scheme (attention_based_tbn_amd/csrc/bn.hip,
bn_multi.hip).  Shared by tests/test_bn_batch_gpu.py, the stand-alone BN cases of tests/test_kernels_gpu.py and
tests/test_conv_variants_gpu.py, and tests/test_bn_domain_cpu.py.  numpy only.

Why per channel.  max|got - ref| / max|ref| over a whole (P, C) tensor is set by the largest channel: a channel a hundred
times smaller may be entirely wrong and pass.  Here every channel is judged on its own scale,
    err_c = max_p |got - ref| / den_c  <  TOL = 1e-4,
with den_c the channel's own max|ref| floored at the channel's natural scale (below), and the channels of one case span
five decades of standard deviation.

Checked domain.  The kernels form var = E[y^2] - mean^2 from fp32 partial sums, and z = y * scale + shift with
shift = beta - mean * scale rounded at the magnitude |mean * scale|: both lose |mean| * rstd of relative precision.  The
generator keeps |mean| <= 4 / rstd (|mean| / std <= 4; for P = 1, where the variance is 0, |mean| <= 4 sqrt(eps)), and it
makes that hold for the SAMPLE of every channel at every P by standardising the noise per channel.  emulate() runs the same
scheme in fp32 on the CPU: inside the domain it stays below 1e-5 per channel (tests/test_bn_domain_cpu.py), so TOL has
about 10x margin.  Larger |mean| / std is a property of the one-pass statistics, not of these tests.

Channel roles (c % 11, a period that no quad, finalize group or tile shares): 3 -> constant 0.0, 7 -> constant 0.5,
5 -> gamma = 0 with beta > 0, 9 -> gamma = 0 with beta < 0; every other channel has gamma of either sign.  The sums of a
constant channel are exact, so mean and rstd are known to the bit there (check_forward)."""
import numpy as np

TOL = 1e-4
EPS = 1e-5
EPS32 = float(np.float32(EPS))           # what the kernels see: eps travels as a float
RSTD_CONST = np.float32(1.0 / np.sqrt(EPS32))


def make_case(P, C, seed, bias=False):
    """one BN layer's inputs: float32 numpy arrays y (P, C), dz (P, C), gamma, beta, rm, rv, bias (C) -- see the module text"""
    rng = np.random.RandomState(seed)
    std = 10.0 ** rng.uniform(-3, 2, C)
    noise = rng.standard_normal((P, C))
    if P >= 2:
        noise = (noise - noise.mean(0)) / np.maximum(noise.std(0), 1e-300)
        mean = rng.uniform(-4, 4, C) * std
    else:
        noise[:] = 0.0
        mean = rng.uniform(-4, 4, C) * np.sqrt(EPS32)
    y = mean + std * noise
    gamma = (0.5 + rng.uniform(0, 1, C)) * rng.choice([-1.0, 1.0], C)
    beta = 0.3 * rng.standard_normal(C)
    role = np.arange(C) % 11
    y[:, role == 3] = 0.0
    y[:, role == 7] = 0.5
    gamma[(role == 5) | (role == 9)] = 0.0
    beta[role == 5] = np.abs(beta[role == 5]) + 0.1
    beta[role == 9] = -np.abs(beta[role == 9]) - 0.1
    dz = rng.standard_normal((P, C)) * 10.0 ** rng.uniform(-2, 2, C)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(P=P, C=C, y=f(y), dz=f(dz), gamma=f(gamma), beta=f(beta), rm=f(rng.standard_normal(C)),
                rv=f(rng.uniform(0.5, 1.5, C)), bias=f(rng.standard_normal(C)) if bias else None, role=role)


GEOM_C = (4, 32, 100, 352, 704, 1024)     # one quad; idle tail threads (100, 352, 704: 256 % (C / 4) != 0); one row lane
GEOM_P = (1, 2, 7, 147, 5000)             # no variance; below the row-lane count; not a multiple of the rows per workgroup


def geometry_case(P, C):
    """the inputs of the one-member geometry cases (GPU) and of the CPU emulation of the bound: same generator, same seed"""
    return make_case(P, C, seed=C * 10007 + P)


def reference(case):
    """float64 BatchNorm (batch statistics over the P rows) + ReLU of a case"""
    y = case["y"].astype(np.float64)
    P = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + EPS32)
    xhat = (y - mean) * rstd
    pre = case["gamma"].astype(np.float64) * xhat + case["beta"].astype(np.float64)
    return dict(mean=mean, var=var, unb=var * (P / (P - 1.0)) if P > 1 else var, rstd=rstd, xhat=xhat, pre=pre,
                z=np.maximum(pre, 0.0))


def reference_backward(case, ref, mask):
    """float64 gradient of relu(bn(y)) with the ReLU decisions `mask` (P, C) bool given"""
    P = case["P"]
    g = case["dz"].astype(np.float64) * mask
    gx = g * ref["xhat"]
    s1, s2 = g.sum(0), gx.sum(0)
    dy = case["gamma"].astype(np.float64) * ref["rstd"] * (g - s1 / P - ref["xhat"] * (s2 / P))
    return dict(dy=dy, dgamma=s2, dbeta=s1, g=g, gx=gx)


def chan_err(got, ref, floor):
    """err_c of the module text for (P, C) tensors or (C,) vectors; a channel whose scale is 0 must match exactly"""
    got = np.asarray(got, np.float64).reshape(-1, np.shape(ref)[-1])
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    with np.errstate(invalid="ignore"):
        num = np.abs(got - ref).max(0)
    num = np.where(np.isfinite(got).all(0), num, np.inf)
    den = np.maximum(np.abs(ref).max(0), np.asarray(floor, np.float64))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))


def assert_chan(got, ref, floor, what, tol=TOL, verbose=True):
    e = chan_err(got, ref, floor)
    c = int(np.argmax(e))
    if verbose:
        print(f"{what}: worst channel {c} err {e[c]:.3e}")
    assert bool(np.all(e < tol)), (what, "channel", c, float(e[c]))
    return float(e[c])


def z_floor(case):
    return np.abs(case["gamma"].astype(np.float64))


def dy_floor(case, ref):
    return np.abs(case["gamma"].astype(np.float64)) * ref["rstd"] * np.abs(case["dz"].astype(np.float64)).max(0)


def assert_decisions(mask, pre, den, what="relu"):
    """the product's ReLU decisions `mask` are the reference's (`pre` > 0, last axis = channel) up to rounding: at most 1e-5
    of the elements differ, each with |reference pre-activation| <= 1e-4 of its channel's scale den_c"""
    dis = np.asarray(mask) != (np.asarray(pre) > 0)
    n = int(dis.sum())
    assert n <= 1e-5 * dis.size, (what, "ReLU decisions differ on", n, "of", dis.size)
    if n:
        cols = np.nonzero(dis)[-1]
        assert bool(np.all(np.abs(np.asarray(pre)[dis]) <= 1e-4 * np.asarray(den)[cols])), (what, "a decision far from 0 differs")


def relu_mask(case, ref, z, what="relu"):
    """the product's decisions z > 0 (the backward reference runs on them), after assert_decisions"""
    mask = np.asarray(z) > 0
    assert_decisions(mask, ref["pre"], np.maximum(np.abs(ref["z"]).max(0), z_floor(case)), what)
    return mask


def product_decisions(y, scale, shift):
    """[y * scale + shift > 0] as every kernel forms it (one fused multiply-add in fp32) from the product's own scale / shift:
    the decisions of an operator that never writes z"""
    return _fma(y, scale, shift) > 0


def check_forward(case, ref, z, mean, rstd, what="fwd", verbose=True):
    """z, save_mean, save_rstd per channel, and the identities of the constant channels; returns the product's ReLU mask"""
    assert_chan(z, ref["z"], z_floor(case), what + " z", verbose=verbose)
    assert_chan(mean, ref["mean"], np.abs(ref["mean"]) + np.sqrt(ref["var"]), what + " save_mean", verbose=verbose)
    assert_chan(rstd, ref["rstd"], 0.0, what + " save_rstd", verbose=verbose)
    role, beta = case["role"], case["beta"]
    for r, v in ((3, 0.0), (7, 0.5)):
        cs = np.nonzero(role == r)[0]
        if cs.size:
            assert np.array_equal(np.asarray(mean)[cs], np.full(cs.size, v, np.float32)), (what, "mean of constant", v)
            assert np.array_equal(np.asarray(rstd)[cs], np.full(cs.size, RSTD_CONST, np.float32)), (what, "rstd of constant", v)
    cs = np.nonzero(role == 3)[0]     # y = 0: shift = beta and z = relu(beta) to the bit (for y = 0.5 shift is rounded at
    if cs.size:                       # |0.5 scale| ~ 150 |gamma|, so z is beta only up to that rounding: the 1e-4 check above)
        assert np.array_equal(np.asarray(z)[:, cs], np.broadcast_to(np.maximum(beta[cs], 0), (case["P"], cs.size))), (what, "z of 0")
    for r in (5, 9):                  # gamma = 0: scale = 0, z = relu(beta) to the bit
        cs = np.nonzero(role == r)[0]
        if cs.size:
            assert np.array_equal(np.asarray(z)[:, cs], np.broadcast_to(np.maximum(beta[cs], 0), (case["P"], cs.size))), (what, "z of gamma 0")
    return relu_mask(case, ref, z, what)


def check_running(case, ref, rm, rv, momentum, what="running", verbose=True):
    """running statistics per channel: mean + conv bias and the unbiased variance, blended with `momentum`.  Scale of the
    mean: what the blend adds up, (1 - m) |rm0| + m (|mean| + std + |bias|); of the variance, formed as E[y^2] - mean^2:
    (1 - m) rv0 + m (var + mean^2)"""
    m = float(np.float32(momentum))
    b = 0.0 if case["bias"] is None else case["bias"].astype(np.float64)
    rm0, rv0 = case["rm"].astype(np.float64), case["rv"].astype(np.float64)
    unbf = case["P"] / (case["P"] - 1.0) if case["P"] > 1 else 1.0
    assert_chan(rm, (1 - m) * rm0 + m * (ref["mean"] + b),
                (1 - m) * np.abs(rm0) + m * (np.abs(ref["mean"]) + np.sqrt(ref["var"]) + np.abs(b)), what + " running_mean", verbose=verbose)
    assert_chan(rv, (1 - m) * rv0 + m * ref["unb"], (1 - m) * rv0 + m * unbf * (ref["var"] + ref["mean"] ** 2),
                what + " running_var", verbose=verbose)


def check_backward(case, ref, bref, dy, dgamma=None, dbeta=None, what="bwd", verbose=True):
    """dy per channel; dgamma / dbeta against the scale of a sum of P signed terms, sqrt(sum of squares of the terms)"""
    assert_chan(dy, bref["dy"], dy_floor(case, ref), what + " dy", verbose=verbose)
    if dgamma is not None:
        assert_chan(dgamma, bref["dgamma"], np.sqrt((bref["gx"] ** 2).sum(0)), what + " dgamma", verbose=verbose)
    if dbeta is not None:
        assert_chan(dbeta, bref["dbeta"], np.sqrt((bref["g"] ** 2).sum(0)), what + " dbeta", verbose=verbose)


def chunk_rows(P, C):
    """rows per statistics / reduce workgroup and its row lanes (bn.hip pick_chunk)"""
    rp = 256 // (C // 4)
    pch = max(64, -(-P // 512))
    return -(-pch // rp) * rp, rp


def host_partials(a, b, bounds, pld=None, pad=np.nan):
    """partials as a conv epilogue hands them over: float64 sums of a | b (P, C) over the row chunks [bounds[i], bounds[i+1])
    cast to float32, laid out [chunk][2][pld] with the columns past C filled with `pad`"""
    C = a.shape[1]
    pld = C if pld is None else pld
    out = np.full((len(bounds) - 1, 2, pld), pad, np.float32)
    for i in range(len(bounds) - 1):
        out[i, 0, :C] = a[bounds[i]:bounds[i + 1]].astype(np.float64).sum(0)
        out[i, 1, :C] = b[bounds[i]:bounds[i + 1]].astype(np.float64).sum(0)
    return out


def ragged_bounds(P, nparts, seed=0):
    """nparts row chunks of uneven (possibly zero) length covering 0..P"""
    rng = np.random.RandomState(seed)
    cuts = np.sort(rng.randint(0, P + 1, nparts - 1)) if nparts > 1 else np.zeros(0, np.int64)
    return [0] + [int(c) for c in cuts] + [P]


# ---------------------------------------------------------------- fp32 emulation of the kernels' arithmetic
_f32 = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_f32)


def _lane_partials(P, C, step):
    """the statistics / reduce kernels' summation: per chunk, row lane r adds rows r, r + RP, ... in fp32, then the lanes are
    added in order; step(rows) -> (first addend, fused multiply-add operands a, b of the second sum)"""
    pch, rp = chunk_rows(P, C)
    out = []
    for p0 in range(0, P, pch):
        p1 = min(P, p0 + pch)
        s1, s2 = np.zeros((rp, C), _f32), np.zeros((rp, C), _f32)
        for t in range(p0, p1, rp):
            n = min(rp, p1 - t)
            g, a, b = step(slice(t, t + n))
            s1[:n] = s1[:n] + g
            s2[:n] = _fma(a, b, s2[:n])
        a1, a2 = np.zeros(C, _f32), np.zeros(C, _f32)
        for r in range(rp):
            a1 = a1 + s1[r]
            a2 = a2 + s2[r]
        out.append((a1, a2))
    return out


def emulate(case):
    """forward and backward of one layer with the kernels' number formats and order of operations (own ReLU decisions)"""
    y, dz, P, C = case["y"], case["dz"], case["P"], case["C"]
    parts = _lane_partials(P, C, lambda r: (y[r], y[r], y[r]))
    s1 = sum(p[0].astype(np.float64) for p in parts)
    s2 = sum(p[1].astype(np.float64) for p in parts)
    mean = s1 / P
    var = np.maximum(s2 / P - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + EPS32)).astype(_f32)
    sc = case["gamma"] * rstd
    mean32 = mean.astype(_f32)
    sh = _fma(-mean32, sc, case["beta"])
    pre = _fma(y, sc, sh)
    z = np.maximum(pre, _f32(0))

    def step(r):
        g = np.where(pre[r] > 0, dz[r], _f32(0))
        return g, g, (y[r] - mean32) * rstd
    parts = _lane_partials(P, C, step)
    b1 = sum(p[0].astype(np.float64) for p in parts)
    b2 = sum(p[1].astype(np.float64) for p in parts)
    sc64, rs64, mu64 = sc.astype(np.float64), rstd.astype(np.float64), mean32.astype(np.float64)
    bb = -sc64 * rs64 * (b2 / P)
    ca, cb, cc = sc, bb.astype(_f32), (-sc64 * (b1 / P) - bb * mu64).astype(_f32)
    dy = _fma(ca, np.where(pre > 0, dz, _f32(0)), _fma(cb, y, cc))
    return dict(z=z, mean=mean32, rstd=rstd, dy=dy, dgamma=b2.astype(_f32), dbeta=b1.astype(_f32), var=var)
