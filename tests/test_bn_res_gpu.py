"""The residual join at operator level: tbn_bn_res_fwd / tbn_bn_res_apply / tbn_bn_res_bwd (attention_based_tbn_amd/csrc/
bn_res.hip) through ctypes against BatchNorm (+ residual) (+ ReLU) in float64 torch.

Bound: 1e-4 relative to the tensor's maximum (TOL of tests/test_kernels_gpu.py).  Shapes: plain; ragged rows; more than the
1024 channels the other BN entries stop at, with few rows; a channel count that is no multiple of 32 and crosses the
1024-channel slice boundary of the backward reduce; many row chunks.  The backward reference takes the ReLU decisions of the
product's own stored z (checked against the reference's z first), which is what the entry promises: the masked gradient g
-- returned as dres -- must be EXACTLY dz where z > 0 and exactly 0 where z == 0, and dy, dgamma, dbeta are those of that g."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import call, lib, ptr  # noqa: E402

DEV = "cuda"
TOL = 1e-4
EPS = 1e-5
MOM = 0.1
NAN = float("nan")
SHAPES = [(4 * 8 * 8, 64), (3 * 7 * 5, 256), (18, 2048), (50, 1028), (1000, 32)]


def st():
    return torch.cuda.current_stream().cuda_stream


def close(got, want, what):
    want = want.double().cpu()
    err = float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30))
    print("%s: %.3g" % (what, err))
    assert err < TOL, (what, err)


class Wide:
    """a (p, c) matrix as the column range [0, c) of a NaN-filled (p, c + pad) buffer"""

    def __init__(self, p, c, pad, src=None):
        self.buf = torch.full((p, c + pad), NAN, device=DEV)
        self.view = self.buf[:, :c]
        self.ld = c + pad
        if src is not None:
            self.view.copy_(src)

    def ptr(self):
        return self.buf.data_ptr()

    def padding_untouched(self):
        return self.ld == self.view.shape[1] or bool(torch.isnan(self.buf[:, self.view.shape[1]:]).all())


def inputs(p, c, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(p, c, generator=g) * (0.5 + 1.5 * torch.rand(c, generator=g)) + torch.randn(c, generator=g)
    return dict(y=y, res=torch.randn(p, c, generator=g), dz=torch.randn(p, c, generator=g),
                gamma=0.5 + torch.rand(c, generator=g), beta=0.3 * torch.randn(c, generator=g),
                rm=torch.randn(c, generator=g), rv=0.5 + torch.rand(c, generator=g))


def reference(t, res, relu, z_product=None):
    """float64 BatchNorm over the rows + residual + ReLU, and its backward for the upstream gradient t['dz']"""
    y, dz = t["y"].double(), t["dz"].double()
    gamma, beta = t["gamma"].double(), t["beta"].double()
    p = y.shape[0]
    mean, var = y.mean(0), y.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma * rstd
    shift = beta - mean * scale
    z = y * scale + shift + (t["res"].double() if res else 0.0)
    if relu:
        z = z.clamp_min(0.0)
    r = dict(mean=mean, rstd=rstd, scale=scale, shift=shift, z=z,
             rm=(1 - MOM) * t["rm"].double() + MOM * mean,
             rv=(1 - MOM) * t["rv"].double() + MOM * var * (p / max(p - 1, 1)))
    if z_product is not None:
        g = torch.where(z_product.double().cpu() > 0, dz, torch.zeros_like(dz)) if relu else dz
        xhat = (y - mean) * rstd
        r.update(g=g, dgamma=(g * xhat).sum(0), dbeta=g.sum(0),
                 dy=scale * (g - g.mean(0) - xhat * (g * xhat).mean(0)))
    return r


def torch_partials(y, chunks, pld):
    """partial[(i*2 + {0,1}) * pld + ch]: fp32 sum | sum of squares of row chunk i, computed by torch"""
    parts = torch.full((chunks * 2, pld), NAN, device=DEV)
    for i, rows in enumerate(torch.tensor_split(torch.arange(y.shape[0]), chunks)):
        blk = y[rows.to(y.device)]
        parts[2 * i, :y.shape[1]] = blk.sum(0)
        parts[2 * i + 1, :y.shape[1]] = (blk * blk).sum(0)
    return parts


def run(p, c, res, relu, seed=0, pads=(0, 0, 0, 0, 0, 0), z_alias=False, dy_alias=False, dres_init=None, t=None):
    """forward + backward of one case -> tensors on the device (views of NaN-padded buffers) and the Wide objects"""
    t = t or inputs(p, c, seed)
    y = Wide(p, c, pads[0], t["y"])
    z = y if z_alias else Wide(p, c, pads[1])
    rs = Wide(p, c, pads[2], t["res"])
    dz = Wide(p, c, pads[3], t["dz"])
    dres = Wide(p, c, pads[4], dres_init)
    d = {k: t[k].to(DEV) for k in ("gamma", "beta", "rm", "rv")}
    stats = torch.full((4, c), NAN, device=DEV)
    if c <= 1024:
        partial = torch.full((lib().tbn_bn_workspace_floats(p, c),), NAN, device=DEV)
        nparts = C.c_int(0)
        call("tbn_bn_stats_partials", y.ptr(), y.ld, p, c, ptr(partial), C.byref(nparts), st())
        nparts, pld = nparts.value, c
    else:
        nparts, pld = 3, c + 4
        partial = torch_partials(y.view, nparts, pld)
    y0 = y.view.clone()
    call("tbn_bn_res_fwd", y.ptr(), y.ld, p, c, ptr(partial), pld, nparts, ptr(d["gamma"]), ptr(d["beta"]), ptr(d["rm"]),
         ptr(d["rv"]), MOM, EPS, stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(),
         rs.ptr() if res else 0, rs.ld, int(relu), z.ptr(), z.ld, st())
    zout = z.view.clone()
    ysrc = Wide(p, c, pads[0], y0)                       # (the forward may have overwritten y)
    dy = ysrc if dy_alias else Wide(p, c, pads[5])
    ws = torch.full((lib().tbn_bn_res_bwd_workspace_floats(p, c),), NAN, device=DEV)
    dgb = torch.full((2, c), NAN, device=DEV)
    zs = Wide(p, c, pads[1], zout)
    call("tbn_bn_res_bwd", dz.ptr(), dz.ld, zs.ptr() if relu else 0, zs.ld, ysrc.ptr(), ysrc.ld, p, c, stats[0].data_ptr(),
         stats[1].data_ptr(), stats[2].data_ptr(), int(relu), dy.ptr(), dy.ld, dres.ptr() if res else 0, dres.ld,
         int(dres_init is not None), dgb[0].data_ptr(), dgb[1].data_ptr(), ptr(ws), st())
    torch.cuda.synchronize()
    return dict(t=t, z=zout, stats=stats, rm=d["rm"], rv=d["rv"], dy=dy.view.clone(), dres=dres.view.clone(), dgamma=dgb[0],
                dbeta=dgb[1], wides=dict(y=ysrc, z=z, res=rs, dz=dz, dres=dres, dy=dy))


def check(out, res, relu, what):
    ref = reference(out["t"], res, relu, z_product=out["z"])
    close(out["z"], ref["z"], what + " z")
    for i, k in enumerate(("mean", "rstd", "scale", "shift")):
        close(out["stats"][i], ref[k], what + " " + k)
    close(out["rm"], ref["rm"], what + " running_mean")
    close(out["rv"], ref["rv"], what + " running_var")
    close(out["dy"], ref["dy"], what + " dy")
    close(out["dgamma"], ref["dgamma"], what + " dgamma")
    close(out["dbeta"], ref["dbeta"], what + " dbeta")
    dz = out["t"]["dz"].to(DEV)
    if res:
        # dres is g itself: dz where the stored output is positive, exactly zero elsewhere
        want = torch.where(out["z"] > 0, dz, torch.zeros_like(dz)) if relu else dz
        assert torch.equal(out["dres"], want), what
    else:
        assert bool(torch.isnan(out["dres"]).all()), what + ": dres written without a residual"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("res", [1, 0])
@pytest.mark.parametrize("p,c", SHAPES)
def test_forward_backward_against_float64(p, c, res, relu):
    out = run(p, c, res, relu, seed=p + c)
    check(out, res, relu, "p %d c %d res %d relu %d" % (p, c, res, relu))
    if relu:
        frac = float((out["z"] == 0).float().mean())
        assert 0.05 < frac < 0.95, frac                  # both sides of the mask are exercised


@pytest.mark.parametrize("p,c", [(3 * 7 * 5, 256), (50, 1028)])
def test_pitches_wider_than_c_leave_the_padding_alone(p, c):
    out = run(p, c, 1, 1, seed=11, pads=(8, 4, 12, 4, 8, 4))
    check(out, 1, 1, "pitched p %d c %d" % (p, c))
    for k, w in out["wides"].items():
        assert w.padding_untouched(), k
    plain = run(p, c, 1, 1, seed=11)
    for k in ("z", "dy", "dres", "dgamma", "dbeta"):
        assert torch.equal(out[k], plain[k]), k          # the pitch changes addresses, not values


def test_partials_of_a_conv_epilogue_at_2048_channels():
    """statistics straight from tbn_conv2d_fwd epilogue 1 (bias-free output + per-tile sums), the training path of a
    Bottleneck's last unit: 1x1 conv 32 -> 2048 over 3 x 6 pixels"""
    n, h, w, cin, cout = 1, 3, 6, 32, 2048
    p = n * h * w
    g = torch.Generator().manual_seed(21)
    x = torch.randn(p, cin, generator=g)
    wt = torch.randn(cout, cin, generator=g) / cin ** 0.5
    t = inputs(p, cout, 22)
    xd, wd = x.to(DEV), wt.to(DEV)
    tiles = lib().tbn_conv2d_stat_tiles(n, h, w, cin, cout, 1, 1, 0)
    partial = torch.full((tiles * 2 * cout,), NAN, device=DEV)
    y = torch.full((p, cout), NAN, device=DEV)
    call("tbn_conv2d_fwd", ptr(xd), cin, ptr(wd), 0, ptr(y), cout, n, h, w, cin, cout, 1, 1, 0, 1, 0, 0, 0, ptr(partial), st())
    close(y, x.double() @ wt.double().t(), "conv output")
    d = {k: t[k].to(DEV) for k in ("gamma", "beta", "rm", "rv", "res")}
    stats = torch.full((4, cout), NAN, device=DEV)
    z = torch.full((p, cout), NAN, device=DEV)
    call("tbn_bn_res_fwd", ptr(y), cout, p, cout, ptr(partial), cout, tiles, ptr(d["gamma"]), ptr(d["beta"]), ptr(d["rm"]),
         ptr(d["rv"]), MOM, EPS, stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(),
         ptr(d["res"]), cout, 1, ptr(z), cout, st())
    t["y"] = (x.double() @ wt.double().t()).float()
    ref = reference(t, 1, 1)
    close(z, ref["z"], "z")
    close(stats[0], ref["mean"], "mean")
    close(stats[1], ref["rstd"], "rstd")
    close(d["rv"], ref["rv"], "running_var")


@pytest.mark.parametrize("p,c", [(4 * 8 * 8, 64), (18, 2048)])
def test_apply_is_the_forwards_apply_pass(p, c):
    """tbn_bn_res_apply with the scale / shift the forward finalized gives the forward's z bit for bit (eval-mode join:
    the same pass with folded running statistics); in place as well"""
    for res, relu in ((1, 1), (0, 0), (1, 0), (0, 1)):
        out = run(p, c, res, relu, seed=5)
        t = out["t"]
        y, r = t["y"].to(DEV), t["res"].to(DEV)
        z = torch.full((p, c), NAN, device=DEV)
        call("tbn_bn_res_apply", ptr(y), c, p, c, out["stats"][2].data_ptr(), out["stats"][3].data_ptr(),
             ptr(r) if res else 0, c, relu, ptr(z), c, st())
        assert torch.equal(z, out["z"]), (res, relu)
        call("tbn_bn_res_apply", ptr(y), c, p, c, out["stats"][2].data_ptr(), out["stats"][3].data_ptr(),
             ptr(r) if res else 0, c, relu, ptr(y), c, st())
        assert torch.equal(y, out["z"]), (res, relu)


@pytest.mark.parametrize("p,c", [(3 * 7 * 5, 256), (50, 1028)])
def test_aliasing_accumulate_and_determinism(p, c):
    base = run(p, c, 1, 1, seed=3)
    again = run(p, c, 1, 1, seed=3)
    for k in ("z", "dy", "dres", "dgamma", "dbeta", "rm", "rv", "stats"):
        assert torch.equal(base[k], again[k]), k         # bit-identical on a second run
    alias = run(p, c, 1, 1, seed=3, z_alias=True, dy_alias=True)
    for k in ("z", "dy", "dres", "dgamma", "dbeta"):
        assert torch.equal(base[k], alias[k]), k         # z written over y, dy written over y
    d0 = torch.randn(p, c, generator=torch.Generator().manual_seed(4))
    acc = run(p, c, 1, 1, seed=3, dres_init=d0)
    assert torch.equal(acc["dres"], d0.to(DEV) + base["dres"])
    assert torch.equal(acc["dy"], base["dy"])


@pytest.mark.parametrize("p,c", [(4 * 8 * 8, 64), (18, 2048)])
def test_upstream_gradient_where_z_is_zero_reaches_no_output(p, c):
    """the mask is exact: replacing dz by huge values wherever the stored z is 0 changes no bit of dy, dres, dgamma, dbeta"""
    base = run(p, c, 1, 1, seed=8)
    t = dict(base["t"])
    dead = base["z"].cpu() == 0
    assert 0.05 < float(dead.float().mean()) < 0.95
    t["dz"] = torch.where(dead, 1e6 * torch.randn(p, c, generator=torch.Generator().manual_seed(9)), t["dz"])
    other = run(p, c, 1, 1, t=t)
    assert torch.equal(other["z"], base["z"])
    for k in ("dy", "dres", "dgamma", "dbeta"):
        assert torch.equal(other[k], base[k]), k
    assert bool((other["dres"][dead.to(DEV)] == 0).all())


def test_arguments_are_checked():
    from attention_based_tbn_amd._lib import TbnHipError
    y = torch.zeros(8, 2052, device=DEV)
    s = torch.zeros(2, 2052, device=DEV)
    with pytest.raises(TbnHipError, match="4..2048"):
        call("tbn_bn_res_apply", ptr(y), 2052, 8, 2052, s[0].data_ptr(), s[1].data_ptr(), 0, 0, 1, ptr(y), 2052, st())
    with pytest.raises(TbnHipError, match="pitch"):
        call("tbn_bn_res_apply", ptr(y), 62, 8, 64, s[0].data_ptr(), s[1].data_ptr(), 0, 0, 1, ptr(y), 64, st())
    assert lib().tbn_bn_res_bwd_workspace_floats(8, 2052) == 0 and lib().tbn_bn_res_bwd_workspace_floats(8, 2048) > 0
