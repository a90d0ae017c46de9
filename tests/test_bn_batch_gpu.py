"""The backbone engine's batched training BatchNorm at operator level: tbn_bn_stats_partials / tbn_bn_fwd_batch /
tbn_bn_bwd_batch (the finalize, apply and reduce kernels of attention_based_tbn_amd/csrc/bn_multi.hip, launched as the
engine launches them) against a float64 reference of BatchNorm + ReLU over the P rows, judged PER CHANNEL on inputs whose
channels span five decades (tests/bn_check.py: checker, generator, checked domain).

Every buffer a kernel writes is a column slice of a wider buffer filled with NaN, with one guard row below: whatever lands
outside the slice, or stays unwritten inside it, is seen.  The backward reference takes the product's own ReLU decisions
(z > 0), which must be the reference's up to rounding (bn_check.relu_mask)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd._lib import BnBwdDesc, BnFwdDesc, BnSeg, call, lib, ptr  # noqa: E402
from tests import bn_check as bc  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Wide:
    """a (rows + 1, ld) NaN buffer and the column slice [col, col + C) of its first `rows` rows"""

    def __init__(self, rows, C_, ld=None, col=0, data=None):
        self.ld, self.col, self.C, self.rows = C_ if ld is None else ld, col, C_, rows
        self.buf = torch.full((rows + 1, self.ld), NAN, device=DEV)
        self.view = self.buf[:rows, col:col + C_]
        self.own = torch.zeros((rows + 1, self.ld), dtype=torch.bool, device=DEV)
        self.own[:rows, col:col + C_] = True
        if data is not None:
            self.view.copy_(dev(data))

    def claim(self, rows, col, C_):
        """a further slice of the same buffer (another member of a shared concat / fused-group buffer)"""
        self.own[:rows, col:col + C_] = True
        return self.buf[:rows, col:col + C_]

    def guards_intact(self):
        return bool(torch.isnan(self.buf[~self.own]).all())


def seg3(views):
    arr = (BnSeg * 3)()
    for i, (v, col_begin) in enumerate(views):
        arr[i] = BnSeg(v.data_ptr(), v.stride(0), col_begin)
    return arr


class Member:
    """device state of one BN layer: inputs from a bn_check case, NaN-filled outputs, and the descriptors of both passes.
    y / z / dz may be given as views into shared buffers (`y`, `zsegs`, `dzsegs`); otherwise each gets its own Wide buffer
    with the pitches of `pitched`."""

    def __init__(self, case, pitched=False, y=None, zsegs=None, dzsegs=None, partial="kernel", running=True,
                 inplace=None, grads=True, ext_bounds=None):
        P, Cn = case["P"], case["C"]
        self.case, self.P, self.C = case, P, Cn
        self.wides = []
        if y is None:
            w = Wide(P, Cn, Cn + 24, 8, case["y"]) if pitched else Wide(P, Cn, data=case["y"])
            self.wides.append(w)
            y = w.view
        else:
            y.copy_(dev(case["y"]))
        self.y, self.y_ld = y, y.stride(0)
        if zsegs is None:
            w = Wide(P, Cn, Cn + 40, 12) if pitched else Wide(P, Cn)
            self.wides.append(w)
            zsegs = [(w.view, 0)]
        self.zsegs = zsegs
        if dzsegs is None:
            w = Wide(P, Cn, Cn + 8, 4, case["dz"]) if pitched else Wide(P, Cn, data=case["dz"])
            self.wides.append(w)
            dzsegs = [(w.view, 0)]
        else:
            ends = [c0 for _, c0 in dzsegs[1:]] + [Cn]
            for (v, c0), c1 in zip(dzsegs, ends):
                v.copy_(dev(case["dz"][:, c0:c1]))
        self.dzsegs = dzsegs
        # statistics partials: from the stand-alone statistics kernel on the (pitched) y, or given by the host
        if isinstance(partial, str):
            self.partial = torch.full((lib().tbn_bn_workspace_floats(P, Cn),), NAN, device=DEV)
            n = C.c_int(-1)
            call("tbn_bn_stats_partials", y.data_ptr(), self.y_ld, P, Cn, ptr(self.partial), C.byref(n), st())
            self.nparts, self.pld = n.value, Cn
            assert self.nparts == -(-P // bc.chunk_rows(P, Cn)[0])
        else:
            self.partial, self.nparts, self.pld = dev(partial), partial.shape[0], partial.shape[2]
        self.gamma, self.beta = dev(case["gamma"]), dev(case["beta"])
        self.bias = None if case["bias"] is None else dev(case["bias"])
        self.rm, self.rv = (dev(case["rm"]), dev(case["rv"])) if running else (None, None)
        self.vec = Wide(6, Cn, Cn + 4, 0)            # save_mean | save_rstd | scale | shift | dgamma | dbeta rows, guarded
        self.mean, self.rstd, self.scale, self.shift, self.dgamma, self.dbeta = (self.vec.view[i] for i in range(6))
        self.wides.append(self.vec)
        # backward
        self.inplace = pitched if inplace is None else inplace
        if self.inplace:
            self.dy = self.y
        else:
            w = Wide(P, Cn, self.y_ld, 0)            # dy is written with y's pitch
            self.wides.append(w)
            self.dy = w.view
        self.grads = grads
        self.dbias = torch.full((Cn,), NAN, device=DEV)
        self.coef = torch.full((3 * Cn,), NAN, device=DEV)
        self.ext_bounds = ext_bounds
        self.bpartial = torch.full((max(1, lib().tbn_bn_bwd_partial_floats(P, Cn)),), NAN, device=DEV)
        self.ext_parts = 0

    def fwd_desc(self):
        d = BnFwdDesc()
        d.y, d.y_ld, d.p, d.c = self.y.data_ptr(), self.y_ld, self.P, self.C
        d.partial, d.pld, d.nparts = ptr(self.partial), self.pld, self.nparts
        d.gamma, d.beta, d.conv_bias = ptr(self.gamma), ptr(self.beta), ptr(self.bias)
        d.running_mean, d.running_var = ptr(self.rm), ptr(self.rv)
        d.save_mean, d.save_rstd, d.scale, d.shift = (v.data_ptr() for v in (self.mean, self.rstd, self.scale, self.shift))
        d.seg, d.nseg = seg3(self.zsegs), len(self.zsegs)
        return d

    def make_ext_partials(self, ref):
        """S1 | S2 partials over the row chunks `ext_bounds`, made on the host from the product's ReLU decisions"""
        mask = self.z() > 0
        g = self.case["dz"].astype(np.float64) * mask
        part = bc.host_partials(g, g * ref["xhat"], self.ext_bounds)
        self.bpartial, self.ext_parts = dev(part), part.shape[0]

    def bwd_desc(self):
        d = BnBwdDesc()
        d.dz, d.nseg = seg3(self.dzsegs), len(self.dzsegs)
        d.y, d.dy, d.y_ld, d.p, d.c = self.y.data_ptr(), self.dy.data_ptr(), self.y_ld, self.P, self.C
        d.scale, d.shift, d.mean, d.rstd = (v.data_ptr() for v in (self.scale, self.shift, self.mean, self.rstd))
        d.partial, d.ext_parts, d.coef = ptr(self.bpartial), self.ext_parts, ptr(self.coef)
        d.dgamma, d.dbeta = (self.dgamma.data_ptr(), self.dbeta.data_ptr()) if self.grads else (0, 0)
        d.dbias = ptr(self.dbias)
        return d

    def z(self):
        return torch.cat([v for v, _ in self.zsegs], dim=1).cpu().numpy()

    def guards_intact(self):
        return all(w.guards_intact() for w in self.wides)

    def outputs(self):
        """every tensor the two passes wrote, for bit comparisons between runs"""
        out = [torch.cat([v for v, _ in self.zsegs], dim=1), self.mean, self.rstd, self.scale, self.shift, self.dy,
               self.dbias, self.coef]
        if self.rm is not None:
            out += [self.rm, self.rv]
        if self.grads:
            out += [self.dgamma, self.dbeta]
        return [t.clone() for t in out]


def forward(members, momentum=0.1):
    descs = (BnFwdDesc * len(members))(*[m.fwd_desc() for m in members])
    call("tbn_bn_fwd_batch", descs, len(members), momentum, bc.EPS, st())


def backward(members):
    descs = (BnBwdDesc * len(members))(*[m.bwd_desc() for m in members])
    call("tbn_bn_bwd_batch", descs, len(members), st())


def run_and_check(members, momentum=0.1, refs=None, what=""):
    """forward + backward of a batch; every member against its float64 reference, guards intact"""
    refs = refs or [bc.reference(m.case) for m in members]
    forward(members, momentum)
    masks = []
    for i, (m, ref) in enumerate(zip(members, refs)):
        tag = f"{what} member {i} (P {m.P} C {m.C})"
        masks.append(bc.check_forward(m.case, ref, m.z(), m.mean.cpu().numpy(), m.rstd.cpu().numpy(), tag))
        sc = m.case["gamma"].astype(np.float64) * ref["rstd"]
        bc.assert_chan(m.scale.cpu().numpy(), sc, 0.0, tag + " scale")
        bc.assert_chan(m.shift.cpu().numpy(), m.case["beta"] - ref["mean"] * sc,
                       np.abs(m.case["beta"]) + np.abs(ref["mean"] * sc), tag + " shift")
        if m.rm is not None:
            bc.check_running(m.case, ref, m.rm.cpu().numpy(), m.rv.cpu().numpy(), momentum, tag)
        if m.ext_bounds is not None:
            m.make_ext_partials(ref)
        assert m.guards_intact(), tag + ": forward wrote outside its slices"
    y_before = [w.buf.clone() for m in members for w in m.wides]
    backward(members)
    for i, (m, ref, mask) in enumerate(zip(members, refs, masks)):
        tag = f"{what} member {i} (P {m.P} C {m.C})"
        bref = bc.reference_backward(m.case, ref, mask)
        bc.check_backward(m.case, ref, bref, m.dy.cpu().numpy(), m.dgamma.cpu().numpy() if m.grads else None,
                          m.dbeta.cpu().numpy() if m.grads else None, tag)
        assert same_bits(m.dbias, torch.zeros_like(m.dbias)), tag + ": dbias must be exact zeros"
        if not m.grads:
            assert bool(torch.isnan(m.vec.view[4:6]).all()), tag + ": dgamma / dbeta written although NULL"
        assert m.guards_intact(), tag + ": backward wrote outside its slices"
    # whatever the backward does not own is bit-unchanged (the in-place dy shares its buffer with y's neighbours)
    after = [w for m in members for w in m.wides]
    for b, w in zip(y_before, after):
        assert torch.equal(bits(b)[~w.own], bits(w.buf)[~w.own])
    return refs


# ---------------------------------------------------------------- geometry of one member
@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "pitched"])
@pytest.mark.parametrize("P", bc.GEOM_P)
@pytest.mark.parametrize("Cn", bc.GEOM_C)
def test_one_member_geometry(Cn, P, pitched):
    """C: one quad (4), 256 % (C / 4) != 0 so that tail threads idle (100, 352, 704), one row lane (1024).  P: 1 (variance 0,
    the unbiased factor's P > 1 branch), fewer rows than row lanes, not a multiple of the rows per apply workgroup, more
    than one statistics chunk and apply workgroup (5000).  dense: every pitch = C, dy in a buffer of its own.  pitched: y at
    column 8 of pitch C + 24 with dy written in place, z at column 12 of pitch C + 40, dz at column 4 of pitch C + 8."""
    m = Member(bc.geometry_case(P, Cn), pitched=pitched)
    run_and_check([m], what=f"C {Cn} P {P}")


# ---------------------------------------------------------------- statistics partials as a conv epilogue supplies them
HOST_P, HOST_C = 1500, 36      # 36 channels: finalize workgroups of 16, 16 and 4 channels


@pytest.fixture(scope="module")
def host_case():
    case = bc.make_case(HOST_P, HOST_C, seed=5)
    return case, bc.reference(case)


@pytest.mark.parametrize("pld", [HOST_C, HOST_C + 20], ids=["pld=C", "pld>C"])
@pytest.mark.parametrize("nparts", [1, 63, 64, 65, 255, 256, 257, 1100])
def test_host_made_partials(host_case, nparts, pld):
    """float64 chunk sums cast to fp32, in uneven chunks: the finalize's 64 row slots see a ragged first trip (1, 63, 65),
    exactly one trip (64, 255, 256), a second trip (257) and a fifth (1100); the columns past C of a pitched partial buffer
    are NaN.  Forward and backward: the backward partials are external with the same chunk count."""
    case, ref = host_case
    bounds = bc.ragged_bounds(HOST_P, nparts, seed=nparts)
    y = case["y"]
    m = Member(case, pitched=True, partial=bc.host_partials(y, y.astype(np.float64) ** 2, bounds, pld),
               ext_bounds=bc.ragged_bounds(HOST_P, nparts, seed=nparts + 1))
    assert (m.nparts, m.pld) == (nparts, pld)
    run_and_check([m], refs=[ref], what=f"nparts {nparts}")


# ---------------------------------------------------------------- batches
BATCH_SHAPES = [(147, 100), (200, 32), (61, 352), (300, 4)]      # (P, C) of members 0..3


@pytest.fixture(scope="module")
def batch_cases():
    cases = [bc.make_case(P, Cn, seed=40 + i, bias=(i % 2 == 1)) for i, (P, Cn) in enumerate(BATCH_SHAPES)]
    return cases, [bc.reference(c) for c in cases]


def make_batch(cases, order=None, ext=(), **kw):
    """members whose y are column ranges of ONE fused-group buffer (NaN columns between them) and whose z slices interleave
    in ONE concat buffer of pitch sum(C), as the siblings of an inception block; dy in place"""
    order = list(range(len(cases))) if order is None else order
    rows = max(c["P"] for c in cases)
    ysum = sum(c["C"] + 4 for c in cases)
    ybuf = Wide(rows, 0, ysum, 0)
    zbuf = Wide(rows, 0, sum(c["C"] for c in cases), 0)
    ycol = zcol = 0
    members = [None] * len(cases)
    for i in order:
        c = cases[i]
        members[i] = Member(c, y=ybuf.claim(c["P"], ycol + 4, c["C"]), zsegs=[(zbuf.claim(c["P"], zcol, c["C"]), 0)], inplace=True,
                            ext_bounds=bc.ragged_bounds(c["P"], 3, seed=i) if i in ext else None, **kw)
        members[i].wides += [ybuf, zbuf]
        ycol += c["C"] + 4
        zcol += c["C"]
    return members


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_batch_members_are_right_and_bit_identical_to_batches_of_one(batch_cases, n):
    """n members of different (P, C) in one finalize / apply / reduce launch each: every member passes the per-channel
    check, nothing outside the members' slices changes, and every output has the bits the member gets as a batch of one
    (bn_multi.hip's header: same arithmetic, same summation order)"""
    cases, refs = batch_cases[0][:n], batch_cases[1][:n]
    together = make_batch(cases)
    run_and_check(together, refs=refs, what=f"batch of {n}")
    alone = make_batch(cases)
    for m in alone:
        forward([m])
    for m in alone:
        backward([m])
    for i, (a, b) in enumerate(zip(together, alone)):
        for k, (ta, tb) in enumerate(zip(a.outputs(), b.outputs())):
            assert same_bits(ta, tb), ("member", i, "output", k)
    assert same_bits(together[0].wides[-2].buf, alone[0].wides[-2].buf)      # the whole fused-group buffer (dy in place)
    assert same_bits(together[0].wides[-1].buf, alone[0].wides[-1].buf)      # the whole concat buffer


def test_batch_is_bit_identical_to_the_stand_alone_operator(batch_cases):
    """with partials from the stand-alone statistics kernel a batch gives the bits of tbn_bn_relu_train_fwd / _bwd (one
    layer per call, flat grid-stride apply kernels): z, saved statistics, scale / shift, running statistics, dy, dgamma,
    dbeta"""
    cases, _ = batch_cases
    cases = [dict(c, bias=None) for c in cases]          # the stand-alone entry has no conv bias
    batch = make_batch(cases)
    forward(batch)
    backward(batch)
    for i, (m, c) in enumerate(zip(batch, cases)):
        P, Cn = c["P"], c["C"]
        y, dz, g, b, rm, rv = (dev(c[k]) for k in ("y", "dz", "gamma", "beta", "rm", "rv"))
        mean, rstd, scale, shift, dg, db = (torch.full((Cn,), NAN, device=DEV) for _ in range(6))
        z, dy = torch.full((P, Cn), NAN, device=DEV), torch.full((P, Cn), NAN, device=DEV)
        ws = torch.full((lib().tbn_bn_workspace_floats(P, Cn),), NAN, device=DEV)
        call("tbn_bn_relu_train_fwd", ptr(y), P, Cn, ptr(g), ptr(b), ptr(rm), ptr(rv), 0.1, bc.EPS, ptr(mean), ptr(rstd),
             ptr(scale), ptr(shift), ptr(z), Cn, ptr(ws), st())
        call("tbn_bn_relu_train_bwd", ptr(dz), Cn, ptr(y), P, Cn, ptr(mean), ptr(rstd), ptr(scale), ptr(shift), ptr(dy),
             ptr(dg), ptr(db), ptr(ws), st())
        got = dict(z=m.zsegs[0][0], mean=m.mean, rstd=m.rstd, scale=m.scale, shift=m.shift, rm=m.rm, rv=m.rv, dy=m.dy,
                   dgamma=m.dgamma, dbeta=m.dbeta)
        want = dict(z=z, mean=mean, rstd=rstd, scale=scale, shift=shift, rm=rm, rv=rv, dy=dy, dgamma=dg, dbeta=db)
        for k in got:
            assert same_bits(got[k], want[k]), ("member", i, k)


def test_two_runs_give_the_same_bits(batch_cases):
    cases, _ = batch_cases
    runs = []
    for _ in range(2):
        batch = make_batch(cases, ext=(1,))
        forward(batch)
        batch[1].make_ext_partials(batch_cases[1][1])
        backward(batch)
        runs.append([t for m in batch for t in m.outputs()] + [batch[0].wides[-2].buf, batch[0].wides[-1].buf])
    for k, (a, b) in enumerate(zip(*runs)):
        assert same_bits(a, b), k


# ---------------------------------------------------------------- running statistics
@pytest.mark.parametrize("momentum,bias,running", [(0.1, True, True), (1.0, True, True), (0.1, False, True), (1.0, False, True),
                                                   (0.1, True, False)])
def test_running_statistics(momentum, bias, running):
    """with a conv bias the running mean carries mean + bias while z and the saved mean (checked by check_forward against
    the bias-free reference) do not; momentum 1.0 leaves nothing of the old value; running_mean == NULL touches neither"""
    case = bc.make_case(147, 100, seed=7, bias=bias)
    m = Member(case, pitched=True, running=running)
    run_and_check([m], momentum=momentum, what=f"momentum {momentum} bias {bias}")
    if bias and running:      # the bias is really in there: without it the check must fail for most channels
        ref = bc.reference(case)
        e = bc.chan_err(m.rm.cpu().numpy(), (1 - momentum) * case["rm"] + momentum * ref["mean"],
                        (1 - momentum) * np.abs(case["rm"]) + momentum * (np.abs(ref["mean"]) + np.sqrt(ref["var"])))
        assert float(np.median(e)) > 1e-2


# ---------------------------------------------------------------- backward options
def test_frozen_layer_writes_no_parameter_gradients():
    """dgamma / dbeta NULL (a partial-BN layer with frozen affine parameters): dy is the same, nothing is written there,
    dbias is exact zeros"""
    case = bc.make_case(147, 100, seed=8)
    m = Member(case, pitched=True, grads=False)
    run_and_check([m], what="frozen")


@pytest.mark.parametrize("pos", [0, 1, 2, "all"])
def test_external_partials_at_every_position(batch_cases, pos):
    """a member whose S1 / S2 partials come from outside has no reduce workgroups: a zero-width entry at the first, middle
    and last position of the reduce table; with all three external no reduce launch happens at all"""
    cases, refs = batch_cases[0][:3], batch_cases[1][:3]
    batch = make_batch(cases, ext=(0, 1, 2) if pos == "all" else (pos,))
    run_and_check(batch, refs=refs, what=f"external {pos}")
    for i, m in enumerate(batch):
        assert (m.ext_parts > 0) == (pos == "all" or i == pos)


# ---------------------------------------------------------------- segments: the general body of the apply / reduce kernels
@pytest.mark.parametrize("nseg", [2, 3])
def test_column_segments(nseg):
    """z written to, and dz read from, 2 and 3 column segments with their own buffers, pitches and column offsets (every
    engine launch has one segment at column 0, which takes the shared row code instead); C = 100 with 5000 rows: idle tail
    threads, several workgroups and a row tail in the general body too"""
    for P in (5000, 7):
        case = bc.make_case(P, 100, seed=9 + nseg)
        begins = [0, 36, 72][:nseg]
        ends = begins[1:] + [100]
        zs, dzs, wides = [], [], []
        for k, (c0, c1) in enumerate(zip(begins, ends)):
            wz = Wide(P, c1 - c0, (c1 - c0) + 8 * (k + 1), 4 * k)
            wd = Wide(P, c1 - c0, (c1 - c0) + 4 * (k + 1), 4 * (k % 2))
            zs.append((wz.view, c0))
            dzs.append((wd.view, c0))
            wides += [wz, wd]
        m = Member(case, pitched=True, zsegs=zs, dzsegs=dzs)
        m.wides += wides
        run_and_check([m], what=f"{nseg} segments P {P}")
