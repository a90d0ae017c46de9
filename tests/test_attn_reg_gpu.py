"""The attention-weight regularisers as one HIP operator (tbn_attn_reg_fwd / _bwd, ops.attn_regularisers): the prior,
contrast and entropy losses of reference core/models/model.py:299-332 and core/models/contrast_loss.py:4-25.

Reference: torch on the CPU in float64 (nn.KLDivLoss / nn.MSELoss / nn.SmoothL1Loss, torch.distributions.Categorical, the
contrast formula written out below) on the same float32 inputs cast up; gradients are float64 autograd of it under a
different random upstream weight per output.  Two bounds, both asserted for every loss and for max|dw - ref|:
  * the project's 1e-3, in the form its golden checks use it (tests/test_model_gpu.py): 1e-3 * max(1, max|ref|) -- the kl
    gradient of a weight that is exactly 0 under a positive prior is -p / 1e-7, of order 1e6, where one float32 ulp is 0.1;
  * at most 4x the error of the torch float32 path get_loss ran before the operator (written out in `terms`), on the
    same inputs and GPU, plus 1e-6 (the two sum in different orders).
One deviation: the contrast loss and total of the log_rebind cases carry one float32 spacing of the reference value on top
of the second bound (test_log_rebind_reads_the_logarithm_as_get_loss_does says why).  Largest errors observed:
profiles/attn_reg.md.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.distributions import Categorical

pytestmark = pytest.mark.gpu

from attention_based_tbn_amd import ops  # noqa: E402
from attention_based_tbn_amd._lib import TbnHipError, lib, ptr  # noqa: E402

DEV = torch.device("cuda")
THRESH = 0.1                       # cfg.model.attention.contrast_thresh
T32 = float(np.float32(THRESH))
EPS32 = float(torch.finfo(torch.float32).eps)
# (r, t, w_ld): degenerate row; config-3 T; odd sizes; the default 4 s window; t beyond one wavefront's lanes; more rows than
# one block and than one pass of the row reducer; a row-pitched input
GEOMETRY = [(1, 1, 1), (3, 8, 8), (5, 13, 13), (7, 25, 25), (2, 70, 70), (257, 25, 25), (5, 13, 16)]
CRIT = {"kl": nn.KLDivLoss, "mse": nn.MSELoss, "smoothl1": nn.SmoothL1Loss}
KIND_RED = [("kl", "sum"), ("kl", "mean"), ("kl", "batchmean"), ("mse", "sum"), ("mse", "mean"), ("smoothl1", "sum"),
            ("smoothl1", "mean")]


def st():
    return torch.cuda.current_stream().cuda_stream


def make_inputs(r, t, seed, rows="softmax", kl_zeros=False, rebind=False):
    """weights: softmax of random logits (rows sum to 1) or one-hot rows (the hard gumbel path); prior: normalised uniform
    draws.  One element equals float32(thresh) exactly -- it must count as "above" -- and every other element of the tensor
    the contrast term reads stays >= 1e-4 away from the threshold (asserted here, on the CPU: a flipped decision cannot
    hide behind a tolerance)."""
    g = torch.Generator().manual_seed(seed)
    if rows == "onehot":
        w = torch.zeros(r, t)
        w[torch.arange(r), torch.randint(0, t, (r,), generator=g)] = 1.0
    else:
        w = torch.softmax(2.0 * torch.randn(r, t, generator=g), 1)
    p = torch.rand(r, t, generator=g) + 0.05
    p = p / p.sum(1, keepdim=True)
    if kl_zeros and t > 1:
        for i in range(r):
            p[i, (3 * i) % t] = 0.0                  # exact zeros in the prior ...
            if rows != "onehot":
                w[i, (3 * i + 1) % t] = 0.0          # ... and in the weights (under a positive prior: gradient -p / 1e-7)
        if rows != "onehot":
            w[0, 0] = 0.0
            p[0, 0] = 0.0                            # and both at once
    if not rebind:
        near = (w - T32).abs() < 1e-4
        w[near] = T32 + 2e-4
        if rows != "onehot" and t > 1:
            w[r // 2, t // 2] = T32                  # exactly on the threshold
    x = torch.log(w + 1e-7) if rebind else w
    on = x == T32
    assert bool(((x.double() - T32).abs()[~on] >= 1e-4).all())
    assert rebind or rows == "onehot" or t == 1 or int(on.sum()) >= 1
    return w, p


def entropy_written_out(x, eps):
    """Categorical(probs=x + 1e-6).entropy() written out, with the clamp constant explicit: torch clamps the normalised
    probabilities to [eps, 1 - eps] with the eps of THEIR dtype (torch.distributions.utils.clamp_probs)"""
    q = x + 1e-6
    p = q / q.sum(-1, keepdim=True)
    return -(p * torch.log(p.clamp(min=eps, max=1 - eps))).sum(-1)


def terms(w, p, kind, red, use_c, use_e, rebind, fp64_clamp32=False):
    """the three losses as get_loss forms them, in the dtype of w (float64 on the CPU: the reference; float32 on the
    GPU: the torch path before the operator)"""
    out = {}
    x = w
    if kind:
        inp = torch.log(w + 1e-7) if kind == "kl" else w
        out["prior"] = CRIT[kind](reduction=red)(inp, p)
    if rebind:
        x = torch.log(w + 1e-7)          # reference model.py:316-317 rebinds `wts`; :320-324 read the rebound tensor
    if use_c:
        hi = x.detach() >= T32            # ContrastLoss: the three lines of contrast_loss.py:17-21
        signed = x.masked_fill(hi, 0) - x.masked_fill(~hi, 0)
        out["contrast"] = signed.sum(dim=1).mean()
    if use_e:
        if fp64_clamp32:
            # rebound rows put normalised probabilities below float32's eps (a one-hot row: log(1 + 1e-7) > 0 among
            # log(1e-7) < 0), where float64's Categorical clamps at 2.2e-16 instead: the float32 definition, in float64
            out["entropy"] = entropy_written_out(x, EPS32).mean()
        else:
            out["entropy"] = Categorical(probs=x + 1e-6, validate_args=False).entropy().mean()
    return out


def with_total(out, mults, training, ethr):
    pm, cm, em = mults
    total = 0
    if "prior" in out:
        total = total + pm * out["prior"]
    if "contrast" in out:
        total = total + cm * out["contrast"]
    if "entropy" in out:
        if training and em > 0:
            em = em * (out["entropy"].detach() >= float(np.float32(ethr))).to(out["entropy"].dtype)
        total = total + em * out["entropy"]
    out["total"] = total
    return out


KEYS = ("prior", "contrast", "entropy", "total")


def run_path(fn, w, up):
    """losses {key: float64 value} and dw of sum_k up[k] * loss_k"""
    w = w.clone().requires_grad_(True)
    out = fn(w)
    obj = sum(up[k] * out[k] for k in KEYS if k in out and torch.is_tensor(out[k]))
    obj.backward()
    return {k: float(torch.as_tensor(out[k]).detach()) for k in KEYS if k in out}, w.grad.detach().double().cpu()


def check(r, t, ld, kind, red, use_c, use_e, mults=(0.25, 0.5, 0.75), training=False, ethr=0.2, rows="softmax", rebind=False,
          seed=0, tag="", pscale=1.0, ulps=0):
    w, p = make_inputs(r, t, 1000 * r + t + seed, rows, kl_zeros=kind == "kl", rebind=rebind)
    p = p * pscale
    g = torch.Generator().manual_seed(seed + 7)
    upv = (torch.rand(4, generator=g) + 0.5).tolist()
    up = dict(zip(KEYS, upv))
    clamp32 = rebind
    ref_l, ref_g = run_path(lambda x: with_total(terms(x, p.double(), kind, red, use_c, use_e, rebind, clamp32), mults,
                                                 training, ethr), w.double(), up)
    pd = p.to(DEV)
    par_l, par_g = run_path(lambda x: with_total(terms(x, pd, kind, red, use_c, use_e, rebind), mults, training, ethr),
                            w.to(DEV), up)
    buf = torch.full((r, ld), 7.0, device=DEV)         # guard columns: a kernel that read them would show
    buf[:, :t] = w.to(DEV)
    wd = buf[:, :t].detach().requires_grad_(True)
    pbuf = torch.full((r, ld), -3.0, device=DEV)
    pbuf[:, :t] = pd

    def op(x):
        o = ops.attn_regularisers(x, pbuf[:, :t] if kind else None, prior_kind=kind, prior_reduction=red,
                                  contrast_thresh=THRESH, use_contrast=use_c, use_entropy=use_e, mults=mults,
                                  training=training, entropy_thresh=ethr, log_rebind=rebind)
        assert [v is not None for v in o] == [bool(kind), use_c, use_e, True]
        assert all(v.dim() == 0 and v.dtype == torch.float32 for v in o if v is not None)
        return {k: v for k, v in zip(KEYS, o) if v is not None}
    got = op(wd)
    sum(up[k] * got[k] for k in got).backward()
    got_l, got_g = {k: float(v.detach()) for k, v in got.items()}, wd.grad.double().cpu()
    assert set(got_l) == set(ref_l) == set(par_l)
    assert got_g.shape == ref_g.shape and bool(torch.isfinite(got_g).all())
    errs = {}
    for k in got_l:
        errs[k] = (abs(got_l[k] - ref_l[k]), abs(par_l[k] - ref_l[k]), abs(ref_l[k]))
    errs["dw"] = (float((got_g - ref_g).abs().max()), float((par_g - ref_g).abs().max()), float(ref_g.abs().max()))
    print("attn_reg", tag, (r, t, ld), kind, red, use_c, use_e, rows, "rebind" if rebind else "",
          {k: "%.2e / %.2e (ref %.2e)" % v for k, v in errs.items()})
    for k, (e_hip, e_par, scale) in errs.items():
        assert e_hip <= 1e-3 * max(1.0, scale), (k, e_hip, scale)
        slack = ulps * float(np.spacing(np.float32(scale))) if k in ("contrast", "total") else 0.0
        assert e_hip <= 4 * e_par + 1e-6 + slack, (k, e_hip, e_par)
    return got_l, got_g, ref_l


@pytest.mark.parametrize("r,t,ld", GEOMETRY)
def test_all_three_terms_across_geometry(r, t, ld):
    """kl (batchmean) + contrast + entropy on softmax rows and on one-hot rows, at every geometry"""
    check(r, t, ld, "kl", "batchmean", True, True, tag="all3")
    check(r, t, ld, "kl", "batchmean", True, True, rows="onehot", tag="all3")


@pytest.mark.parametrize("r,t,ld", GEOMETRY)
def test_each_term_alone_across_geometry(r, t, ld):
    check(r, t, ld, "kl", "batchmean", False, False, tag="prior")
    check(r, t, ld, None, "sum", True, False, tag="contrast")
    check(r, t, ld, None, "sum", False, True, tag="entropy")
    check(r, t, ld, None, "sum", False, True, rows="onehot", tag="entropy")


@pytest.mark.parametrize("kind,red", KIND_RED)
def test_every_valid_kind_and_reduction(kind, red):
    for r, t, ld in ((5, 13, 16), (257, 25, 25)):
        check(r, t, ld, kind, red, False, False, tag="kind")
        check(r, t, ld, kind, red, True, True, rows="onehot", tag="kind")


def test_smoothl1_takes_both_branches():
    """weights and priors in [0, 1] never leave the quadratic branch: a prior scaled up puts |w - p| on both sides of 1"""
    w, p = make_inputs(5, 13, 1000 * 5 + 13)
    d = (w - 15.0 * p).abs()
    assert int((d >= 1).sum()) >= 5 and int((d < 1).sum()) >= 5 and float((d - 1).abs().min()) > 1e-4
    for red in ("sum", "mean"):
        check(5, 13, 16, "smoothl1", red, False, False, pscale=15.0, tag="smoothl1-linear")


@pytest.mark.parametrize("r,t,ld", [(3, 8, 8), (5, 13, 16), (2, 70, 70), (257, 25, 25)])
def test_log_rebind_reads_the_logarithm_as_get_loss_does(r, t, ld):
    """with the kl prior get_loss hands log(w + 1e-7) to the contrast and entropy terms (reference model.py:316-324).
    Prior, entropy and dw keep the bound "4x the torch path + 1e-6".  The contrast loss, and total which carries it, get
    ONE float32 spacing of the reference value on top -- a deviation from the bound the issue states, for these two
    quantities of these cases only.  Why: the rebound contrast loss is a sum of logarithms of magnitude 50 ... 400, where
    neighbouring float32 numbers are up to 3.05e-5 apart; both paths return a float32, and either may land on the float32
    nearest the float64 value or on its neighbour.  Measured at (2, 70): operator 3.89e-5 from the float64 value 415
    (1.3 spacings), torch path 8.40e-6 (it landed on the nearest one), so four times the torch path asks for the
    nearest float32, which a float32 sum of 70 float32 logarithms does not promise on either path."""
    check(r, t, ld, "kl", "batchmean", True, True, rebind=True, tag="rebind", ulps=1)
    check(r, t, ld, "kl", "sum", True, True, rebind=True, rows="onehot", tag="rebind", ulps=1)


def test_zero_multipliers_report_losses_and_total_carries_no_gradient():
    """epoch + 1 < decay_step: every multiplier is 0 -- the losses are still reported, total is 0 and its gradient is 0"""
    got_l, _, ref_l = check(7, 25, 25, "kl", "batchmean", True, True, mults=(0, 0, 0), training=True, tag="mults0")
    assert got_l["total"] == 0.0 and abs(got_l["prior"]) > 1e-3 and abs(got_l["entropy"]) > 1e-3
    w, p = make_inputs(7, 25, 11)
    wd = w.to(DEV).requires_grad_(True)
    o = ops.attn_regularisers(wd, p.to(DEV), prior_kind="kl", prior_reduction="batchmean", contrast_thresh=THRESH,
                              use_contrast=True, use_entropy=True, mults=(0, 0, 0), training=True, entropy_thresh=0.2)
    o[3].backward()
    assert float(wd.grad.abs().max()) == 0.0


def test_entropy_switch_off_is_decided_on_the_device():
    """peaked rows (mean entropy well below the threshold): training=True takes the entropy share out of total and of its
    gradient, training=False gives it back; flat rows (well above) keep it either way"""
    r, t, ethr = 6, 13, 1.0
    g = torch.Generator().manual_seed(5)
    peaked = torch.softmax(12.0 * torch.randn(r, t, generator=g), 1)
    flat = torch.softmax(0.1 * torch.randn(r, t, generator=g), 1)
    ent = {}
    for name, w in (("peaked", peaked), ("flat", flat)):
        ent[name] = float(Categorical(probs=w.double() + 1e-6).entropy().mean())
    assert ent["peaked"] < ethr - 0.05 and ent["flat"] > ethr + 0.05, ent       # the gap, on the CPU
    mults = (0.0, 0.0, 0.5)
    for name, w in (("peaked", peaked), ("flat", flat)):
        for training in (True, False):
            wd = w.to(DEV).requires_grad_(True)
            o = ops.attn_regularisers(wd, None, use_entropy=True, mults=mults, training=training, entropy_thresh=ethr)
            o[3].backward()
            off = training and name == "peaked"
            w64 = w.double().requires_grad_(True)
            h = Categorical(probs=w64 + 1e-6, validate_args=False).entropy().mean()
            (h * (0.0 if off else 0.5)).backward()
            assert abs(float(o[2]) - ent[name]) < 1e-5
            assert abs(float(o[3]) - (0.0 if off else 0.5 * ent[name])) < 1e-5, (name, training)
            assert float((wd.grad.double().cpu() - w64.grad).abs().max()) < 1e-5, (name, training)
            if off:
                assert float(o[3]) == 0.0 and float(wd.grad.abs().max()) == 0.0
            else:
                assert float(wd.grad.abs().max()) > 1e-3


def test_two_runs_give_the_same_bits():
    r, t = 257, 25
    w, p = make_inputs(r, t, 21, kl_zeros=True)
    res = []
    for _ in range(2):
        wd = w.to(DEV).requires_grad_(True)
        o = ops.attn_regularisers(wd, p.to(DEV), prior_kind="kl", prior_reduction="batchmean", contrast_thresh=THRESH,
                                  use_contrast=True, use_entropy=True, mults=(0.25, 0.25, 0.25), training=True,
                                  entropy_thresh=0.2)
        (o[0] * 0.3 + o[1] * 0.7 + o[2] * 1.1 + o[3]).backward()
        res.append((torch.stack(list(o)).detach().cpu(), wd.grad.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_host_checks_refuse_before_any_launch():
    w = torch.softmax(torch.randn(4, 8), 1).to(DEV)
    p = torch.softmax(torch.randn(4, 8), 1).to(DEV)
    with pytest.raises(TbnHipError, match="attn_reg.*batchmean"):
        ops.attn_regularisers(w, p, prior_kind="mse", prior_reduction="batchmean")
    with pytest.raises(TbnHipError, match="attn_reg.*batchmean"):
        ops.attn_regularisers(w, p, prior_kind="smoothl1", prior_reduction="batchmean")
    with pytest.raises(TbnHipError, match="attn_reg.*prior"):
        ops.attn_regularisers(w, None, prior_kind="kl")
    rowterms = torch.full((12,), 5.0, device=DEV)
    losses = torch.full((4,), 5.0, device=DEV)
    dw = torch.full((4, 8), 5.0, device=DEV)
    f = C.c_float

    def fwd(w_ld=8, p_=p, p_ld=8, r=4, t=8, kind=1, red=2, w_=w, rebind=0):
        return lib().tbn_attn_reg_fwd(ptr(w_), w_ld, ptr(p_), p_ld, r, t, kind, red, 1, f(0.1), 1, f(1), f(1), f(1), 0, f(0.2),
                                      rebind, ptr(rowterms), ptr(losses), st())

    def bwd(w_ld=8, dw_ld=8, kind=1, red=2):
        return lib().tbn_attn_reg_bwd(ptr(losses), ptr(w), w_ld, ptr(p), 8, ptr(losses), 4, 8, kind, red, 1, f(0.1), 1, f(1),
                                      f(1), f(1), 0, f(0.2), 0, ptr(dw), dw_ld, st())
    bad = [fwd(w_ld=7), fwd(p_ld=7), fwd(r=0), fwd(t=0), fwd(kind=4), fwd(kind=-1), fwd(red=3), fwd(p_=None), fwd(w_=None),
           fwd(kind=2, red=2), fwd(kind=3, red=2), fwd(kind=2, red=1, rebind=1), bwd(w_ld=7), bwd(dw_ld=7), bwd(kind=2, red=2)]
    for i, rc in enumerate(bad):
        assert rc < 0, i
    assert b"attn_reg" in lib().tbn_last_error()
    torch.cuda.synchronize()
    assert bool((rowterms == 5.0).all()) and bool((losses == 5.0).all()) and bool((dw == 5.0).all())   # nothing was launched
    assert fwd() == 0 and fwd(p_=None, kind=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all())


# --------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def cfg3():
    """the train_cfg3_mha configuration (prior + contrast + entropy), one training forward shared by the tests below"""
    from tests.util import load_case, prior_target
    from tests.test_model_gpu import build_product, to_dev
    cfg, modality, meta, data, inp, target = load_case("train_cfg3_mha")
    model, crit = build_product(cfg, modality, meta)
    B, n = inp[modality[0]].shape[:2]
    tgt = {"class": to_dev(target["class"]), "weights": prior_target(cfg, B, n).to(DEV)}
    model.train()
    out = model(to_dev(inp))
    return model, crit, tgt, out, data


@pytest.mark.parametrize("ep", [0, 20])
def test_model_losses_with_the_operator_on_and_off(cfg3, ep):
    model, crit, tgt, out, data = cfg3
    res = {}
    for on in (True, False):
        model.fused_attention_losses = on
        loss, bs = model.get_loss(crit, tgt, out, epoch=ep)
        (gw,) = torch.autograd.grad(loss["total"], out["weights"], retain_graph=True)
        res[on] = (loss, gw, bs)
    model.fused_attention_losses = True
    (lon, gon, bon), (loff, goff, boff) = res[True], res[False]
    assert list(lon.keys()) == list(loff.keys()) and bon == boff
    assert {"prior", "contrast", "entropy"} <= set(lon)
    for k in lon:
        a, b = torch.as_tensor(lon[k]), torch.as_tensor(loff[k])
        assert a.shape == b.shape and a.requires_grad == b.requires_grad and a.dtype == b.dtype, k
        want = float(data[f"ep{ep}_loss_{k}"])
        print("cfg3 ep", ep, k, float(a), float(b), want)
        assert abs(float(a) - float(b)) <= 1e-5 * max(1.0, abs(float(b))), k        # a few float32 ulps
        assert abs(float(a.detach()) - want) < 1e-3 * max(1.0, abs(want)), (ep, k)  # the golden test's tolerance
    assert gon.shape == goff.shape
    scale = max(1.0, float(goff.abs().max()))
    print("cfg3 ep", ep, "d total / d weights: max", float(goff.abs().max()), "diff", float((gon - goff).abs().max()))
    assert float((gon - goff).abs().max()) <= 1e-5 * scale
    if ep == 0:
        assert float(gon.abs().max()) == 0.0        # epoch + 1 < decay_step: the regularisers carry no gradient


def test_model_falls_back_for_a_criterion_the_operator_does_not_cover(cfg3):
    model, crit, tgt, out, data = cfg3
    wts = out["weights"].squeeze(1)
    assert model._fused_attention_losses(crit, tgt, wts, (0.25, 0.25, 0.25)) is not None
    for prior in (nn.KLDivLoss(reduction="batchmean", log_target=True), nn.KLDivLoss(reduction="none"),
                  nn.MSELoss(), nn.NLLLoss(), nn.SmoothL1Loss(beta=0.5)):
        c2 = dict(crit, prior=prior)
        assert model._fused_attention_losses(c2, tgt, wts, (0.25, 0.25, 0.25)) is None, prior
    from attention_based_tbn_amd.core.models.contrast_loss import ContrastLoss
    c2 = dict(crit, contrast=ContrastLoss(threshold=0.1, reduction="sum"))
    assert model._fused_attention_losses(c2, tgt, wts, (0.25, 0.25, 0.25)) is None
    assert model._fused_attention_losses(crit, dict(tgt, weights=tgt["weights"].cpu()), wts, (0.25, 0.25, 0.25)) is None
    assert model._fused_attention_losses(crit, tgt, wts.double(), (0.25, 0.25, 0.25)) is None
    model.fused_attention_losses = False
    assert model._fused_attention_losses(crit, tgt, wts, (0.25, 0.25, 0.25)) is None
    model.fused_attention_losses = True
