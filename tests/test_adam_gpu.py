"""`FusedAdam` / `tbn_opt_adam_step` on the GPU against `torch.optim.Adam` run on the CPU in float64 from the same fp32 values.

Error measure, per tensor: max|got - ref64| / max|ref64| for the parameter, `exp_avg` and `exp_avg_sq`.  Bound, per tensor:
4 x max(the same measure of torch's own float32 CPU run, 2^-23) -- the factor covers fused multiply-adds, the lerp form of
`exp_avg` and the host-rounded `step_size` / `inv_sqrt_bc2`, each at most one ulp per step.  A missing bias correction or
weight decay moves the parameters by about lr = 1e-3.

Worst measured on an MI355X (test 1, both weight decays): see profiles/adam_step.md."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("exp_avg", "exp_avg_sq")
FLOOR = 2.0 ** -23


def _cpu_run(p0, groups, grads, dtype, clip=None, lr=1e-3):
    """torch.optim.Adam on CPU copies in `dtype`.  `groups`: [(parameter indices, weight_decay)]; `grads[s][i]`: fp32 tensor or
    None.  -> per step [(parameter, exp_avg, exp_avg_sq) or None per tensor], the optimiser, the last total norm"""
    ps = [torch.nn.Parameter(p.to(dtype).clone(), requires_grad=True) for p in p0]
    opt = torch.optim.Adam([{"params": [ps[i] for i in idx], "weight_decay": wd} for idx, wd in groups], lr=lr)
    trace, norm = [], None
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(dtype).clone()
        if clip:
            norm = torch.nn.utils.clip_grad_norm_(ps, clip)
        opt.step()
        trace.append([(p.detach().clone(),) + tuple(opt.state[p][k].clone() for k in KEYS) if len(opt.state[p]) else
                      (p.detach().clone(), None, None) for p in ps])
    return trace, opt, ps, norm


def _rel(a, b):
    """max|a - b| / max|b| (b: the float64 reference); 0 when both are all zero"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d, s = float((a - b).abs().max()), float(b.abs().max())
    return d / s if s > 0 else (0.0 if d == 0 else float("inf"))


def _check(got, ref64, ref32, what, report):
    """got / ref64 / ref32: lists over tensors of (p, exp_avg, exp_avg_sq); asserts the module's bound per tensor"""
    for i, (g, r64, r32) in enumerate(zip(got, ref64, ref32)):
        for name, a, b, c in zip(("param",) + KEYS, g, r64, r32):
            assert (a is None) == (b is None), (what, i, name)
            if a is None:
                continue
            err, err32 = _rel(a, b), _rel(c, b)
            bound = 4 * max(err32, FLOOR)
            report.setdefault(name, []).append((err, err32, i))
            assert err <= bound, f"{what}: tensor {i} {name}: {err:.3e} > {bound:.3e} (fp32 CPU torch: {err32:.3e})"


def _print(report, what):
    for name, rows in report.items():
        err, err32, i = max(rows)
        print(f"{what}: worst {name} error {err:.3e} (tensor {i}; fp32 CPU torch there {err32:.3e}, "
              f"worst fp32 CPU torch {max(r[1] for r in rows):.3e})")


def _state(opt, params):
    return [(p,) + tuple(opt.state[p][k] for k in KEYS) if len(opt.state[p]) else (p, None, None) for p in params]


def _seeded(shapes, nsteps, seed, scale=lambda i: 10.0 ** ((i % 4) - 2)):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * scale(i) for i, s in enumerate(shapes)] for _ in range(nsteps)]
    return p0, grads


SHAPES = [(1,), (3,), (5, 7), (4, 32), (1000,), (16384,), (16385,), (64, 3, 3, 3), (33, 129)]


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_update_rule_against_fp64_torch(wd):
    """every launch path of the kernel: one element, the scalar tail, exactly one chunk, a chunk boundary, lengths that are no
    multiple of 4, a gradient at element offset 1 of a larger buffer (scalar path), a frozen parameter, a parameter without
    a gradient in two of the six steps (its `step` falls behind), and an all-zero gradient without decay (bit-unchanged)"""
    from attention_based_tbn_amd.core.utils import FusedAdam
    shapes = SHAPES + [(37,), (6,), (50,)]
    n = len(SHAPES)
    UNALIGNED, FROZEN, ZERO, SKIPPED = n, n + 1, n + 2, 3
    p0, grads = _seeded(shapes, 6, 11)
    for s, gs in enumerate(grads):
        gs[FROZEN] = None
        gs[ZERO] = torch.zeros(shapes[ZERO])
        if s in (1, 2):
            gs[SKIPPED] = None
    groups = [([i for i in range(len(shapes)) if i != ZERO], wd), ([ZERO], 0.0)]
    ref64, opt64, ps64, _ = _cpu_run(p0, groups, grads, torch.float64)
    ref32, _, _, _ = _cpu_run(p0, groups, grads, torch.float32)

    params = [torch.nn.Parameter(p.to(DEV), requires_grad=(i != FROZEN)) for i, p in enumerate(p0)]
    opt = FusedAdam([{"params": [params[i] for i in idx], "weight_decay": w} for idx, w in groups], lr=1e-3)
    holder = torch.zeros(64, device=DEV)
    report = {}
    for s, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if g is None else g.to(DEV)
        holder[1:38] = gs[UNALIGNED].to(DEV)
        params[UNALIGNED].grad = holder[1:38]
        assert params[UNALIGNED].grad.data_ptr() % 16 == 4 and params[UNALIGNED].grad.is_contiguous()
        opt.step()
        _check(_state(opt, params), ref64[s], ref32[s], f"wd {wd} step {s}", report)
    _print(report, f"update rule, weight_decay {wd}")
    assert torch.equal(params[ZERO].detach().cpu(), p0[ZERO])
    assert torch.equal(params[FROZEN].detach().cpu(), p0[FROZEN]) and len(opt.state[params[FROZEN]]) == 0
    for i, p in enumerate(params):
        if i != FROZEN:
            assert float(opt.state[p]["step"]) == (4 if i == SKIPPED else 6), i
            assert float(opt64.state[ps64[i]]["step"]) == float(opt.state[p]["step"])


def test_more_tensors_than_one_launch_table_holds():
    from attention_based_tbn_amd.core.utils import FusedAdam
    from attention_based_tbn_amd.core.utils.optim import MAX_TENSORS
    shapes = [(k,) for k in range(1, 102)]
    assert len(shapes) > 2 * MAX_TENSORS
    p0, grads = _seeded(shapes, 2, 12)
    groups = [(list(range(len(shapes))), 1e-4)]
    ref64, _, _, _ = _cpu_run(p0, groups, grads, torch.float64)
    ref32, _, _, _ = _cpu_run(p0, groups, grads, torch.float32)
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-4)
    report = {}
    for s, gs in enumerate(grads):
        for p, g in zip(params, gs):
            p.grad = g.to(DEV)
        opt.step()
        _check(_state(opt, params), ref64[s], ref32[s], f"101 tensors step {s}", report)
    _print(report, "101 tensors")


@pytest.mark.parametrize("gscale,clips", [(1.0, True), (1e-3, False)])
@pytest.mark.parametrize("consumed", [False, True])
def test_clip_in_memory_and_folded(gscale, clips, consumed):
    """`step(clip_grad=c)` leaves the gradients as `clip_grad_norm_` does; `step(clip_grad=c, grads_consumed=True)` leaves them
    bit-unchanged; both update like fp64 `clip_grad_norm_` + `optim.Adam`.  Rescaled gradients: the coefficient is as exact as
    the norm (2e-6 relative, the bound of the SGD test) and the product adds one rounding (2^-23)."""
    from attention_based_tbn_amd.core.utils import FusedAdam
    clip = 2.0
    shapes = [(5, 7), (16385,), (33, 129), (3,)]
    p0, grads = _seeded(shapes, 3, 13, scale=lambda i: gscale)
    groups = [(list(range(len(shapes))), 1e-4)]
    ref64, _, ps64, _ = _cpu_run(p0, groups, grads, torch.float64, clip=clip)
    ref32, _, _, _ = _cpu_run(p0, groups, grads, torch.float32, clip=clip)
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-4)
    report = {}
    for s, gs in enumerate(grads):
        for p, g in zip(params, gs):
            p.grad = g.to(DEV)
        norm64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
        assert (norm64 > clip) == clips
        opt.step(clip_grad=clip, grads_consumed=consumed)
        assert opt.last_total_norm.is_cuda and abs(float(opt.last_total_norm) - norm64) <= 2e-6 * norm64
        for p, g in zip(params, gs):
            if consumed or not clips:
                assert torch.equal(p.grad.cpu(), g)
            else:
                want = g.double() * (clip / (norm64 + 1e-6))
                np.testing.assert_allclose(p.grad.double().cpu().numpy(), want.numpy(), rtol=2e-6 + FLOOR, atol=0)
        _check(_state(opt, params), ref64[s], ref32[s], f"clip step {s}", report)
    _print(report, f"clip (coefficient {'< 1' if clips else '1'}, {'folded' if consumed else 'in memory'})")


@pytest.mark.parametrize("fused_first", [True, False])
def test_state_interchanges_with_torch_adam(fused_first):
    """three steps of one optimiser, `load_state_dict(other.state_dict())`, two more steps of both on the same gradients"""
    from attention_based_tbn_amd.core.utils import FusedAdam
    shapes = [(5, 7), (16385,), (33, 129), (3,)]
    p0, grads = _seeded(shapes, 5, 14)
    groups = [(list(range(len(shapes))), 1e-4)]
    ref64, _, _, _ = _cpu_run(p0, groups, grads, torch.float64)
    ref32, _, _, _ = _cpu_run(p0, groups, grads, torch.float32)

    def make(cls, values):
        ps = [torch.nn.Parameter(v.detach().clone().to(DEV)) for v in values]
        return ps, cls(ps, lr=1e-3, weight_decay=1e-4)

    def run(ps, opt, steps):
        for s in steps:
            for p, g in zip(ps, grads[s]):
                p.grad = g.to(DEV)
            opt.step()

    first, second = (FusedAdam, torch.optim.Adam) if fused_first else (torch.optim.Adam, FusedAdam)
    pa, oa = make(first, p0)
    run(pa, oa, range(3))
    pb, ob = make(second, pa)
    # (a copy, as a checkpoint file makes one: `load_state_dict` adopts the tensors it is given, and the two optimisers
    # would count their steps on one shared `step` tensor)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    fused = oa if fused_first else ob
    for p in fused.param_groups[0]["params"]:
        st = fused.state[p]["step"]
        assert st.device.type == "cpu" and st.dtype == torch.float32 and st.dim() == 0 and float(st) == 3
    run(pa, oa, range(3, 5))
    run(pb, ob, range(3, 5))
    for i, (a, b) in enumerate(zip(_state(oa, pa), _state(ob, pb))):
        for name, x, y, r64, r32 in zip(("param",) + KEYS, a, b, ref64[4][i], ref32[4][i]):
            bound = 4 * max(_rel(r32, r64), FLOOR)
            err = _rel(x, y)
            print(f"{first.__name__} -> {second.__name__}: tensor {i} {name} differs by {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (i, name, err, bound)
        assert float(oa.state[pa[i]]["step"]) == float(ob.state[pb[i]]["step"]) == 5
    # both also sit within the bound of the float64 run
    report = {}
    _check(_state(oa, pa), ref64[4], ref32[4], "continued run", report)
    _check(_state(ob, pb), ref64[4], ref32[4], "resumed run", report)


def test_autograd_bookkeeping_and_refusals():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.core.utils import FusedAdam
    p = torch.nn.Parameter(torch.ones(40, device=DEV))
    opt = FusedAdam([p], lr=1e-3)
    seen = []
    for s in range(3):
        p.grad = torch.full((40,), 0.5, device=DEV)
        opt.step()
        st = opt.state[p]
        seen.append((p._version, st["exp_avg"]._version, st["exp_avg_sq"]._version))
    assert all(b > a for x, y in zip(seen, seen[1:]) for a, b in zip(x, y)), seen

    def refused(bad, grad):
        good = torch.nn.Parameter(torch.ones(8, device=DEV))
        good.grad = torch.ones(8, device=DEV)
        bad.grad = grad
        o = FusedAdam([good, bad], lr=1e-3)
        with pytest.raises(TbnHipError):
            o.step()
        with pytest.raises(TbnHipError):
            o.step(clip_grad=1.0)
        assert torch.equal(good.detach().cpu(), torch.ones(8))
        assert all(float(s["step"]) == 0 for s in o.state.values() if "step" in s)     # refused before anything advanced

    refused(torch.nn.Parameter(torch.ones(8)), torch.ones(8))                                          # CPU among GPU
    refused(torch.nn.Parameter(torch.ones(8, device=DEV, dtype=torch.float16)), torch.ones(8, device=DEV, dtype=torch.float16))
    refused(torch.nn.Parameter(torch.ones(4, 6, device=DEV).t()), torch.ones(6, 4, device=DEV))      # non-contiguous


def _adam_replay(params, micro_grads, k, clip, lr, wd):
    """core/tools/train.py:66-94 with torch's own clip_grad_norm_ + optim.Adam on float64 CPU copies; `micro_grads[it][i]` is
    what iteration it's backward adds to parameter i's .grad (None: nothing).  -> per iteration the parameters"""
    ps = [torch.nn.Parameter(p.double().clone()) for p in params]
    opt = torch.optim.Adam(ps, lr, betas=(0.9, 0.999), weight_decay=wd)
    trace = []
    for it, gs in enumerate(micro_grads):
        if (it + 1) % k == 0:
            opt.zero_grad()
        for p, g in zip(ps, gs):
            if g is not None:
                p.grad = g.double().clone() if p.grad is None else p.grad + g.double()
        if clip:
            torch.nn.utils.clip_grad_norm_(ps, clip)
        if (it + 1) % k == k - 1:
            opt.step()
        trace.append([p.detach().clone() for p in ps])
    return trace


@pytest.mark.parametrize("k,clip", [(1, 2.0), (2, None)])
def test_train_step_with_fused_adam_on_the_real_model(k, clip):
    """`TrainStep` + `FusedAdam` on the small three-modality model, four iterations; every iteration's micro-gradients are
    captured on the GPU and the reference loop is replayed with float64 `optim.Adam` on the CPU.  Parameters after every
    iteration within 4e-6 (max|dp| / max|p| per tensor).  k = 1 with a clip runs the folded launch form.
    Measured on an MI355X: worst 1.3e-6 (k = 1) and 7.2e-7 (k = 2), both at fusion.fusion_layer.0.weight.  That is float32
    conditioning, not the kernel: in a few of its 1.6 M elements the clipped gradient and the decay term cancel to |d| < eps
    in the first step, where p moves by lr * d / (|d| + eps) and one ulp of wd * p (7e-13) becomes 6e-8 of p."""
    from tests.util import load_case
    from tests.test_model_gpu import build_product, to_dev
    from attention_based_tbn_amd.core.utils import FusedAdam, TrainStep
    cfg, modality, meta, data, inp, target = load_case("train_cfg4_all_noattn")
    model, crit = build_product(cfg, modality, meta)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    params = [p for _, p in named]
    p0 = [p.detach().cpu().clone() for p in params]
    lr, wd = 1e-3, 0.0005
    opt = FusedAdam(params, lr, betas=(0.9, 0.999), weight_decay=wd)
    step = TrainStep(model, opt, crit, accumulator_step=k, clip_grad=clip)
    micro = []
    hooks = [p.register_hook(lambda g, i=i: micro[-1].__setitem__(i, g.detach().clone())) for i, p in enumerate(params)]
    gen = torch.Generator().manual_seed(k)
    got = []
    for it in range(4):
        micro.append([None] * len(params))
        x = {m: v + 0.05 * torch.randn(v.shape, generator=gen) for m, v in inp.items()}
        step(it, to_dev(x), {"class": to_dev(target["class"])}, epoch=0)
        if k == 1:      # the folded form: the optimiser took the clip, the gradients are as the backward left them
            assert step.last_total_norm is opt.last_total_norm and opt.last_total_norm.is_cuda
            assert all(torch.equal(p.grad, g) for p, g in zip(params, micro[-1]) if g is not None)
        torch.cuda.synchronize()
        micro[-1] = [None if g_ is None else g_.cpu() for g_ in micro[-1]]
        got.append([p.detach().cpu().clone() for p in params])
    for h in hooks:
        h.remove()
    assert all(float(opt.state[p]["step"]) == (4 if k == 1 else 2) for p in params if len(opt.state[p]))
    want = _adam_replay(p0, micro, k, clip, lr, wd)
    worst = (0.0, "", 0)
    for it in range(4):
        for (n, _), a, b in zip(named, got[it], want[it]):
            e = _rel(a, b)
            worst = max(worst, (e, n, it))
            assert e <= 4e-6, (it, n, e)
    print("TrainStep + FusedAdam (k %d, clip %s): worst parameter error %.3e at %s, iteration %d" % ((k, clip) + worst))
    assert not all(torch.equal(a, b) for a, b in zip(got[-1], p0))
