"""`FusedAdam` on the host: construction through `build_optimizer`, the all-CPU step (torch's own Adam), and the checkpoint
path -- an Adam run saved with `save_checkpoint` carries both moments and `step` over the reference's per-layer layout
and resumes bit for bit; SGD checkpoints come out as before."""
import copy

import pytest
import torch

RGB_ONLY = ["data.flow.enable=False", "data.audio.enable=False", "model.attention.enable=False"]


def test_build_optimizer_adam_is_fused_adam():
    from attention_based_tbn_amd import _lib
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.utils import FusedAdam, build_optimizer
    net = torch.nn.Linear(4, 2)
    cfg = load_config(["train.optim.type=adam", "train.optim.lr=0.001", "train.optim.weight_decay=0.0001"])
    opt, sched, warm = build_optimizer(cfg, net)
    assert isinstance(opt, FusedAdam) and isinstance(opt, torch.optim.Adam)
    g = opt.param_groups[0]
    assert g["betas"] == (0.9, 0.999) and g["lr"] == 0.001 and g["weight_decay"] == 0.0001 and g["eps"] == 1e-8
    assert sched is None and warm is None
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(net.parameters(), amsgrad=True)
    with pytest.raises(ValueError, match="lr"):
        FusedAdam(net.parameters(), lr=torch.tensor(1e-3))
    assert "tbn_opt_adam_step" in _lib.SIGNATURES     # tests/test_host_cpu.py then checks the header and the export


@pytest.mark.parametrize("clip", [None, 0.5])
def test_all_cpu_parameters_take_torchs_own_step(clip):
    from attention_based_tbn_amd.core.utils import FusedAdam
    g = torch.Generator().manual_seed(5)
    shapes = [(3,), (5, 7), (16,), (2, 3, 3)]
    p0 = [torch.randn(s, generator=g) for s in shapes]
    mine = [torch.nn.Parameter(p.clone()) for p in p0]
    ref = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = FusedAdam(mine, lr=1e-2, weight_decay=1e-4)
    want = torch.optim.Adam(ref, lr=1e-2, weight_decay=1e-4)
    for s in range(5):
        grads = [torch.randn(sh, generator=g) for sh in shapes]
        for i, (a, b) in enumerate(zip(mine, ref)):
            skip = i == 2 and s in (1, 2)            # this parameter has no gradient in two of the five iterations
            a.grad = None if skip else grads[i].clone()
            b.grad = None if skip else grads[i].clone()
        if clip:
            norm = torch.nn.utils.clip_grad_norm_(ref, clip)
            assert float(norm) > clip
            opt.step(clip_grad=clip)
            assert torch.equal(opt.last_total_norm, norm)
        else:
            opt.step()
        want.step()
        for a, b in zip(mine, ref):
            assert torch.equal(a, b), s
    for i, (a, b) in enumerate(zip(mine, ref)):
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(opt.state[a][k], want.state[b][k]), (i, k)
        assert float(opt.state[a]["step"]) == (3 if i == 2 else 5)


def _rgb_model(seed):
    from attention_based_tbn_amd.config import get_modality, load_config
    from attention_based_tbn_amd.core.models import build_model
    cfg = load_config(RGB_ONLY)
    torch.manual_seed(seed)
    model, _, _ = build_model(cfg, get_modality(cfg), torch.device("cpu"))
    return model


def _hand_grads(model, seed):
    g = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g) * 0.01 if p.requires_grad else None


@pytest.fixture(scope="module")
def adam_checkpoint(tmp_path_factory):
    """the RGB-only model on the CPU after two FusedAdam steps on hand-set gradients, and its checkpoint file"""
    from attention_based_tbn_amd.core.utils import FusedAdam, save_checkpoint
    model = _rgb_model(0)
    opt = FusedAdam(model.parameters(), lr=1e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-4)
    for s in range(2):
        _hand_grads(model, 10 + s)
        opt.step()
    fn = str(tmp_path_factory.mktemp("adam") / "ck.pth")
    save_checkpoint(model, opt, 3, [1.0], [2.0], [3.0], None, 1, filename=fn)
    return model, opt, fn


def test_adam_checkpoint_resumes_with_moments_and_step(adam_checkpoint):
    """the resume bug: the optimiser state of an Adam run used to be written empty and loaded as zero moments, step 0"""
    from attention_based_tbn_amd.core.utils import FusedAdam, load_checkpoint
    from attention_based_tbn_amd.core.utils.misc import reference_parameter_names
    model, opt, fn = adam_checkpoint
    data = torch.load(fn, map_location="cpu")
    names = reference_parameter_names(model)
    assert list(data.keys()) == ["epoch", "train_loss", "validation_loss", "validation_accuracy", "optimizer", "model"]
    assert data["optimizer"]["param_groups"][0]["params"] == list(range(len(names)))
    st0 = data["optimizer"]["state"][0]
    assert st0["exp_avg"].shape == (64, 3, 7, 7)
    assert st0["exp_avg_sq"].shape == (64, 3, 7, 7)
    assert float(st0["step"]) == 2
    # the reference's own load: optim.Adam over its per-layer parameters
    ref_params = [torch.nn.Parameter(torch.zeros_like(data["model"][n])) for n in names]
    ref_opt = torch.optim.Adam(ref_params, lr=0.1)
    ref_opt.load_state_dict(data["optimizer"])
    assert torch.equal(ref_opt.state[ref_params[0]]["exp_avg"], st0["exp_avg"])
    assert ref_opt.param_groups[0]["betas"] == (0.8, 0.99)
    # resume here
    model2 = _rgb_model(1)
    opt2 = FusedAdam(model2.parameters(), lr=0.5)
    load_checkpoint(fn, model2, opt2)
    nstate = 0
    for (n1, p1), (n2, p2) in zip(model.named_parameters(), model2.named_parameters()):
        assert n1 == n2 and torch.equal(p1, p2), n1
        s1, s2 = opt.state.get(p1, {}), opt2.state.get(p2, {})
        assert set(s1) == set(s2), n1
        for k in s1:
            assert torch.equal(s1[k], s2[k]), (n1, k)
            assert s2[k].dtype == torch.float32 and s2[k].device.type == "cpu"
        nstate += len(s1) > 0
    assert nstate >= 4
    g2 = opt2.param_groups[0]
    assert (g2["lr"], tuple(g2["betas"]), g2["eps"], g2["weight_decay"]) == (1e-3, (0.8, 0.99), 1e-7, 1e-4)
    # and the run continues as if it had never stopped (on copies: the fixture stays as it is)
    model1 = copy.deepcopy(model)
    opt1 = FusedAdam(model1.parameters(), lr=0.5)
    opt1.load_state_dict(opt.state_dict())
    for m_, o_ in ((model1, opt1), (model2, opt2)):
        _hand_grads(m_, 12)
        o_.step()
    for (n1, p1), (_, p2) in zip(model1.named_parameters(), model2.named_parameters()):
        assert torch.equal(p1, p2), n1
    assert not torch.equal(model1.Base_RGB.flat_weight, model.Base_RGB.flat_weight)


def test_mismatched_step_inside_a_flat_tensor_is_refused(adam_checkpoint):
    from attention_based_tbn_amd.core.utils import FusedAdam
    from attention_based_tbn_amd.core.utils.misc import optimizer_state_from_reference, reference_parameter_names
    model, _, fn = adam_checkpoint
    saved = torch.load(fn, map_location="cpu")["optimizer"]
    names = reference_parameter_names(model)
    slot = names.index("Base_RGB.conv2_3x3.weight")      # lands in Base_RGB.flat_weight behind conv1's slot
    saved["state"][slot]["step"] = torch.tensor(7.0)
    model2 = _rgb_model(1)
    with pytest.raises(ValueError, match="Base_RGB") as e:
        optimizer_state_from_reference(model2, FusedAdam(model2.parameters()), saved)
    assert "2" in str(e.value) and "7" in str(e.value)


def _sgd_state_to_reference_before(model, optimizer):
    """`optimizer_state_to_reference` as it was before it learnt Adam's state (this project's own code, kept as the
    yardstick for the SGD file layout)"""
    from attention_based_tbn_amd.core.utils.misc import FLAT_NAMES, _backbones, reference_parameter_names
    names = reference_parameter_names(model)
    own = dict(model.named_parameters())
    per_name = {}
    for pre, m in _backbones(model):
        flat = {}
        for a in FLAT_NAMES:
            st = optimizer.state.get(getattr(m, a), {})
            flat[a] = st.get("momentum_buffer")
        if all(v is None for v in flat.values()):
            continue
        have = {a for a, v in flat.items() if v is not None}
        flat = {a: (v if v is not None else torch.zeros_like(getattr(m, a))) for a, v in flat.items()}
        owner = {flat[a].untyped_storage().data_ptr(): a for a in FLAT_NAMES}
        for key, view in m.reference_param_views(flat):
            if owner[view.untyped_storage().data_ptr()] in have:
                per_name[pre + "." + key] = view.detach().clone(memory_format=torch.contiguous_format)
    state = {}
    for i, n in enumerate(names):
        if n in per_name:
            state[i] = {"momentum_buffer": per_name[n]}
        elif n in own and optimizer.state.get(own[n], {}).get("momentum_buffer") is not None:
            state[i] = {"momentum_buffer": optimizer.state[own[n]]["momentum_buffer"].detach().clone()}
    g0 = {k: v for k, v in optimizer.param_groups[0].items() if k != "params"}
    g0["params"] = list(range(len(names)))
    return {"state": state, "param_groups": [g0]}


def test_sgd_checkpoint_state_is_unchanged():
    from attention_based_tbn_amd.core.utils import FusedSGD
    from attention_based_tbn_amd.core.utils.misc import optimizer_state_to_reference
    model = _rgb_model(0)
    opt = FusedSGD(model.parameters(), 0.01, momentum=0.9, weight_decay=0.0005)
    g = torch.Generator().manual_seed(2)
    for n, p in model.named_parameters():     # hand-set buffers; the frozen flat tensors and one plain parameter keep none
        if p.requires_grad and n != "classifier.noun.bias":
            opt.state[p]["momentum_buffer"] = torch.randn(p.shape, generator=g)
    got, want = optimizer_state_to_reference(model, opt), _sgd_state_to_reference_before(model, opt)
    assert len(want["state"]) > 100 and len(want["state"]) < len(want["param_groups"][0]["params"])
    assert list(got.keys()) == list(want.keys())
    assert got["param_groups"] == want["param_groups"]
    assert list(got["param_groups"][0].keys()) == list(want["param_groups"][0].keys())
    assert list(got["state"].keys()) == list(want["state"].keys())
    for i, w in want["state"].items():
        s = got["state"][i]
        assert list(s.keys()) == ["momentum_buffer"]
        assert s["momentum_buffer"].dtype == w["momentum_buffer"].dtype and s["momentum_buffer"].shape == w["momentum_buffer"].shape
        assert s["momentum_buffer"].stride() == w["momentum_buffer"].stride()
        assert torch.equal(s["momentum_buffer"], w["momentum_buffer"])
