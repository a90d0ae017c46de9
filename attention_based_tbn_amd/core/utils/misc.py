"""Checkpoint and score-file formats of the reference (`core/utils/misc.py:56-165`), unchanged on the wire:
`torch.save` of {epoch, train_loss, validation_loss, validation_accuracy, optimizer, model[, conf_mat, scheduler]}
with the reference's `state_dict` key names (the flat GPU parameter storage is unpacked by the model), and the
EPIC-Kitchens `action_recognition` JSON of `save_scores`."""
import json
import os

import numpy as np
import torch

from ...config import get_modality  # noqa: F401  (reference exports it from misc as well)


def get_time_diff(start_time, end_time):
    hours = int((end_time - start_time) / 3600)
    minutes = int((end_time - start_time) / 60) - (hours * 60)
    seconds = int(np.floor((end_time - start_time) % 60))
    return (hours, minutes, seconds)


def save_checkpoint(model, optimizer, epoch, train_loss_hist, val_loss_hist, val_acc_hist, confusion_matrix,
                    num_gpus, scheduler=None, filename="checkpoint.pth"):
    target = getattr(model, "module", model) if num_gpus > 1 else model
    # the optimiser state is written over the reference's per-layer parameter list, so the file loads in the
    # reference (`optimizer.load_state_dict`) as well as here
    data = {"epoch": epoch, "train_loss": train_loss_hist, "validation_loss": val_loss_hist,
            "validation_accuracy": val_acc_hist, "optimizer": optimizer_state_to_reference(target, optimizer)}
    data["model"] = target.state_dict()
    if confusion_matrix:
        data["conf_mat"] = confusion_matrix
    if scheduler:
        data["scheduler"] = scheduler.state_dict()
    torch.save(data, filename)


def load_checkpoint(filename, model, optimizer=None, scheduler=None, num_gpus=1, map_location="cpu"):
    """Inverse of `save_checkpoint` (the reference inlines this in train.py:219-240 / test.py:60-66).  Accepts
    checkpoints written by the reference: their per-layer momentum buffers (SGD) or moments and `step` (Adam) are scattered
    into the flat ones."""
    data = torch.load(filename, map_location=map_location)
    target = model.module if (num_gpus > 1 and hasattr(model, "module")) else model
    target.load_state_dict(data["model"])
    if optimizer is not None and "optimizer" in data:
        n_saved = sum(len(g["params"]) for g in data["optimizer"]["param_groups"])
        n_here = sum(len(g["params"]) for g in optimizer.param_groups)
        if n_saved == n_here:
            optimizer.load_state_dict(data["optimizer"])
        else:   # written by the reference: one slot per per-layer parameter
            optimizer_state_from_reference(target, optimizer, data["optimizer"])
    if scheduler is not None and "scheduler" in data:
        scheduler.load_state_dict(data["scheduler"])
    return data


FLAT_NAMES = ("flat_weight", "flat_bias", "bn_weight_first", "bn_weight_rest", "bn_bias_first", "bn_bias_rest")


def _backbones(model):
    from ..models.bn_inception import BNInception
    return [(n, m) for n, m in model.named_modules() if isinstance(m, BNInception)]


def reference_parameter_names(model):
    """Names of `model.parameters()` of the REFERENCE model, in its order (= the index space of a reference
    checkpoint's optimizer state): the state_dict keys minus the buffers."""
    own = dict(model.named_parameters())
    bb = _backbones(model)
    names = []
    for key in model.state_dict().keys():
        pre = next((n for n, _ in bb if key.startswith(n + ".") and not key.startswith(n + ".last_linear.")), None)
        if pre is not None:
            if key.endswith((".running_mean", ".running_var", ".num_batches_tracked")):
                continue
            names.append(key)
        elif key in own:
            names.append(key)
    return names


# the per-parameter tensor states that travel through the flat <-> per-layer views: FusedSGD / optim.SGD keep
# `momentum_buffer`, FusedAdam / optim.Adam `exp_avg` and `exp_avg_sq` (plus the scalar `step`, carried separately)
STATE_TENSORS = ("momentum_buffer", "exp_avg", "exp_avg_sq")


def optimizer_state_from_reference(model, optimizer, ref_state):
    """Load a reference checkpoint's optimiser state (SGD: one momentum buffer per per-layer parameter; Adam: both moments
    and `step`) into an optimiser built over THIS model's parameters (flat backbone storage): the tensors are scattered
    into flat ones.  Adam's `step` is one number per flat tensor, so the per-layer slots that land in one flat tensor must
    agree on it; a checkpoint in which they do not cannot be represented here and raises ValueError."""
    names = reference_parameter_names(model)
    ref_idx = [i for g in ref_state["param_groups"] for i in g["params"]]
    assert len(ref_idx) == len(names), f"reference optimizer has {len(ref_idx)} parameters, the model {len(names)}"
    by_name = {n: ref_state["state"].get(i, {}) for n, i in zip(names, ref_idx)}
    own = {p: n for n, p in model.named_parameters()}
    bb = dict(_backbones(model))
    done = {}
    for pre, m in bb.items():
        for a in FLAT_NAMES:
            done[getattr(m, a)] = {}
        for k in STATE_TENSORS:
            flat = {a: torch.zeros_like(getattr(m, a)) for a in FLAT_NAMES}
            owner = {flat[a].untyped_storage().data_ptr(): a for a in FLAT_NAMES}
            filled = set()
            for key, view in m.reference_param_views(flat):
                buf = by_name.get(pre + "." + key, {}).get(k)
                if buf is not None:
                    view.copy_(buf.to(view.device))
                    filled.add(owner[view.untyped_storage().data_ptr()])
            for a in filled:   # a flat tensor none of whose layers had a buffer (frozen BN affine) keeps none
                done[getattr(m, a)][k] = flat[a]
        for key, view in m.reference_param_views(flat):   # (`flat` only says which flat tensor a layer lands in)
            step = by_name.get(pre + "." + key, {}).get("step")
            if step is None:
                continue
            st = done[getattr(m, owner[view.untyped_storage().data_ptr()])]
            if "step" in st and float(st["step"]) != float(step):
                raise ValueError(f"optimizer state of {pre}: the layers stored in one flat tensor disagree on `step` "
                                 f"({float(st['step']):g} and {float(step):g} at {key}); no such state exists here")
            st["step"] = step
    for group in optimizer.param_groups:
        for p in group["params"]:
            st = done[p] if p in done else by_name.get(own.get(p), {})
            for k in STATE_TENSORS:
                if st.get(k) is not None:
                    optimizer.state[p][k] = st[k].to(p.device).clone()
            if st.get("step") is not None:   # torch keeps it as a 0-dim float32 tensor on the host
                optimizer.state[p]["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
    for k in ("lr", "momentum", "weight_decay", "betas", "eps"):
        if k in ref_state["param_groups"][0]:
            for g in optimizer.param_groups:
                g[k] = ref_state["param_groups"][0][k]


def optimizer_state_to_reference(model, optimizer):
    """`optimizer.state_dict()` re-expressed over the reference's per-layer parameter list (what the reference's
    `optim.SGD.load_state_dict` / `optim.Adam.load_state_dict` expects).  Every per-layer slot of a flat tensor gets that
    tensor's `step`."""
    names = reference_parameter_names(model)
    own = dict(model.named_parameters())
    per_name = {}
    for pre, m in _backbones(model):
        states = {a: optimizer.state.get(getattr(m, a), {}) for a in FLAT_NAMES}
        for k in STATE_TENSORS:
            flat = {a: states[a].get(k) for a in FLAT_NAMES}
            if all(v is None for v in flat.values()):
                continue
            have = {a for a, v in flat.items() if v is not None}
            flat = {a: (v if v is not None else torch.zeros_like(getattr(m, a))) for a, v in flat.items()}
            owner = {flat[a].untyped_storage().data_ptr(): a for a in FLAT_NAMES}
            for key, view in m.reference_param_views(flat):
                a = owner[view.untyped_storage().data_ptr()]
                if a in have:   # frozen tensors have no buffer, as in torch
                    slot = per_name.setdefault(pre + "." + key, {})
                    if "step" in states[a] and "step" not in slot:
                        slot["step"] = states[a]["step"].detach().clone()
                    slot[k] = view.detach().clone(memory_format=torch.contiguous_format)
    state = {}
    for i, n in enumerate(names):
        if n in per_name:
            state[i] = per_name[n]
        elif n in own:
            st = optimizer.state.get(own[n], {})
            slot = {k: st[k].detach().clone() for k in ("step",) + STATE_TENSORS if torch.is_tensor(st.get(k))}
            if slot:
                state[i] = slot
    g0 = {k: v for k, v in optimizer.param_groups[0].items() if k != "params"}
    g0["params"] = list(range(len(names)))
    return {"state": state, "param_groups": [g0]}


def save_scores(scores, file_name, action_names):
    """reference misc.py:115-165, same JSON document"""
    out_result = {"version": "0.1", "challenge": "action_recognition"}
    for key in scores.keys():
        scores[key] = torch.cat(scores[key], dim=0)
    results = {}
    ids = scores["action_id"].cpu()
    host = {k: v.detach().float().cpu() for k, v in scores.items() if k != "action_id"}
    for idx in range(ids.shape[0]):
        a_id = str(ids[idx].item())
        results[a_id] = {}
        for key, val in host.items():
            if key == "action":
                top, ind = val[idx].topk(100, dim=0, largest=True, sorted=True)   # only the top 100 action scores
                results[a_id][key] = {action_names[i.item()]: s.item() for i, s in zip(ind, top)}
            else:
                results[a_id][key] = {str(i): s.item() for i, s in enumerate(val[idx])}
    out_result["results"] = results
    os.makedirs(os.path.split(file_name)[0], exist_ok=True)
    with open(file_name, "w") as f:
        json.dump(out_result, f, indent=4)
