"""Cost of the Adam step on the config-4 parameter set (RGB+Flow+Audio, ~32.6 M trainable parameters), one process.

Whole step, clip included (host clock around STEPS calls that end in a device synchronise, so a host-bound arm shows as such):
  fused_adam   FusedAdam.step(clip_grad=20, grads_consumed=True)
  torch_adam   torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (default: foreach)
  torch_fused  the same with fused=True
  fused_sgd    FusedSGD.step(clip_grad=20, grads_consumed=True), the yardstick
Kernels alone (device events around LAUNCHES back-to-back calls of the C entry on a prebuilt table): opt_adam against opt_sgd,
GB/s from the algorithmic bytes (28 B and 20 B per element).  The arms alternate within a round; one warm-up round, then the
median of three.  The model is built once; every arm owns clones of its parameters and random gradients (norm > 20, so the
clip bites).

    python scripts/adam_step.py [--out profiles/adam_step.md]      (rewrites the tables; the notes below them stay)
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIG4 = ["model.attention.enable=False", "data.audio.audio_length=1.279", "data.sampling=async"]   # bench.py CONFIGS[4]
CLIP, STEPS, LAUNCHES, ROUNDS = 20.0, 10, 20, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "adam_step.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "adam_step.py measures on the GPU"
    from attention_based_tbn_amd._lib import AdamTensor, OptTensor, call, ptr, stream_ptr
    from attention_based_tbn_amd.config import get_modality, load_config
    from attention_based_tbn_amd.core.models import build_model
    from attention_based_tbn_amd.core.utils import FusedAdam, FusedSGD
    from attention_based_tbn_amd.core.utils.optim import _chunks
    dev = torch.device("cuda:0")
    cfg = load_config(CONFIG4)
    torch.manual_seed(0)
    model, _, _ = build_model(cfg, get_modality(cfg), dev)
    shapes = [p.detach() for p in model.parameters() if p.requires_grad]
    nelem = sum(p.numel() for p in shapes)
    g = torch.Generator(device=dev).manual_seed(1)
    master = [torch.randn(p.shape, generator=g, device=dev) * 0.01 for p in shapes]
    norm = float(torch.sqrt(sum((m.double() ** 2).sum() for m in master)))
    assert norm > CLIP, norm

    def own():
        ps = [torch.nn.Parameter(p.clone()) for p in shapes]
        for p, m in zip(ps, master):
            p.grad = m.clone()
        return ps

    def restore(ps):
        for p, m in zip(ps, master):
            p.grad.copy_(m)

    def torch_arm(**kw):
        ps = own()
        opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.999), weight_decay=5e-4, **kw)

        def step():
            torch.nn.utils.clip_grad_norm_(ps, CLIP)
            opt.step()
        return ps, step

    def fused_arm(cls, **kw):
        ps = own()
        opt = cls(ps, lr=1e-3, weight_decay=5e-4, **kw)
        return ps, (lambda: opt.step(clip_grad=CLIP, grads_consumed=True)), opt

    arms = {}
    arms["fused_adam"] = fused_arm(FusedAdam, betas=(0.9, 0.999))
    arms["torch_adam"] = torch_arm()
    arms["torch_fused"] = torch_arm(fused=True)
    arms["fused_sgd"] = fused_arm(FusedSGD, momentum=0.9)

    def time_steps(ps, step):
        restore(ps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3

    whole = {k: [] for k in arms}
    for r in range(ROUNDS + 1):
        for k, arm in arms.items():
            t = time_steps(arm[0], arm[1])
            if r > 0:
                whole[k].append(t)

    # kernels alone, on the state the fused arms have by now
    ps_a, _, opt_a = arms["fused_adam"]
    ps_s, _, opt_s = arms["fused_sgd"]
    ents_a = [AdamTensor(ptr(p), ptr(p.grad), ptr(opt_a.state[p]["exp_avg"]), ptr(opt_a.state[p]["exp_avg_sq"]), p.numel(),
                         1e-3, 1.0) for p in ps_a]
    ents_s = [OptTensor(ptr(p), ptr(p.grad), ptr(opt_s.state[p]["momentum_buffer"]), p.numel()) for p in ps_s]
    tabs = {"opt_adam": (list(_chunks(ents_a, AdamTensor)),
                         lambda a, n: call("tbn_opt_adam_step", a, n, 0.9, 0.999, 1e-8, 5e-4, 0, stream_ptr()), 28),
            "opt_sgd": (list(_chunks(ents_s)),
                        lambda a, n: call("tbn_opt_sgd_step", a, n, 1e-3, 0.9, 5e-4, 0, stream_ptr()), 20)}

    def time_kernel(chunks, launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCHES):
            for a, n in chunks:
                launch(a, n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / LAUNCHES

    kern = {k: [] for k in tabs}
    for r in range(ROUNDS + 1):
        for k, (chunks, launch, _) in tabs.items():
            t = time_kernel(chunks, launch)
            if r > 0:
                kern[k].append(t)

    lines = ["## Adam step on the config-4 parameter set (scripts/adam_step.py)", "",
             f"{len(shapes)} tensors, {nelem / 1e6:.2f} M parameters ({nelem * 4 / 1e6:.1f} MB of gradients), gradient norm "
             f"{norm:.1f} against clip_grad {CLIP:g}; {torch.cuda.get_device_name(0)}, torch {torch.__version__}.",
             f"One process, arms alternated, one warm-up round, median of {ROUNDS} (all rounds listed).", "",
             f"Whole step with the clip (host clock around {STEPS} steps ending in a synchronise), ms per step:", "",
             "| arm | median | rounds |", "|---|---|---|"]
    for k, ts in whole.items():
        lines.append(f"| {k} | {statistics.median(ts):.3f} | {', '.join('%.3f' % t for t in ts)} |")
    lines += ["", f"Update kernel alone (device events around {LAUNCHES} back-to-back launches), algorithmic bytes:", "",
              "| kernel | B / element | median ms | GB/s | rounds ms |", "|---|---|---|---|---|"]
    gbs = {}
    for k, ts in kern.items():
        med = statistics.median(ts)
        gbs[k] = nelem * tabs[k][2] / med / 1e6
        lines.append(f"| {k} | {tabs[k][2]} | {med:.4f} | {gbs[k]:.0f} | {', '.join('%.4f' % t for t in ts)} |")
    lines += ["", f"opt_adam reaches {gbs['opt_adam'] / gbs['opt_sgd']:.3f} of opt_sgd's GB/s in this run.", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    notes = ""         # what the file says below the tables (from its first "### " heading on) is kept
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = f.read()
        notes = old[old.index("\n### "):] if "\n### " in old else ""
    with open(args.out, "w") as f:
        f.write(text + notes)


if __name__ == "__main__":
    main()
