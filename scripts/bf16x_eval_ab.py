"""Same-process A/B of the split-bf16 convolution math (conv_math = "bf16x6" / "bf16x3") against the fp32 kernels.

  python scripts/bf16x_eval_ab.py [--out FILE]      (FILE: the tables below as markdown; they are pasted into the
                                                     "Per-launch timings" / "Eval forward A/B" sections of profiles/bf16x_eval.md)

Part 1, per launch: conv2_3x3, inception_3a_double_3x3_2, inception_4d_double_3x3_2 at R = 96 frames and at the config-5
eval chunk (256 frames), eval epilogue: the tuned plan's fp32 choice vs bf16x6 vs bf16x3 (the tile the engine would take:
the layer's tuned LDS-halo tile, else the size heuristic), alternated A B C A B C ... after a warm-up; median of the
alternations, each a batch of launches between two events.
Part 2, eval forward: one RGB backbone (256 frames) and the config-5 model (11 clips x 25 segments x 3 modalities = 275 frames per backbone:
one full eval chunk of 256 frames + 19),
f32 vs bf16x6 alternated the same way.
Both accountings: algorithmic FLOPs (2 M Cout 9 Cin) against the 157.3 TF/s fp32-MFMA peak, and executed bf16 MFMA FLOPs
(6x / 3x the algorithmic ones) against the 2516.6 TF/s bf16 peak.  Stops at the first failing step.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attention_based_tbn_amd._lib import ConvDesc, call, ptr  # noqa: E402
from attention_based_tbn_amd.core.models.bn_inception import BNInception  # noqa: E402

DEV = "cuda"
F32_PEAK, BF16_PEAK = 157.3, 2516.6      # TF/s
LAYERS = [("conv2_3x3", 56), ("inception_3a_double_3x3_2", 28), ("inception_4d_double_3x3_2", 14)]
ALTERNATIONS, BATCH = 6, 20


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(arms, reps, warm=10):
    """arms: {name: fn}; returns {name: median ms over ALTERNATIONS rounds of A B C ...}"""
    for fn in arms.values():
        timed(fn, warm)
    ms = {k: [] for k in arms}
    for _ in range(ALTERNATIONS):
        for k, fn in arms.items():
            ms[k].append(timed(fn, reps))
    return {k: statistics.median(v) for k, v in ms.items()}


def per_launch(lines):
    net = BNInception(1000, 3).to(DEV).eval()
    st = torch.cuda.current_stream().cuda_stream
    lines += ["| layer | R | fp32 choice | fp32 ms | TF/s (% of 157.3) | bf16x6 tile | bf16x6 ms | speed-up | alg TF/s | exec bf16 TF/s (% of 2516.6) | bf16x3 ms | speed-up |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    worst6 = None
    for R in (96, 256):
        with torch.no_grad():
            net(torch.randn(R, 3, 224, 224, device=DEV))         # tunes the eval plan of this frame count
        plan = net._plans[(R, 224, 224)]
        for name, hw in LAYERS:
            L = net._layers[name]
            cin, cout = L["cin"], L["cout"]
            info = (C.c_int * 16)()
            call("tbn_backbone_launch_info", plan.handle, name.encode(), 0, info)
            variant, mt, nt, stages = info[0], info[1], info[2], info[3]
            x = torch.randn(R, hw, hw, cin, device=DEV)
            w = (torch.randn(cout, 3, 3, cin, device=DEV) / (9 * cin) ** 0.5).contiguous()
            sc, sh = torch.rand(cout, device=DEV) + 0.5, torch.randn(cout, device=DEV)
            y = torch.empty(R, hw, hw, cout, device=DEV)

            def desc(flags, stg):
                d = ConvDesc()
                d.inp, d.in_ld, d.weight, d.out, d.out_ld = ptr(x), cin, ptr(w), ptr(y), cout
                d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = R, hw, hw, cin, cout, 3, 1, 1
                d.epilogue, d.flags, d.stages, d.scale, d.shift = 2, flags, stg, ptr(sc), ptr(sh)
                return d
            d32 = desc({0: 0, 1: 4, 2: 8, 3: 16}[variant], stages)
            d6, d3 = desc(32, 0), desc(64, 0)
            xt = (mt, nt) if variant == 1 else (0, 0)            # what tbn_backbone_forward passes
            arms = {"f32": lambda: call("tbn_conv_launch", C.byref(d32), mt, nt, 0, st),
                    "bf16x6": lambda: call("tbn_conv_launch", C.byref(d6), xt[0], xt[1], 0, st),
                    "bf16x3": lambda: call("tbn_conv_launch", C.byref(d3), xt[0], xt[1], 0, st)}
            ms = alternate(arms, BATCH)
            fl = 2.0 * R * hw * hw * cout * 9 * cin
            tf = lambda t: fl / t / 1e9
            s6, s3 = ms["f32"] / ms["bf16x6"], ms["f32"] / ms["bf16x3"]
            if R == 96:
                worst6 = s6 if worst6 is None else min(worst6, s6)
            lines.append("| %s | %d | variant %d <%d,%d> | %.4f | %.1f (%.1f %%) | %s | %.4f | %.2fx | %.1f | %.1f (%.1f %%) | %.4f | %.2fx |" % (
                name, R, variant, mt, nt, ms["f32"], tf(ms["f32"]), 100 * tf(ms["f32"]) / F32_PEAK,
                "tuned <%d,%d>" % xt if variant == 1 else "heuristic", ms["bf16x6"], s6, tf(ms["bf16x6"]),
                6 * tf(ms["bf16x6"]), 600 * tf(ms["bf16x6"]) / BF16_PEAK, ms["bf16x3"], s3))
            print(lines[-1], flush=True)
    return worst6


def eval_forward(lines):
    lines += ["", "| eval forward | f32 ms | bf16x6 ms | speed-up |", "|---|---|---|---|"]
    net = BNInception(1000, 3).to(DEV).eval()
    x = torch.randn(256, 3, 224, 224, device=DEV)

    def run(model, inp, mode):
        model.conv_math = mode
        with torch.no_grad():
            model(inp)
    ms = alternate({m: (lambda m=m: run(net, x, m)) for m in ("f32", "bf16x6")}, 3, warm=3)
    lines.append("| RGB backbone, 256 frames 224 x 224 | %.2f | %.2f | %.3fx |" % (ms["f32"], ms["bf16x6"], ms["f32"] / ms["bf16x6"]))
    print(lines[-1], flush=True)
    del net, x
    from attention_based_tbn_amd.config import load_config, get_modality
    from attention_based_tbn_amd.core.models import build_model
    cfg = load_config(["data.audio.audio_length=1.279"])
    modality = get_modality(cfg)
    model, _, _ = build_model(cfg, modality, torch.device(DEV))
    model.eval()
    B, n = 11, cfg.test.num_segments
    inp = {"RGB": torch.rand(B, n, 3, 224, 224, device=DEV) - 0.45, "Flow": torch.rand(B, n, 10, 224, 224, device=DEV) - 0.5,
           "Audio": torch.randn(B, n, 1, 256, 256, device=DEV) * 3 - 6}
    ms = alternate({m: (lambda m=m: run(model, inp, m)) for m in ("f32", "bf16x6")}, 2, warm=2)
    lines.append("| config-5 model (%s), %d clips x %d segments | %.2f | %.2f | %.3fx |" % (
        "+".join(modality), B, n, ms["f32"], ms["bf16x6"], ms["f32"] / ms["bf16x6"]))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["box: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), ""]
    worst6 = per_launch(lines)
    eval_forward(lines)
    lines += ["", "criterion (bf16x6 >= 1.5x per launch at R = 96 on every measured layer): %s (smallest speed-up %.2fx)" % (
        "MET" if worst6 >= 1.5 else "NOT MET", worst6)]
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
