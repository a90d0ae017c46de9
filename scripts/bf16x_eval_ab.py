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
With --all (conv_math_layers = "all", weights pre-split into bf16 planes; results go to profiles/bf16x_eval_all.md) instead:
per launch the merged 1x1 groups of inception_3a / 4d / 5a (the plan's fp32 choice vs the pointwise kernel on planes, bf16x6
and bf16x3) and the three 3x3 layers with the weights split while staging vs read from planes; then the two eval forwards
with the arms f32 | bf16x6 "3x3" | bf16x6 "all", and the run-to-run spread of each arm's alternations; last, the RGB
backbone's summed launch time per rerouted layer class (3x3 / 1x1 / rest) in the same three arms, from the launch profiler.
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


def alternate_spread(arms, reps, warm=10):
    """as alternate(), returning {name: (median, min, max)}"""
    for fn in arms.values():
        timed(fn, warm)
    ms = {k: [] for k in arms}
    for _ in range(ALTERNATIONS):
        for k, fn in arms.items():
            ms[k].append(timed(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def split_planes(w, cout, k, cin, np_, st):
    from attention_based_tbn_amd._lib import lib
    planes = torch.empty(lib().tbn_conv_weight_planes_bytes(cout, k, cin, np_), dtype=torch.uint8, device=DEV)
    call("tbn_conv_split_weights", ptr(w), cout, k, cin, np_, ptr(planes), st)
    return planes


def per_launch_all(lines):
    net = BNInception(1000, 3).to(DEV).eval()
    st = torch.cuda.current_stream().cuda_stream
    lines += ["| 1x1 group | R | M x Cin x Cout | fp32 choice | fp32 ms | bf16x6 planes ms | speed-up | exec bf16 TF/s (% of 2516.6) | bf16x3 planes ms | speed-up |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    rows3 = ["", "| 3x3 layer | R | tile | bf16x6 staging-split ms | bf16x6 planes ms | planes / staging | bf16x3 staging-split ms | bf16x3 planes ms | planes / staging |",
             "|---|---|---|---|---|---|---|---|---|"]
    for R in (96, 256):
        with torch.no_grad():
            net(torch.randn(R, 3, 224, 224, device=DEV))
        plan = net._plans[(R, 224, 224)]
        for blk, hw in (("inception_3a", 28), ("inception_4d", 14), ("inception_5a", 7)):
            parts = [blk + s for s in ("_1x1", "_3x3_reduce", "_double_3x3_reduce", "_pool_proj")]
            cin, cout = net._layers[parts[0]]["cin"], sum(net._layers[q]["cout"] for q in parts)
            info = (C.c_int * 16)()
            call("tbn_backbone_launch_info", plan.handle, parts[0].encode(), 0, info)
            variant, mt, nt, stages = info[0], info[1], info[2], info[3]
            x = torch.randn(R, hw, hw, cin, device=DEV)
            w = (torch.randn(cout, 1, 1, cin, device=DEV) / cin ** 0.5).contiguous()
            sc, sh = torch.rand(cout, device=DEV) + 0.5, torch.randn(cout, device=DEV)
            y = torch.empty(R, hw, hw, cout, device=DEV)
            pl = {6: split_planes(w, cout, 1, cin, 6, st), 3: split_planes(w, cout, 1, cin, 3, st)}

            def desc(flags, stg, wt):
                d = ConvDesc()
                d.inp, d.in_ld, d.weight, d.out, d.out_ld = ptr(x), cin, ptr(wt), ptr(y), cout
                d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = R, hw, hw, cin, cout, 1, 1, 0
                d.epilogue, d.flags, d.stages, d.scale, d.shift = 2, flags, stg, ptr(sc), ptr(sh)
                return d
            d32 = desc({0: 0, 1: 4, 2: 8, 3: 16}[variant], stages, w)
            d6, d3 = desc(32 | 128, 0, pl[6]), desc(64 | 128, 0, pl[3])
            arms = {"f32": lambda: call("tbn_conv_launch", C.byref(d32), mt, nt, 0, st),
                    "bf16x6": lambda: call("tbn_conv_launch", C.byref(d6), 0, 0, 0, st),
                    "bf16x3": lambda: call("tbn_conv_launch", C.byref(d3), 0, 0, 0, st)}
            ms = alternate(arms, BATCH)
            fl = 2.0 * R * hw * hw * cout * cin
            lines.append("| %s | %d | %d x %d x %d | variant %d <%d,%d> | %.4f | %.4f | %.2fx | %.1f (%.1f %%) | %.4f | %.2fx |" % (
                blk, R, R * hw * hw, cin, cout, variant, mt, nt, ms["f32"], ms["bf16x6"], ms["f32"] / ms["bf16x6"],
                6 * fl / ms["bf16x6"] / 1e9, 600 * fl / ms["bf16x6"] / 1e9 / BF16_PEAK, ms["bf16x3"], ms["f32"] / ms["bf16x3"]))
            print(lines[-1], flush=True)
        for name, hw in LAYERS:
            L = net._layers[name]
            cin, cout = L["cin"], L["cout"]
            info = (C.c_int * 16)()
            call("tbn_backbone_launch_info", plan.handle, name.encode(), 0, info)
            xt = (info[1], info[2]) if info[0] == 1 else (0, 0)
            x = torch.randn(R, hw, hw, cin, device=DEV)
            w = (torch.randn(cout, 3, 3, cin, device=DEV) / (9 * cin) ** 0.5).contiguous()
            sc, sh = torch.rand(cout, device=DEV) + 0.5, torch.randn(cout, device=DEV)
            y = torch.empty(R, hw, hw, cout, device=DEV)
            pl = {6: split_planes(w, cout, 3, cin, 6, st), 3: split_planes(w, cout, 3, cin, 3, st)}

            def desc3(flags, wt):
                d = ConvDesc()
                d.inp, d.in_ld, d.weight, d.out, d.out_ld = ptr(x), cin, ptr(wt), ptr(y), cout
                d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = R, hw, hw, cin, cout, 3, 1, 1
                d.epilogue, d.flags, d.scale, d.shift = 2, flags, ptr(sc), ptr(sh)
                return d
            ds = {"s6": desc3(32, w), "p6": desc3(32 | 128, pl[6]), "s3": desc3(64, w), "p3": desc3(64 | 128, pl[3])}
            ms = alternate({k: (lambda d=d: call("tbn_conv_launch", C.byref(d), xt[0], xt[1], 0, st)) for k, d in ds.items()}, BATCH)
            rows3.append("| %s | %d | %s | %.4f | %.4f | %.3f | %.4f | %.4f | %.3f |" % (
                name, R, "tuned <%d,%d>" % xt if info[0] == 1 else "heuristic", ms["s6"], ms["p6"], ms["p6"] / ms["s6"],
                ms["s3"], ms["p3"], ms["p3"] / ms["s3"]))
            print(rows3[-1], flush=True)
    lines += rows3


def eval_forward_all(lines):
    lines += ["", "| eval forward | f32 ms (min - max) | bf16x6 \"3x3\" ms (min - max) | bf16x6 \"all\" ms (min - max) | all vs f32 | all vs 3x3 |",
              "|---|---|---|---|---|---|"]
    ARMS = (("f32", "f32", "3x3"), ("3x3", "bf16x6", "3x3"), ("all", "bf16x6", "all"))

    def run(model, inp, mode, layers):
        model.conv_math, model.conv_math_layers = mode, layers
        with torch.no_grad():
            model(inp)

    def row(label, ms):
        f = lambda t: "%.2f (%.2f - %.2f)" % t
        lines.append("| %s | %s | %s | %s | %.3fx | %.3fx |" % (label, f(ms["f32"]), f(ms["3x3"]), f(ms["all"]),
                                                             ms["f32"][0] / ms["all"][0], ms["3x3"][0] / ms["all"][0]))
        print(lines[-1], flush=True)
    net = BNInception(1000, 3).to(DEV).eval()
    x = torch.randn(256, 3, 224, 224, device=DEV)
    row("RGB backbone, 256 frames 224 x 224",
        alternate_spread({a: (lambda m=m, l=l: run(net, x, m, l)) for a, m, l in ARMS}, 3, warm=3))
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
    row("config-5 model (%s), %d clips x %d segments" % ("+".join(modality), B, n),
        alternate_spread({a: (lambda m=m, l=l: run(model, inp, m, l)) for a, m, l in ARMS}, 2, warm=2))


def class_sums_all(lines):
    """RGB backbone, 256 frames: the summed per-launch event time (tbn_profile_enable(2), keyed per layer) of the two layer
    classes "all" reroutes, in each arm.  A layer's class is read off the kernel that ran it in the "all" arm."""
    from attention_based_tbn_amd._lib import lib
    L = lib()
    net = BNInception(1000, 3).to(DEV).eval()
    x = torch.randn(256, 3, 224, 224, device=DEV)
    ARMS = (("f32", "f32", "3x3"), ("3x3", "bf16x6", "3x3"), ("all", "bf16x6", "all"))

    def profiled(mode, layers):
        net.conv_math, net.conv_math_layers = mode, layers
        L.tbn_profile_reset()
        L.tbn_profile_enable(2)
        try:
            with torch.no_grad():
                net(x)
            torch.cuda.synchronize()
        finally:
            L.tbn_profile_enable(0)
        out, name = [], C.create_string_buffer(256)
        for i in range(L.tbn_profile_num_entries()):
            cnt, ms, fl = C.c_long(), C.c_double(), C.c_double()
            L.tbn_profile_entry(i, name, 256, C.byref(cnt), C.byref(ms), C.byref(fl))
            kernel, label = name.value.decode().split(" | ", 1)
            out.append((kernel, label[4:].split(" | ")[0] if label.startswith("fwd ") else label, cnt.value, ms.value))
        L.tbn_profile_reset()
        return out
    for _, m, l in ARMS:          # warm-up: plan tuning, planes
        profiled(m, l)
    cls = {}
    for kernel, layer, _, _ in profiled("bf16x6", "all"):
        cls[layer] = "1x1" if "_pw_kernel" in kernel else ("3x3" if "_planes_kernel" in kernel else "rest")
    sums = {a: {"3x3": [], "1x1": [], "rest": []} for a, _, _ in ARMS}
    launches = {}
    for _ in range(5):
        for a, m, l in ARMS:
            tot, n = {"3x3": 0.0, "1x1": 0.0, "rest": 0.0}, {"3x3": 0, "1x1": 0, "rest": 0}
            for _, layer, cnt, ms in profiled(m, l):
                k = cls.get(layer, "rest")
                tot[k] += ms
                n[k] += cnt
            for k in tot:
                sums[a][k].append(tot[k])
            launches[a] = n
    lines += ["", "| layer class (RGB backbone, 256 frames, summed launch time) | f32 ms (launches) | bf16x6 \"3x3\" ms (launches) | bf16x6 \"all\" ms (launches) | all vs f32 | all vs 3x3 |",
              "|---|---|---|---|---|---|"]
    for k, label in (("3x3", "3x3 / stride 1, map <= 64 wide"), ("1x1", "1x1 / stride 1 GEMMs"), ("rest", "other conv launches (stem, stride 2)")):
        med = {a: statistics.median(sums[a][k]) for a, _, _ in ARMS}
        lines.append("| %s | %.3f (%d) | %.3f (%d) | %.3f (%d) | %.3fx | %.3fx |" % (
            label, med["f32"], launches["f32"][k], med["3x3"], launches["3x3"][k], med["all"], launches["all"][k],
            med["f32"] / med["all"], med["3x3"] / med["all"]))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--all", action="store_true", help="the conv_math_layers = \"all\" tables (profiles/bf16x_eval_all.md)")
    a = ap.parse_args()
    lines = ["box: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), ""]
    if a.all:
        per_launch_all(lines)
        eval_forward_all(lines)
        class_sums_all(lines)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
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
