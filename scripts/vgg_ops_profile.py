"""Cost of a VGG16 train step on the operator route, one process on one MI355X.

1. The three new kernels at R = 96 frames (device events around LAUNCHES back-to-back calls of the C entry): time and achieved
   GB/s of their algorithmic bytes next to a device-to-device copy of the same number of bytes (half read, half written) in the
   same round.  First convolution (RGB and Flow, 224 x 224): frames read once + the 64-channel NHWC map written once; its weight
   gradient: dy + frames read once.  MaxPool2d(2, 2) on the 224 x 224 x 64 map: map read, pooled map + uint8 argmax written;
   backward with the ReLU gate: pooled gradient + argmax + the map read, the gradient written.  Adaptive pool at 7 x 7 x 512 and
   14 x 14 x 512: map read, features written (and the reverse).
2. tbn_linear_fwd / _dgrad / _wgrad at (M, K, N) = (96, 25088, 4096), classifier.0, against torch's F.linear and its autograd in
   the same round: time, TFLOP/s, and GB/s of the 411 MB weight every one of them streams once.
3. One train step of VGG16, RGB, 96 x 224 x 224 (forward, backward of a sum loss, FusedSGD with momentum) against the same
   network on torch.nn (tests/vgg_twin.py, torch.optim.SGD) in the same process, arms alternated (host clock around STEPS steps
   ending in a device synchronise), and the per-kernel time shares of one operator-route step from the library's kernel
   timeline (begin / end events that ride on each dispatch).

One warm-up round, then the median of ROUNDS; (min .. max) beside it.

    python scripts/vgg_ops_profile.py [--out profiles/vgg_ops.md]      (rewrites the tables; the notes below the marker stay)
"""
import argparse
import csv
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, LAUNCHES, STEPS, ROUNDS = 96, 10, 3, 3
MARK = "<!-- notes -->"


def events_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def host_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def rounds(arms, timer, count):
    """{name: (median, min, max) over ROUNDS of timer(fn, count)}, arms alternated inside every round, one warm-up round"""
    seen = {k: [] for k in arms}
    for r in range(ROUNDS + 1):
        for k, fn in arms.items():
            t = timer(fn, count)
            if r > 0:
                seen[k].append(t)
        print("round", r, {k: round(v[-1], 4) for k, v in seen.items() if v}, flush=True)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in seen.items()}


def kernel_arms(dev):
    """-> [(title, {arm: fn}, {arm: bytes})]"""
    from attention_based_tbn_amd._lib import call, lib, ptr, stream_ptr
    st = stream_ptr()
    g = torch.Generator(device=dev).manual_seed(1)
    src = torch.empty(1 << 29, device=dev)            # 2 GiB each: the copy arm's buffers
    dst = torch.empty(1 << 29, device=dev)
    groups = []

    def copy_arm(nbytes):
        return lambda: dst[:nbytes // 8].copy_(src[:nbytes // 8])

    h = w = 224
    y = torch.empty(R, h, w, 64, device=dev)
    dy = torch.randn(R, h, w, 64, generator=g, device=dev)
    for cin, name in ((3, "RGB"), (10, "Flow")):
        x = torch.randn(R, cin, h, w, generator=g, device=dev)
        wt = torch.randn(64, 3, 3, cin, generator=g, device=dev)
        dw = torch.empty_like(wt)
        partial = torch.empty(lib().tbn_conv3_first_stat_rows(R, cin, h, w) * 128, device=dev)
        ws = torch.empty(lib().tbn_conv3_first_wgrad_workspace_floats(R, cin, h, w), device=dev)
        nb = 4 * (x.numel() + y.numel())
        groups.append(("first conv, %s (cin %d), 224 x 224" % (name, cin), {
            "forward (epilogue 0, bias-free, ReLU)": lambda x=x, wt=wt: call(
                "tbn_conv3_first_fwd", ptr(x), ptr(wt), 0, ptr(y), 64, R, h, w, x.shape[1], 64, 0, 2, 0, 0, 0, st),
            "forward (epilogue 1, statistics)": lambda x=x, wt=wt, partial=partial: call(
                "tbn_conv3_first_fwd", ptr(x), ptr(wt), 0, ptr(y), 64, R, h, w, x.shape[1], 64, 1, 0, 0, 0, ptr(partial), st),
            "weight gradient": lambda x=x, dw=dw, ws=ws: call(
                "tbn_conv3_first_wgrad", ptr(dy), 64, ptr(x), ptr(dw), R, h, w, x.shape[1], 64, ptr(ws), st),
            "copy of the same bytes": copy_arm(nb),
        }, {"forward (epilogue 0, bias-free, ReLU)": nb, "forward (epilogue 1, statistics)": nb, "weight gradient": nb,
            "copy of the same bytes": nb}))
    # MaxPool2d(2, 2) on the first stage's map
    z = torch.randn(R, h, w, 64, generator=g, device=dev).relu_()
    pooled = torch.empty(R, h // 2, w // 2, 64, device=dev)
    argmax = torch.empty(R, h // 2, w // 2, 64, device=dev, dtype=torch.uint8)
    dpool = torch.randn(R, h // 2, w // 2, 64, generator=g, device=dev)
    din = torch.empty_like(z)
    nf = 4 * (z.numel() + pooled.numel()) + argmax.numel()
    nbw = 4 * (dpool.numel() + din.numel()) + argmax.numel()
    groups.append(("MaxPool2d(2, 2), 224 x 224 x 64", {
        "forward (+ argmax)": lambda: call("tbn_maxpool2_fwd", ptr(z), 64, ptr(pooled), 64, ptr(argmax), R, h, w, 64, st),
        "copy of the forward's bytes": copy_arm(nf),
        "backward": lambda: call("tbn_maxpool2_bwd", ptr(dpool), 64, ptr(argmax), 0, 0, ptr(din), 64, R, h, w, 64, 0, st),
        "copy of the backward's bytes": copy_arm(nbw),
        "backward with the ReLU gate": lambda: call("tbn_maxpool2_bwd", ptr(dpool), 64, ptr(argmax), ptr(z), 64, ptr(din), 64,
                                                    R, h, w, 64, 0, st),
        "copy of the gated backward's bytes": copy_arm(nbw + 4 * z.numel()),
        "relu_mask_bwd alone (the pass the gate saves)": lambda: call("tbn_relu_mask_bwd", ptr(din), ptr(z), 0, ptr(y),
                                                                      din.numel(), st),
    }, {"forward (+ argmax)": nf, "copy of the forward's bytes": nf, "backward": nbw, "copy of the backward's bytes": nbw,
        "backward with the ReLU gate": nbw + 4 * z.numel(), "copy of the gated backward's bytes": nbw + 4 * z.numel(),
        "relu_mask_bwd alone (the pass the gate saves)": 12 * z.numel()}))
    for hh in (7, 14):
        m = torch.randn(R, hh, hh, 512, generator=g, device=dev)
        feat = torch.empty(R, 512 * 49, device=dev)
        dm = torch.empty_like(m)
        nb = 4 * (m.numel() + feat.numel())
        groups.append(("AdaptiveAvgPool2d((7, 7)) + flatten, %d x %d x 512" % (hh, hh), {
            "forward": lambda m=m, hh=hh: call("tbn_adaptive_avgpool7_fwd", ptr(m), 512, ptr(feat), R, hh, hh, 512, st),
            "backward": lambda dm=dm, hh=hh: call("tbn_adaptive_avgpool7_bwd", ptr(feat), ptr(dm), 512, R, hh, hh, 512, 0, st),
            "copy of the same bytes": copy_arm(nb),
        }, {"forward": nb, "backward": nb, "copy of the same bytes": nb}))
    return groups


def linear_arms(dev):
    from attention_based_tbn_amd._lib import call, lib, ptr, stream_ptr
    import torch.nn.functional as F
    st = stream_ptr()
    M, K, N = R, 25088, 4096
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(M, K, generator=g, device=dev)
    wt = torch.randn(N, K, generator=g, device=dev) * 0.01
    b = torch.zeros(N, device=dev)
    out, dout = torch.empty(M, N, device=dev), torch.randn(M, N, generator=g, device=dev)
    dx, dw, db = torch.empty(M, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
    ws_d = torch.empty(N * K, device=dev)
    ws_w = torch.empty(max(lib().tbn_linear_wgrad_workspace_floats(M, K, N), 1), device=dev)
    arms = {
        "tbn_linear_fwd": lambda: call("tbn_linear_fwd", ptr(x), K, ptr(wt), ptr(b), ptr(out), N, M, K, N, 1, st),
        "torch F.linear": lambda: F.linear(x, wt, b),
        "tbn_linear_dgrad": lambda: call("tbn_linear_dgrad", ptr(dout), N, ptr(wt), ptr(dx), K, M, K, N, 0, ptr(ws_d), st),
        "torch dout @ w": lambda: torch.matmul(dout, wt),
        "tbn_linear_wgrad (+ bias)": lambda: call("tbn_linear_wgrad", ptr(dout), N, ptr(x), K, ptr(dw), ptr(db), M, K, N,
                                                  ptr(ws_w), st),
        "torch dout.T @ x": lambda: torch.matmul(dout.t(), x),
    }
    return arms, 2.0 * M * K * N, 4.0 * N * K


def step_arms(dev):
    from attention_based_tbn_amd.core.models import VGG
    from attention_based_tbn_amd.core.utils.optim import FusedSGD
    from tests.vgg_twin import TwinVGG
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(R, 3, 224, 224, generator=g, device=dev)
    Rw = torch.randn(R, 4096, generator=g, device=dev) * 1e-3
    net = VGG("16", "RGB", 3).to(dev).train()
    twin = TwinVGG("16", 3)
    twin.load_state_dict(net.state_dict())
    twin.to(dev).train()
    opts = {"ops": FusedSGD(net.parameters(), lr=1e-4, momentum=0.9), "nn": torch.optim.SGD(twin.parameters(), lr=1e-4,
                                                                                             momentum=0.9)}

    def step(model, opt):
        def run():
            opt.zero_grad(set_to_none=True)
            (model(x) * Rw).sum().backward()
            opt.step()
        return run
    return {"VGG16 on the HIP operators + FusedSGD": step(net, opts["ops"]),
            "the same network on torch.nn + torch.optim.SGD": step(twin, opts["nn"])}


def timeline_shares(run):
    """{kernel name: (launches, total ms)} of ONE call of run() from the library's kernel timeline"""
    from attention_based_tbn_amd._lib import call
    torch.cuda.synchronize()
    call("tbn_timeline_enable", 1)
    run()
    torch.cuda.synchronize()
    seen = {}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "timeline.csv")
        call("tbn_timeline_dump", path.encode())
        call("tbn_timeline_enable", 0)
        with open(path) as f:
            for row in csv.DictReader(f):
                n, ms = seen.get(row["Kernel_Name"], (0, 0.0))
                seen[row["Kernel_Name"]] = (n + 1, ms + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    return seen


def write(path, lines, notes):
    """the tables so far (rewritten after every section, so a run cut short leaves what it measured), then the kept notes"""
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n\n" + MARK + (notes or "\n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgg_ops.md"))
    ap.add_argument("--skip-step", action="store_true", help="kernels and GEMMs only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vgg_ops_profile.py measures on the GPU"
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = ["# VGG on the operator route (scripts/vgg_ops_profile.py)", "",
             "One %s (%s, %d CUs; HIP %s, torch %s), one process, R = %d frames.  Medians of %d rounds after a warm-up round, "
             "arms alternated inside a round; (min .. max) beside them."
             % (torch.cuda.get_device_name(0), props.gcnArchName, props.multi_processor_count, torch.version.hip,
                torch.__version__, R, ROUNDS), "",
             "## The new kernels (device events around %d back-to-back launches)" % LAUNCHES, "",
             "| operand | arm | algorithmic MB | ms | GB/s |", "|---|---|---|---|---|"]
    notes = ""
    if os.path.exists(args.out):
        with open(args.out) as f:
            text = f.read()
        if MARK in text:
            notes = text.split(MARK, 1)[1]
    alone = {}
    for title, arms, nbytes in kernel_arms(dev):
        print(title, flush=True)
        res = rounds(arms, events_ms, LAUNCHES)
        for k, (med, lo, hi) in res.items():
            lines.append("| %s | %s | %.1f | %.4f (%.4f .. %.4f) | %.0f |" % (title, k, nbytes[k] / 1e6, med, lo, hi,
                                                                            nbytes[k] / med / 1e6))
            alone[(title, k)] = med
        del arms
        torch.cuda.empty_cache()
    arms, flops, wbytes = linear_arms(dev)
    print("linear", flush=True)
    res = rounds(arms, events_ms, LAUNCHES)
    lines += ["", "## The Linear entries at (M, K, N) = (%d, 25088, 4096), classifier.0" % R, "",
              "| arm | ms | TFLOP/s | GB/s of the 411 MB weight |", "|---|---|---|---|"]
    for k, (med, lo, hi) in res.items():
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.1f | %.0f |" % (k, med, lo, hi, flops / med / 1e9, wbytes / med / 1e6))
        alone[("linear", k)] = med
    del arms
    torch.cuda.empty_cache()
    write(args.out, lines, notes)
    if not args.skip_step:
        arms = step_arms(dev)
        print("train step", flush=True)
        res = rounds(arms, host_ms, STEPS)
        ours = res["VGG16 on the HIP operators + FusedSGD"][0]
        lines += ["", "## One train step of VGG16, RGB, %d x 224 x 224 (host clock around %d steps ending in a synchronise)"
                  % (R, STEPS), "", "| arm | ms per step | against torch.nn |", "|---|---|---|"]
        nn_ms = res["the same network on torch.nn + torch.optim.SGD"][0]
        for k, (med, lo, hi) in res.items():
            lines.append("| %s | %.1f (%.1f .. %.1f) | %.2f x |" % (k, med, lo, hi, med / nn_ms))
        shares = timeline_shares(arms["VGG16 on the HIP operators + FusedSGD"])
        total = sum(ms for _, ms in shares.values())
        lines += ["", "Kernels of the library in ONE operator-route step (kernel timeline; %.1f ms of kernel time in total, "
                  "%.1f ms per step on the host clock; torch's own kernels -- the weight permutes, `rand` -- are not in it):"
                  % (total, ours), "", "| kernel | launches | ms | share of the library's kernel time |", "|---|---|---|---|"]
        for k, (n, ms) in sorted(shares.items(), key=lambda kv: -kv[1][1])[:24]:
            lines.append("| `%s` | %d | %.3f | %.1f %% |" % (k.replace("|", "/"), n, ms, 100 * ms / total))
        first = "first conv, RGB (cin 3), 224 x 224"
        f_ms = alone[(first, "forward (epilogue 0, bias-free, ReLU)")] + alone[(first, "weight gradient")]
        l_ms = sum(alone[("linear", k)] for k in ("tbn_linear_fwd", "tbn_linear_dgrad", "tbn_linear_wgrad (+ bias)"))
        lines += ["", "Shares of the step, from the stand-alone times above: the first layer (forward + weight gradient) %.3f ms = "
                  "%.1f %%; classifier.0 (forward + data gradient + weight gradient) %.3f ms = %.1f %%."
                  % (f_ms, 100 * f_ms / ours, l_ms, 100 * l_ms / ours)]
    write(args.out, lines, notes)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
