"""Cost of BNInception_Audio on the operator route, one process on one MI355X.

The two stem kernels at R = 96 frames of 256 x 256 and 256 x 420 (device events around LAUNCHES back-to-back calls of the
C entry): time and achieved GB/s of their algorithmic bytes -- forward: the spectrogram read once plus the 64-channel NHWC
output written once; weight gradient: dy read once plus the spectrogram read once -- next to a device-to-device copy that
moves the same number of bytes (half of them read, half written) in the same run.  The copy is the yardstick.

Forward + backward of BNInception_Audio(1000) at R = 96, 256 x 256, training mode, loss = sum(out * R), against the engine's
BNInception(1000, 1) at the same shape (host clock around STEPS steps that end in a device synchronise).  The engine is the
yardstick; it tunes its plan in the warm-up round.

The arms alternate within a round; one warm-up round, then the median of three.

    python scripts/bna_step.py [--out profiles/bna_ops.md]      (rewrites the tables; the notes below the marker stay)
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R, LAUNCHES, STEPS, ROUNDS = 96, 10, 5, 3
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
    """{name: median over ROUNDS of timer(fn, count)} with the arms alternated inside every round, after one warm-up round"""
    seen = {k: [] for k in arms}
    for r in range(ROUNDS + 1):
        for k, fn in arms.items():
            t = timer(fn, count)
            if r > 0:
                seen[k].append(t)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in seen.items()}


def stem_arms(h, w, dev):
    from attention_based_tbn_amd._lib import call, lib, ptr, stream_ptr
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator(device=dev).manual_seed(h + w)
    x = torch.randn(R, 1, h, w, generator=g, device=dev)
    wt = torch.randn(64, 3, generator=g, device=dev)
    y = torch.empty(R, oh, ow, 64, device=dev)
    dy = torch.randn(R, oh, ow, 64, generator=g, device=dev)
    partial = torch.empty(lib().tbn_audio_stem_stat_rows(R, h, w) * 128, device=dev)
    ws = torch.empty(lib().tbn_audio_stem_wgrad_workspace_floats(R, h, w), device=dev)
    dw = torch.empty(64, 3, device=dev)
    fwd_bytes = 4 * (x.numel() + y.numel())
    wg_bytes = 4 * (x.numel() + dy.numel())
    src = torch.randn(max(fwd_bytes, wg_bytes) // 8, generator=g, device=dev)
    dst = torch.empty_like(src)
    st = stream_ptr()
    arms = {
        "stem forward (epilogue 1)": lambda: call("tbn_audio_stem_fwd", ptr(x), ptr(wt), 0, ptr(y), 64, R, h, w, 1, 0, 0, 0,
                                                   ptr(partial), st),
        "copy, forward's bytes": lambda: dst[:fwd_bytes // 8].copy_(src[:fwd_bytes // 8]),
        "stem weight gradient": lambda: call("tbn_audio_stem_wgrad", ptr(dy), 64, ptr(x), ptr(dw), R, h, w, ptr(ws), st),
        "copy, weight gradient's bytes": lambda: dst[:wg_bytes // 8].copy_(src[:wg_bytes // 8]),
    }
    nbytes = {"stem forward (epilogue 1)": fwd_bytes, "copy, forward's bytes": fwd_bytes, "stem weight gradient": wg_bytes,
              "copy, weight gradient's bytes": wg_bytes}
    return arms, nbytes


def wgrad_split(h, w, dev):
    """{kernel name: median ms} of the weight gradient's launches, from the library's kernel timeline (begin / end events
    that ride on each dispatch), over LAUNCHES calls"""
    import csv
    import tempfile
    from attention_based_tbn_amd._lib import call
    arms, _ = stem_arms(h, w, dev)
    run = arms["stem weight gradient"]
    run()
    call("tbn_timeline_enable", 1)
    for _ in range(LAUNCHES):
        run()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "timeline.csv")
        call("tbn_timeline_dump", path.encode())
        call("tbn_timeline_enable", 0)
        seen = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                seen.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    return {k: statistics.median(v) for k, v in seen.items()}


def model_arms(dev):
    from attention_based_tbn_amd.core.models import BNInception, BNInception_Audio
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(R, 1, 256, 256, generator=g, device=dev)
    Rw = torch.randn(R, 1024, generator=g, device=dev)
    nets = {"BNInception_Audio (operators)": BNInception_Audio(1000, False).to(dev).train(),
            "BNInception(1000, 1) (engine)": BNInception(1000, 1).to(dev).train()}

    def step(net):
        def run():
            for p in net.parameters():
                p.grad = None
            (net(x) * Rw).sum().backward()
        return run
    return {k: step(n) for k, n in nets.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "bna_ops.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bna_step.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = ["# BNInception_Audio on the operator route (scripts/bna_step.py)", "",
             "One MI355X, one process, R = %d frames.  Medians of %d rounds after a warm-up round, arms alternated inside a "
             "round; (min .. max) beside them." % (R, ROUNDS), "",
             "## The stem kernels (device events around %d back-to-back launches)" % LAUNCHES, "",
             "| input | arm | algorithmic MB | ms | GB/s | share of the copy's rate |", "|---|---|---|---|---|---|"]
    for h, w in ((256, 256), (256, 420)):
        arms, nbytes = stem_arms(h, w, dev)
        res = rounds(arms, events_ms, LAUNCHES)
        for k, (med, lo, hi) in res.items():
            copy = res["copy, forward's bytes" if "forward" in k else "copy, weight gradient's bytes"][0]
            lines.append("| %d x %d | %s | %.1f | %.4f (%.4f .. %.4f) | %.0f | %.2f |"
                         % (h, w, k, nbytes[k] / 1e6, med, lo, hi, nbytes[k] / med / 1e6, copy / med))
        del arms
        torch.cuda.empty_cache()
    lines += ["", "The weight gradient's launches at 256 x 256, each alone (library timeline, median of %d calls):" % LAUNCHES, "",
              "| kernel | ms |", "|---|---|"]
    lines += ["| `%s` | %.4f |" % kv for kv in wgrad_split(256, 256, dev).items()]
    torch.cuda.empty_cache()
    res = rounds(model_arms(dev), host_ms, STEPS)
    eng = res["BNInception(1000, 1) (engine)"][0]
    lines += ["", "## Forward + backward at 256 x 256 (host clock around %d steps ending in a synchronise)" % STEPS, "",
              "| backbone | ms per step | against the engine |", "|---|---|---|"]
    for k, (med, lo, hi) in res.items():
        lines.append("| %s | %.2f (%.2f .. %.2f) | %.2f x |" % (k, med, lo, hi, med / eng))
    notes = ""
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = f.read()
        if MARK in old:
            notes = old[old.index(MARK) + len(MARK):]
    text = "\n".join(lines) + "\n\n" + MARK + notes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text if text.endswith("\n") else text + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
