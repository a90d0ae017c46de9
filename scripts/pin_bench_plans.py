"""Writes bench_plans.json, the launch plans every bench.py run adopts (bench.pin_plans), from plan-cache directories.

  TBN_PLAN_CACHE=/tmp/p python bench.py --steps 40 --warmup 5      # tunes the config-4 shapes and stores their plans
  TBN_PLAN_CACHE=/tmp/p python bench.py --config 3 --steps 5 --warmup 1 ...
  python scripts/pin_bench_plans.py /tmp/p [more directories: a later one wins for the same file name]

Re-tune after a kernel change: a plan only loads into the library version named in its file name, and shapes without a
committed plan are tuned in every run (the line's config.launch_plans says which)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(dirs):
    plans = {}
    for d in dirs:
        for name in sorted(os.listdir(d)):
            if name.startswith("tbnplan_") and name.endswith(".bin"):
                with open(os.path.join(d, name), "rb") as f:
                    plans[name] = f.read().hex()
    assert plans, "no tbnplan_*.bin file in " + " ".join(dirs)
    doc = {"what": "tuned launch plans (tbn_backbone_plan_export) of the benchmarked shapes, written by "
                   "scripts/pin_bench_plans.py; file names as core/models/bn_inception.py's plan cache",
           "plans": dict(sorted(plans.items()))}
    with open(os.path.join(ROOT, "bench_plans.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("\n".join(sorted(plans)))


if __name__ == "__main__":
    main(sys.argv[1:])
