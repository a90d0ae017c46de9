"""SHA-256 of what every split-bf16 convolution instantiation writes (conv_bf16x.hip), to compare two builds of the library.

  python scripts/bf16x_hashes.py [--out FILE]                       the shipped library
  TBN_LIB=scripts/ab/lib_<variant>.so python scripts/bf16x_hashes.py [--out FILE]     a variant build (build.py)

Through the C ABI (tbn_conv_launch, tbn_conv_split_weights), inputs drawn on the CPU from fixed seeds:
  * the three kernels -- 3x3 splitting its weights while staging (flag 32 / 64), 3x3 on weight planes (+ 128), pointwise on
    weight planes (+ 128, 1x1) -- x {bf16x6, bf16x3} x the eight tiles and the heuristic tile (0, 0) x epilogue {0 with a
    bias, 2} on two shapes per kernel: (2, 9, 11, 32, 160) has one K chunk, ragged M and ragged Cout; (1, 56, 56, 64, 192)
    and (2, 14, 14, 608, 320) have several chunks, and the 56-wide 3x3 map takes <2,3> / <2,4> at bf16x6 past 64 KB of LDS
    (the launcher raises the dynamic-LDS limit of those instantiations);
  * the weight planes of each shape's weight tensor, both plane counts (bf16x_split_planes_kernel).
One line per output: "<key> <sha256>", then the count.  Equal files from two builds = the builds compute the same bits.
Stops at the first failing launch.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attention_based_tbn_amd._lib import ConvDesc, call, lib, ptr  # noqa: E402

DEV = "cuda"
SHAPES = {3: [(2, 9, 11, 32, 160), (1, 56, 56, 64, 192)],      # tests/bf16x_emu.py CASES
          1: [(2, 9, 11, 32, 160), (2, 14, 14, 608, 320)]}     # tests/bf16x_pw_emu.py PW_CASES
KINDS = [("3x3", 3, 0), ("3x3_planes", 3, 128), ("pw", 1, 128)]
TILES = [(mt, nt) for mt in (1, 2) for nt in (1, 2, 3, 4)] + [(0, 0)]


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(61)
    lines = []
    for kind, k, planes_flag in KINDS:
        for n, h, w, cin, cout in SHAPES[k]:
            x = torch.randn(n, h, w, cin, generator=g).to(DEV)
            wt = (torch.randn(cout, k, k, cin, generator=g) / (k * k * cin) ** 0.5).to(DEV)
            bias, sh = torch.randn(cout, generator=g).to(DEV), torch.randn(cout, generator=g).to(DEV)
            sc = (torch.rand(cout, generator=g) + 0.5).to(DEV)
            for flag, np_ in ((32, 6), (64, 3)):
                weight = wt
                if planes_flag:
                    weight = torch.full((lib().tbn_conv_weight_planes_bytes(cout, k, cin, np_),), 0xa5, dtype=torch.uint8, device=DEV)
                    call("tbn_conv_split_weights", ptr(wt), cout, k, cin, np_, ptr(weight), st)
                    lines.append("split np%d %dx%dx%dx%d %s" % (np_, cout, k, k, cin, sha(weight)))
                for mt, nt in TILES:
                    for epi in (0, 2):
                        y = torch.full((n, h, w, cout), 3.0, device=DEV)
                        d = ConvDesc()
                        d.inp, d.in_ld, d.weight, d.out, d.out_ld = ptr(x), cin, ptr(weight), ptr(y), cout
                        d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.pad = n, h, w, cin, cout, k, 1, k // 2
                        d.epilogue, d.flags = epi, flag | planes_flag
                        if epi == 2:
                            d.scale, d.shift = ptr(sc), ptr(sh)
                        else:
                            d.bias = ptr(bias)
                        call("tbn_conv_launch", C.byref(d), mt, nt, 0, st)
                        lines.append("%s bf16x%d %s tile %d,%d epi %d %s" % (
                            kind, np_, "x".join(map(str, (n, h, w, cin, cout))), mt, nt, epi, sha(y)))
    lines.append("outputs hashed: %d" % len(lines))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
