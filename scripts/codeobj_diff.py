#!/usr/bin/env python3
"""Compares the gfx950 kernels of two builds symbol by symbol; no GPU needed.

    python scripts/codeobj_diff.py <dir or file A> <dir or file B>

Each argument is a directory of object files (csrc/ of a plain build, scripts/ab/obj_<variant>/ of a variant build) or
one file: a host object (its gfx950 code object is taken out of .hip_fatbin) or a device code object
(`hipcc --offload-device-only -c`).  Per file name present on both sides: the kernel (FUNC) symbols of A and B, the names
only one side has, and the names whose bytes differ.  Exit status 1 when any name or byte differs.
"""
import os
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(path, tmp):
    """bytes of the gfx950 code object inside `path` (or `path` itself when it already is one)"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] == b"\x7fELF" and struct.unpack_from("<H", data, 18)[0] == 224:   # EM_AMDGPU
        return data
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(tmp, "unused")],
                       capture_output=True)
    if r.returncode != 0:   # a source without kernels has no .hip_fatbin
        return None
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                    "--input=" + fat, "--output=" + co], check=True)
    with open(co, "rb") as f:
        return f.read()


def kernels(elf):
    """{symbol name: bytes} of every FUNC symbol of an ELF64 little-endian code object"""
    if elf is None:
        return {}
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in secs:
        if s[1] != 2:   # SHT_SYMTAB
            continue
        strtab = secs[s[6]]
        for off in range(s[4], s[4] + s[5], 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, off)
            if (info & 15) != 2 or shndx == 0 or shndx >= shnum:   # STT_FUNC, defined
                continue
            end = elf.index(b"\0", strtab[4] + name)
            sec = secs[shndx]
            beg = sec[4] + value - sec[3]
            out[elf[strtab[4] + name:end].decode()] = elf[beg:beg + size]
    return out


def objects(path):
    if os.path.isdir(path):
        return {f: os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith((".o", ".co"))}
    return {"": path}


def main():
    a, b = objects(sys.argv[1]), objects(sys.argv[2])
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(set(a) & set(b)):
            ka, kb = kernels(code_object(a[f], tmp)), kernels(code_object(b[f], tmp))
            only = sorted(set(ka) ^ set(kb))
            differ = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
            print("%-16s kernels %d / %d, names on one side only %d, byte-identical %d, differ %d"
                  % (f or os.path.basename(a[f]), len(ka), len(kb), len(only), len(set(ka) & set(kb)) - len(differ), len(differ)))
            for n in only:
                print("  only in %s: %s" % ("A" if n in ka else "B", n))
            for n in differ:
                print("  differs: %s (%d / %d bytes)" % (n, len(ka[n]), len(kb[n])))
            bad += len(only) + len(differ)
    for f in sorted(set(a) ^ set(b)):
        print("%-16s on one side only" % f)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
