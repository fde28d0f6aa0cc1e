#!/usr/bin/env python3
"""Per kernel of the built library: size of the kernel-argument segment and kernel-argument preload length (dwords that
gfx950 delivers in SGPRs when a wave starts; csrc/Makefile PRELOAD).

    python tools/kernarg_report.py [libmi355schur.so] [--json] [--filter SUBSTRING]

Source: the kernel descriptors (`<kernel>.kd`, 64 bytes each) of the gfx950 code object bundled in the library, printed by
llvm-objdump as `.amdhsa_*` directives. Only `.amdhsa_kernarg_size` and `.amdhsa_user_sgpr_kernarg_preload_length` are read.
"""
import argparse
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "julia-phd-krylov-spdes_amd", "libmi355schur.so")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def llvm_tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/lib/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if not p:
        raise RuntimeError(f"{name} not found (ROCM_PATH/llvm/bin or PATH)")
    return p


def code_object(lib, arch="gfx950"):
    """bytes of the `arch` code object in the library's offload bundle (uncompressed clang-offload-bundler layout)"""
    data = open(lib, "rb").read()
    base = data.find(BUNDLE_MAGIC)
    if base < 0:
        raise RuntimeError(f"{lib}: no offload bundle")
    n, = struct.unpack_from("<Q", data, base + len(BUNDLE_MAGIC))
    pos = base + len(BUNDLE_MAGIC) + 8
    for _ in range(n):
        off, size, tlen = struct.unpack_from("<QQQ", data, pos)
        triple = data[pos + 24:pos + 24 + tlen].decode()
        pos += 24 + tlen
        if triple.startswith("hip") and triple.endswith(arch) and size:
            return data[base + off:base + off + size]
    raise RuntimeError(f"{lib}: no {arch} code object in the bundle")


def report(lib=DEFAULT_LIB):
    """{mangled kernel name: (kernarg segment bytes, preload dwords)}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "device.co")
        with open(co, "wb") as f:
            f.write(code_object(lib))
        text = subprocess.run([llvm_tool("llvm-objdump"), "-d", "--section=.rodata", co], check=True, capture_output=True,
                              text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
            out[name] = [None, 0]
            continue
        if name is None:
            continue
        m = re.match(r"\s*\.amdhsa_kernarg_size\s+(\d+)", line)
        if m:
            out[name][0] = int(m.group(1))
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
        if m:
            out[name][1] = int(m.group(1))
        if ".end_amdhsa_kernel" in line:
            name = None
    return {k: tuple(v) for k, v in out.items()}


def demangle(names):
    for tool in ("llvm-cxxfilt", "c++filt"):
        try:
            exe = llvm_tool(tool)
            res = subprocess.run([exe], input="\n".join(names), capture_output=True, text=True, check=True)
            return dict(zip(names, res.stdout.splitlines()))
        except (RuntimeError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}   # mangled names if no demangler is installed


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib", nargs="?", default=DEFAULT_LIB)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    args = ap.parse_args()
    rep = report(args.lib)
    if args.json:
        json.dump({k: {"kernarg_size": v[0], "preload_length": v[1]} for k, v in rep.items()}, sys.stdout, indent=1)
        print()
        return
    pretty = demangle(list(rep))
    print(f"{'kernarg B':>9} {'preload':>7}  kernel")
    for k in sorted(rep, key=lambda k: pretty[k]):
        if args.filter in pretty[k]:
            print(f"{rep[k][0]:9d} {rep[k][1]:7d}  {pretty[k]}")
    print(f"{len(rep)} kernels, {sum(1 for v in rep.values() if v[1])} with a preload length > 0")


if __name__ == "__main__":
    main()
