#!/usr/bin/env python3
"""Device-code comparison of two builds, kernel by kernel; needs no GPU.

    tools/codeobj_diff.py PARENT_BUILD_DIR BRANCH_BUILD_DIR [--objects NAME ...]

The two directories hold the object files of two builds (floodplanet_code_amd/csrc/build_NAME of tools/build_variant.sh).
From every object (all *.o of a directory, or the named ones; a name may exist on one side only -- a kernel may live in
another object after a split) the gfx950 code object is taken out of .hip_fatbin (llvm-objcopy, clang-offload-bundler
--unbundle) and its kernels are matched across all objects of a side by demangled name.  Per kernel one line: same /
DIFFERENT / ADDED / REMOVED, the code size, and from the code object's metadata VGPRs, SGPRs, spilled VGPRs / SGPRs,
scratch bytes and static LDS bytes (parent -> branch where they differ).  For a kernel whose machine code differs, the
multiset difference of the instruction mnemonics (llvm-objdump -d) follows.  Exit status 0 only if no kernel was added,
removed or changed."""
import argparse
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("vspill", ".vgpr_spill_count"), ("sspill", ".sgpr_spill_count"),
        ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"))


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """the gfx950 code object inside a host object file (None: the object carries no device code)"""
    stem = os.path.join(tmp, os.path.basename(obj))
    try:
        run("llvm-objcopy", "--dump-section", f".hip_fatbin={stem}.fatbin", obj)
    except subprocess.CalledProcessError:      # no such section
        return None
    if not os.path.exists(stem + ".fatbin") or TARGET not in run("clang-offload-bundler", "--list", "--type=o", f"--input={stem}.fatbin"):
        return None
    run("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={stem}.fatbin", f"--output={stem}.co")
    return stem + ".co"


def func_symbols(co, demangle):
    """{symbol index: (address, size, name)} of the FUNC symbols of .symtab"""
    out = {}
    table = run("llvm-readelf", "-s", "-W", *(["-C"] if demangle else []), co).split("Symbol table '.symtab'")[-1]
    for line in table.splitlines():
        m = re.match(r"\s*(\d+):\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\d+\s+(.+)$", line)
        if m:
            out[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3)), m.group(4).strip())
    return out


def kernels_of(co):
    """{demangled name: dict(code=bytes, sym=mangled name, co=path, vgpr=..., ...)} of one code object"""
    meta, cur = {}, None
    for line in run("llvm-readelf", "--notes", co).splitlines():
        if re.match(r"\s+- \.", line):
            cur = {}
        m = re.match(r"\s+(?:- )?(\.\w+):\s+(\S+)\s*$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    text = next(re.split(r"\s+", l.split("]", 1)[1].strip()) for l in run("llvm-readelf", "-S", "-W", co).splitlines()
                if re.search(r"\]\s+\.text\s", l))
    text_addr, text_off = int(text[2], 16), int(text[3], 16)
    blob = open(co, "rb").read()
    mangled, plain = func_symbols(co, False), func_symbols(co, True)
    out = {}
    for idx, (addr, size, sym) in mangled.items():
        if sym not in meta:          # a device function that is no kernel
            continue
        off = addr - text_addr + text_off
        k = dict(code=blob[off:off + size], sym=sym, co=co)
        k.update({short: int(meta[sym].get(key, 0)) for short, key in META})
        out[plain[idx][2]] = k
    return out


def side(directory, names, tmp):
    kernels = {}
    objs = names if names else sorted(f for f in os.listdir(directory) if f.endswith(".o"))
    for name in objs:
        path = os.path.join(directory, name)
        if not os.path.exists(path):
            continue
        sub = os.path.join(tmp, str(len(os.listdir(tmp))))
        os.mkdir(sub)
        co = code_object(path, sub)
        for kname, k in (kernels_of(co) if co else {}).items():
            k["obj"] = name
            kernels.setdefault(kname, []).append(k)
    # two different kernels of one name (internal linkage) are told apart by a hash of their code, on both sides alike, so that
    # the same kernel keeps its key when it moves to another object; identical copies count once
    out = {}
    for kname, ks in kernels.items():
        codes = {k["code"] for k in ks}
        for k in ks:
            out[kname if len(codes) == 1 else f"{kname} #{hashlib.sha256(k['code']).hexdigest()[:8]}"] = k
    return out


def mnemonics(k):
    c = collections.Counter()
    for line in run("llvm-objdump", "-d", f"--disassemble-symbols={k['sym']}", k["co"]).splitlines():
        m = re.match(r"\t(\w+)", line)
        if m:
            c[m.group(1)] += 1
    return c


def figures(a, b):
    def one(key):
        va, vb = (a or b)[key], (b or a)[key]
        return f"{key} {va}" if va == vb else f"{key} {va} -> {vb}"
    size = one("size")
    return ", ".join([size] + [one(short) for short, _ in META])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_dir")
    ap.add_argument("branch_dir")
    ap.add_argument("--objects", nargs="+", default=None, help="object file names looked up in both directories")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        pa, br = os.path.join(tmp, "parent"), os.path.join(tmp, "branch")
        os.mkdir(pa), os.mkdir(br)
        for name in args.objects or []:
            if not any(os.path.exists(os.path.join(d, name)) for d in (args.parent_dir, args.branch_dir)):
                sys.exit(f"codeobj_diff: {name} is in neither directory")
        A, B = side(args.parent_dir, args.objects, pa), side(args.branch_dir, args.objects, br)
        for k in list(A.values()) + list(B.values()):
            k["size"] = len(k["code"])
        counts = collections.Counter()
        for name in sorted(set(A) | set(B)):
            a, b = A.get(name), B.get(name)
            verdict = "REMOVED" if b is None else "ADDED" if a is None else "same" if a["code"] == b["code"] else "DIFFERENT"
            counts[verdict] += 1
            where = (a or b)["obj"] if a is None or b is None or a["obj"] == b["obj"] else f"{a['obj']} -> {b['obj']}"
            print(f"{verdict:9s} {name}  [{where}]  {figures(a, b)}")
            if verdict == "DIFFERENT":
                ma, mb = mnemonics(a), mnemonics(b)
                gone, new = ma - mb, mb - ma
                print("          mnemonics parent - branch: " + (", ".join(f"{m} x{n}" for m, n in sorted(gone.items())) or "none"))
                print("          mnemonics branch - parent: " + (", ".join(f"{m} x{n}" for m, n in sorted(new.items())) or "none"))
        print("kernels: " + ", ".join(f"{counts[v]} {v}" for v in ("same", "DIFFERENT", "ADDED", "REMOVED")))
        return 0 if counts["same"] == sum(counts.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
