#!/usr/bin/env python3
"""Compare the device code of two builds of libwvknn.so kernel by kernel.

    tools/kernel_digest.py PARENT.so NEW.so [-o profiles/NAME.json]

From each library: the gfx950 code objects of its .hip_fatbin section (one
offload bundle per translation unit), each disassembled with llvm-objdump; for
every kernel symbol (a function with a NAME.kd descriptor) the sha256 of its
instruction text, addresses, encodings and offset comments stripped.  The two
libraries are compared as sets of (kernel name, digest) pairs: a host-only
change leaves the new set a subset of the parent's (a unit that stops
launching a kernel stops instantiating it; the same kernel then still comes
from another unit) and the set of names identical.  Exit status 0 on that
verdict, 1 otherwise.
"""
import argparse
import collections
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib: str, tmp: str):
    """The gfx950 code objects of lib's fat binary, as files under tmp."""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib,
                    os.path.join(tmp, "unused.so")], check=True)
    blob = open(fat, "rb").read()
    out, pos = [], blob.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                path = os.path.join(tmp, f"co{len(out)}.o")
                with open(path, "wb") as f:
                    f.write(blob[pos + off:pos + off + size])
                out.append(path)
        pos = blob.find(MAGIC, p)
    if not out:
        raise SystemExit(f"{lib}: no gfx950 code object in .hip_fatbin (a compressed bundle?)")
    return out


SYM = re.compile(r"^[0-9a-f]* ?<(.+)>:$")
STRIP = re.compile(r"\s*//.*$|<[^>]*\+0x[0-9a-f]+>")
PCREL = re.compile(r"^(s_addc?_u32 s\d+, s\d+, )(0x[0-9a-f]+|-?\d+)$")


def kernel_digests(co: str):
    """{(kernel name, digest)} of one code object."""
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], check=True, capture_output=True,
                          text=True).stdout
    kernels = {line.split()[-1][:-3] for line in syms.splitlines() if line.rstrip().endswith(".kd")}
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                         check=True, capture_output=True, text=True).stdout
    pairs, name, h, pcrel = set(), None, None, 0
    for line in dis.splitlines() + ["<end>:"]:
        m = SYM.match(line.strip())
        if m:
            if name in kernels:
                pairs.add((name, h.hexdigest()))
            name, h = m.group(1), hashlib.sha256()
        elif name is not None and line.strip() and line.strip() != "...":  # "...": zero padding behind a function
            text = STRIP.sub("", line).strip()
            # s_getpc_b64 + s_add_u32 / s_addc_u32 literal: a pc-relative offset to a function or a
            # constant elsewhere in the code object, which moves with the object's layout
            if text.startswith("s_getpc_b64"):
                pcrel = 2
            elif pcrel and PCREL.match(text):
                text, pcrel = PCREL.sub(r"\1<rel>", text), pcrel - 1
            h.update((text + "\n").encode())
    missing = kernels - {n for n, _ in pairs}
    if missing:
        raise SystemExit(f"{co}: no disassembly for {sorted(missing)[:3]}")
    return pairs


def library_digests(lib: str):
    with tempfile.TemporaryDirectory() as tmp:
        pairs = collections.Counter()  # a kernel that several units instantiate counts once per unit
        for co in code_objects(lib, tmp):
            pairs.update(kernel_digests(co))
        return pairs


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    old_c, new_c = library_digests(a.parent), library_digests(a.new)
    old, new = set(old_c), set(new_c)
    old_names, new_names = sorted({n for n, _ in old}), sorted({n for n, _ in new})
    added = sorted(new - old)
    ok = not added and old_names == new_names
    res = {
        "parent_pairs": sum(old_c.values()), "new_pairs": sum(new_c.values()),
        "parent_distinct_pairs": len(old), "new_distinct_pairs": len(new),
        "parent_kernel_names": old_names, "new_kernel_names": new_names,
        "pairs_not_in_parent": [list(p) for p in added],
        "pairs_only_in_parent": [list(p) for p in sorted(old - new)],
        "names_identical": old_names == new_names,
        "verdict": "device code unchanged" if ok else "DEVICE CODE DIFFERS",
    }
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_names")}, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
