#!/usr/bin/env python3
"""Register / LDS / occupancy figures of every kernel of one csrc file, from hipcc's kernel-resource-usage remarks.

    python scripts/kernel_resources.py k_dense.hip [extra hipcc flags]

or, of the library as built (every kernel whose name contains the words given; no compilation), from the metadata notes of
its code objects: VGPRs, SGPR and VGPR spills, scratch and LDS.

    python scripts/kernel_resources.py --lib [k_dense k_bm_tiles ...]
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spsparse_amd import build as b  # noqa: E402


BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
NOTE_KEYS = {".name": "name", ".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".sgpr_spill_count": "sgpr_spill",
             ".vgpr_spill_count": "vgpr_spill", ".private_segment_fixed_size": "scratch", ".group_segment_fixed_size": "lds"}


def code_objects(lib):
    """The gfx950 code objects (ELF images) of a built library: one offload bundle per translation unit in .hip_fatbin."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(b.hipcc()))), "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([os.path.join(tools, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "rest")])
        d = open(fat, "rb").read()
    at = d.find(BUNDLE_MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", d, at + len(BUNDLE_MAGIC))
        q = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", d, q)
            triple = d[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                yield d[at + off:at + off + size]
        at = d.find(BUNDLE_MAGIC, at + 1)


def library_kernels(lib=None):
    """{mangled kernel name: {"vgpr", "agpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch" (bytes per lane), "lds" (bytes per
    workgroup)}} of every kernel in the built library, read from the AMDGPU metadata note of each code object."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(b.hipcc()))), "llvm", "bin")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, elf in enumerate(code_objects(lib or b.LIB)):
            path = os.path.join(tmp, "co%d.elf" % i)
            open(path, "wb").write(elf)
            notes = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
            cur = None
            for ln in notes.splitlines():
                m = re.match(r"\s+(- )?(\.\w+):\s+(\S+)\s*$", ln)
                if ln.startswith("  - "):                            # a kernel's record begins
                    cur = {}
                if m and cur is not None and m.group(2) in NOTE_KEYS and len(ln) - len(ln.lstrip()) == (2 if m.group(1) else 4):
                    k = NOTE_KEYS[m.group(2)]
                    cur[k] = m.group(3) if k == "name" else int(m.group(3))
                    if k == "name":
                        out[cur["name"]] = cur
    return out


def main_lib(words):
    rows = library_kernels()
    names = sorted(n for n in rows if not words or any(w in n for w in words))
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    for n, d in zip(names, plain):
        r = rows[n]
        d = re.sub(r"\(.*", "", d).replace("void spsamd::", "")
        print("%-60s vgpr %4s sgpr-spill %4s vgpr-spill %3s scratch %4s lds %7s" % (d[:60], r.get("vgpr"), r.get("sgpr_spill"), r.get("vgpr_spill"), r.get("scratch"), r.get("lds")))


def main():
    if sys.argv[1] == "--lib":
        return main_lib(sys.argv[2:])
    src = os.path.join(b.CSRC, sys.argv[1])
    cmd = [b.hipcc()] + b.FLAGS + sys.argv[2:] + ["-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    cur = {}
    rows = []
    for ln in err.splitlines():
        m = re.search(r"remark: [^:]+:\d+:\d+:\s+(.*?)\s*\[-Rpass", ln) or re.search(r"remark:\s+(.*?)\s*\[-Rpass", ln)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    for r in rows:
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(.*", "", name).replace("void spsamd::", "")
        print("%-60s vgpr %4s agpr %3s sgpr %4s lds %7s scratch %4s occ %s" % (name[:60], r.get("VGPRs"), r.get("AGPRs"), r.get("SGPRs"),
              r.get("LDS Size [bytes/block]"), r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]")))


if __name__ == "__main__":
    main()
