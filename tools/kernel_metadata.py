#!/usr/bin/env python3
"""Register and memory figures of every kernel in a built libnerfdet_hip.so, from the code objects' metadata notes: one JSON object
{kernel symbol: [vgpr, sgpr, lds bytes, scratch bytes]}.  With two libraries, the kernels of the first whose figures differ in (or are
missing from) the second, and the kernels only the second has; exit status 1 when a kernel of the first changed.
    python tools/kernel_metadata.py nerf-det_amd/lib/libnerfdet_hip.so [other.so]
"""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def code_objects(lib):
    """The gfx code objects of every offload bundle in the library's .hip_fatbin section."""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        data = open(fat, "rb").read()
    at = data.find(MAGIC)
    while at >= 0:
        p = at + len(MAGIC)
        (n,) = struct.unpack_from("<Q", data, p)
        p += 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tlen].decode()
            p += tlen
            if "gfx" in triple and size:
                yield data[at + off:at + off + size]
        at = data.find(MAGIC, at + len(MAGIC))


def metadata(lib):
    out = {}
    for obj in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], check=True, capture_output=True, text=True).stdout
        # one "- .agpr_count:" ... block per kernel inside amdhsa.kernels
        for block in re.split(r"\n\s+- \.", notes):
            name = re.search(r"\.symbol:\s+'?([^\s']+?)(?:\.kd)?'?\s*$", block, flags=re.M)
            if not name:
                continue
            vals = [re.search(re.escape(k) + r":\s+(\d+)", block) for k in KEYS]
            if all(vals):
                out[name.group(1)] = [int(v.group(1)) for v in vals]
    return out


def main():
    a = metadata(sys.argv[1])
    if len(sys.argv) < 3:
        print(json.dumps(a, indent=0, sort_keys=True))
        return 0
    b = metadata(sys.argv[2])
    changed = {k: (a[k], b.get(k)) for k in a if a[k] != b.get(k)}
    new = sorted(k for k in b if k not in a)
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}: {len(a) - len(changed)} with identical vgpr / sgpr / lds / scratch, "
          f"{len(changed)} changed or missing, {len(new)} new")
    for k, (x, y) in sorted(changed.items()):
        print(f"  changed {k}: {x} -> {y}")
    for k in new:
        print(f"  new {k}: {b[k]}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
