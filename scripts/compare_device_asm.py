"""Compares two device assembly files of one source kernel by kernel, whatever order the kernels were emitted in.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include -S --offload-device-only SRC.hip -o before.s   (at the parent)
    hipcc ... -S --offload-device-only SRC.hip -o after.s                                                    (at the change)
    python scripts/compare_device_asm.py before.s after.s

A host-side change that instantiates the same kernels in another order moves their sections and renumbers the local
labels, so a plain diff is large although no kernel changed.  Here the file is cut at every section directive, the
function numbers of local labels (.LBB12_3, BB12_3 in comments, .Lfunc_end12) and the per-file id symbol (__hip_cuid_*)
are blanked, and the sections -- instruction streams, kernel descriptors, resource-usage comments -- are compared as
multisets keyed by their directive (a kernel's name is part of it); the metadata note is compared as sorted lines.
Prints every section that differs and exits 1, or "identical" and exits 0."""

import collections
import re
import sys


def sections(path):
    out, key, buf = collections.defaultdict(list), "<head>", []
    for line in open(path):
        if line.startswith(("\t.section", "\t.text", "\t.amdgpu_metadata")):
            out[key].append("".join(buf))
            key, buf = line.strip(), []
        line = re.sub(r"\.L(func_end|func_begin|tmp|JTI)\d+", r".L\1", re.sub(r"BB\d+_", "BB_", line))
        buf.append(re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line))
    out[key].append("".join(buf))
    return out


def main(before, after):
    a, b = sections(before), sections(after)
    differ = []
    for key in sorted(set(a) | set(b)):
        if key.startswith(".amdgpu_metadata"):
            same = sorted("".join(a[key]).splitlines()) == sorted("".join(b[key]).splitlines())
        else:
            same = sorted(a[key]) == sorted(b[key])
        if not same:
            differ.append(key)
    for key in differ:
        print("DIFFERS", key[:200])
    print(f"{len(a)} / {len(b)} sections: " + (f"{len(differ)} differ" if differ else "identical"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
