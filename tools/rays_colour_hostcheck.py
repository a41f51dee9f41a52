"""The host check of coloured ray integration ("Checked without a GPU"): writes every call of every case set of
tests/rays_colour_cases.py with the CPU reference's per-voxel (c_v, R_v, G_v, B_v) to a scratch directory, builds
tools/rays_colour_hostcheck.cpp -- rays_walk_sdf compiled for the host with -ffp-contract=off, AddressSanitizer and UBSan, a stand-alone
program -- and runs it over them as a child process.  No GPU, no device code.

    python tools/rays_colour_hostcheck.py [--hipcc /opt/rocm/bin/hipcc]
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
    a = ap.parse_args()
    import oracle as O
    from tests import rays_colour_cases as CC
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rays_colour_hostcheck")
        # the sanitizers are for the host side only: -Xarch_host at the compile, and the plain flag at the link step alone, where no
        # device code is compiled
        obj = os.path.join(tmp, "rays_colour_hostcheck.o")
        subprocess.check_call([a.hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tsdf_amd", "csrc"), "-c",
                               os.path.join(ROOT, "tools", "rays_colour_hostcheck.cpp"), "-o", obj])
        subprocess.check_call([a.hipcc, "-fsanitize=address,undefined", obj, "-o", exe])
        files = []
        for c in CC.cases():
            _, geom = CC.make_geometry(O, c)
            dims, vs, offset, trunc = geom
            cols = CC.reference(c.name)[5]
            for k, ((o, p, rgb, lo, hi, flags), col) in enumerate(zip(c.calls, cols)):
                dense = np.zeros((int(np.prod(dims)), 4), np.uint64)
                for (x, y, z), v in col.items():
                    dense[(z * dims[1] + y) * dims[0] + x] = v
                path = os.path.join(tmp, "%s_%d.call" % (c.name, k))
                with open(path, "wb") as f:
                    f.write(struct.pack("<3I3f3f3fiIQQ", *dims, *[float(v) for v in vs], *[float(v) for v in offset], float(trunc), float(lo),
                                        float(hi), int(flags), 0, len(p), len(o)))
                    for arr in (o, p, rgb, dense):
                        f.write(np.ascontiguousarray(arr).tobytes())
                files.append(path)
        sys.exit(subprocess.call([exe] + files))


if __name__ == "__main__":
    main()
