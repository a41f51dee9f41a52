#!/usr/bin/env python3
"""How often the bilateral filter's fp32 chain falls back to double on the benchmark's depth streams -- on the CPU, through
tsdf_selftest_bilateral_chain_image (the staged kernel's own tap expressions and test, wave by wave), and a bit-for-bit check of that
host run against the oracle on the first frame of each stream.
    python tools/bilateral_chain_shares.py [first_frame last_frame]"""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle as O
from tsdf_amd import _capi, synth

W, H = 640, 480


def shares(depth, out=None):
    counts = (C.c_uint64 * 4)()
    rc = _capi.lib.tsdf_selftest_bilateral_chain_image(30.0, 4.5, depth.ctypes.data, 16, W, H,
                                                       out.ctypes.data if out is not None else None, counts)
    assert rc == 0, _capi.lib.tsdf_last_error()
    return np.array(list(counts), dtype=np.int64)


def main():
    first, last = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (0, 25)
    O.build()
    for name, seed, n_stream, inside in (("config3", 0x5EED0003, 200, False), ("config4", 0x5EED0004, 100, True)):
        frames = [np.ascontiguousarray(synth.depth_frame(i, n_stream, seed=seed, inside=inside)[0]) for i in range(first, last + 1)]
        out = np.empty_like(frames[0])
        shares(frames[0], out)
        same = np.array_equal(out.reshape(H, W), O.bilateral_u16(frames[0], W, H, 30.0, 4.5, nthreads=O.max_threads()))
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            per_frame = list(pool.map(shares, frames))
        t = np.sum(per_frame, axis=0)
        worst = max(c[1] / c[0] for c in per_frame)
        print("%s (seed 0x%X, frames %d-%d): %d wave half columns, %d fall back = %.4f %% (worst frame %.4f %%); "
              "%d lane half columns, %d fail = %.5f %%; host chain == oracle on frame %d: %s"
              % (name, seed, first, last, t[0], t[1], 100.0 * t[1] / t[0], 100.0 * worst, t[2], t[3], 100.0 * t[3] / t[2], first, same))


if __name__ == "__main__":
    main()
