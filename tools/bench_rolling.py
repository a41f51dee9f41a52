"""Cost of the rolling volume (include/tsdf_amd.h, "rolling volume") at 512^3 with the first 25 frames of bench.py's stream (640 x 480, seed
0x5EED0003) fused into 8-bit weights.  Prints one JSON line and writes it to profiles/rolling_bench.json.

Host wall-clock times of whole calls, each ending in a device synchronise, as the median (and range) of --reps repetitions after
--warmup, the variants alternating inside every repetition; after every shift the volume is put back as it was, outside the timed window:

  snapshot_ms, restore_ms           the sparse snapshot's two calls on the same volume, and
  snapshot_restore_ms               both in one window: the floor of a shift by construction
  shift_100_ms, shift_111_ms        tsdf_volume_shift by (1, 0, 0) and by (1, 1, 1) bricks without `leaving`,
  shift_100_leaving_ms, ..          and with it
  page_in_100_ms, page_in_1000_ms   tsdf_volume_restore_shifted with TSDF_RESTORE_KEEP_OTHERS of 100 and of 1000 bricks
  select_ms                         tsdf_snapshot_select of the inner half of the grid per axis from the volume's snapshot

With --parent-tree DIR (a built checkout of the parent commit) tsdf_volume_restore alone is timed in fresh child processes, the parent's
library and this one alternating --ab-rounds times: the medians of each side and their spread between repeats go into "restore_ab".
Nothing about the speed was known when the feature was specified, and no pass mark is fixed for the shift.

    python tools/bench_rolling.py [--size 512] [--frames 25] [--reps 10] [--warmup 2] [--parent-tree DIR] [--ab-rounds 3]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, PERIOD = 0x5EED0003, 200


def fused_volume(tsdf_amd, n, n_frames):
    from tsdf_amd import synth
    vol = tsdf_amd.TSDFVolume((n,) * 3, (3000.0,) * 3)
    for i in range(n_frames):
        d, cam = synth.depth_frame(i, PERIOD, seed=SEED)
        vol.integrate(d, synth.WIDTH, synth.HEIGHT, cam)
    vol.synchronize()
    return vol


def timed(vol, variants, reps, warmup, after=None):
    times = {v: [] for v in variants}
    for r in range(warmup + reps):
        for v, fn in variants.items():
            vol.synchronize()
            t0 = time.perf_counter()
            fn()
            vol.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                times[v].append(t)
            if after:
                after(v)
    return times


def summary(times):
    res = {}
    for v, ts in times.items():
        res[v + "_ms"] = round(float(np.median(ts)), 4)
        res[v + "_ms_range"] = [round(min(ts), 4), round(max(ts), 4)]
    return res


def ab_summary(runs):
    """The two sides' medians per round, each side's spread between its own repeats, and the change against the parent: round by round
    (the two runs of a round are neighbours in time), as medians of medians, and whether every change median lies inside the parent's own
    range (with as many repeats on both sides that fails often for two equal libraries: it is recorded, not relied on)."""
    ab = {}
    for side, rs in runs.items():
        medians = [r["restore_ms"] for r in rs]
        ab[side] = {"restore_ms_medians": medians, "spread_ms": round(max(medians) - min(medians), 4),
                    "ranges": [r["range"] for r in rs], "n_bricks": rs[0]["n_bricks"]}
    p, c = ab["parent"]["restore_ms_medians"], ab["change"]["restore_ms_medians"]
    ab["change_minus_parent_ms_per_round"] = [round(y - x, 4) for x, y in zip(p, c)]
    ab["change_minus_parent_ms"] = round(float(np.median(c) - np.median(p)), 4)
    ab["largest_difference_of_a_round_within_parent_spread"] = bool(max(abs(y - x) for x, y in zip(p, c)) <= max(p) - min(p))
    ab["change_medians_inside_parent_range"] = all(min(p) <= m <= max(p) for m in c)
    return ab


def restore_only(a):
    """Child process: the old entry point alone, with whatever tree is first on the path (only what the parent commit has is used)."""
    sys.path.insert(0, os.path.abspath(a.tree))
    import tsdf_amd
    assert os.path.abspath(tsdf_amd.__file__).startswith(os.path.abspath(a.tree)), tsdf_amd.__file__
    vol = fused_volume(tsdf_amd, a.size, a.frames)
    snap = vol.snapshot()
    ts = timed(vol, {"restore": lambda: vol.restore(snap)}, a.reps, a.warmup)["restore"]
    print(json.dumps({"restore_ms": round(float(np.median(ts)), 4), "range": [round(min(ts), 4), round(max(ts), 4)], "n_bricks": snap.n_bricks}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=25, help="frames fused before the measurements")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit, for the A/B of tsdf_volume_restore")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_bench.json"))
    ap.add_argument("--restore-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.restore_only:
        return restore_only(a)

    sys.path.insert(0, ROOT)
    import torch
    import tsdf_amd
    assert torch.cuda.is_available(), "bench_rolling needs a GPU"
    n = a.size
    assert n % 8 == 0
    vol = fused_volume(tsdf_amd, n, a.frames)
    assert vol.weight_storage() == (8, False)
    offset = tuple(vol.offset())
    base = vol.snapshot()                                    # the state every variant starts from
    D, Wt = vol.get_distance_data(), vol.get_weight_data()
    ids, d, w, _ = base.download()
    assert len(ids) >= 1000, "the scene has fewer than 1000 live bricks at this size"
    i = base.info
    geometry = dict(fill_distance=i.fill_distance, voxel_size=tuple(i.voxel_size), offset=tuple(i.offset))
    pick = lambda k: np.sort(np.random.default_rng(k).choice(len(ids), size=k, replace=False))
    pages = {k: tsdf_amd.Snapshot.from_arrays((n,) * 3, ids[pick(k)], d[pick(k)], w[pick(k)], **geometry) for k in (100, 1000)}
    del d, w
    work, leaving, selected = tsdf_amd.Snapshot(), tsdf_amd.Snapshot(), tsdf_amd.Snapshot()
    nb = n // 8
    left = {}

    def put_back(v):
        if v.startswith("shift"):
            vol.restore(base)
            vol.offset(*offset)
            vol.synchronize()

    def snapshot_restore():
        vol.snapshot(into=work)
        vol.restore(work)

    def shift(s, out):
        def run():
            if out:
                left[s] = vol.shift(s, work=work, leaving=leaving).n_bricks
            else:
                tsdf_amd._capi.check(tsdf_amd._capi.lib.tsdf_volume_shift(vol._h, (ctypes.c_int32 * 3)(*s), work._h, None))
        return run

    variants = {
        "snapshot": lambda: vol.snapshot(into=work),
        "restore": lambda: vol.restore(base),
        "snapshot_restore": snapshot_restore,
        "shift_100": shift((1, 0, 0), False),
        "shift_100_leaving": shift((1, 0, 0), True),
        "shift_111": shift((1, 1, 1), False),
        "shift_111_leaving": shift((1, 1, 1), True),
        "page_in_100": lambda: vol.restore(pages[100], keep_others=True),
        "page_in_1000": lambda: vol.restore(pages[1000], keep_others=True),
        "select": lambda: base.select((nb // 4,) * 3, (nb - nb // 4,) * 3, into=selected),
    }
    res = {"voxels": n ** 3, "bricks": nb ** 3, "live_bricks": int(i.n_bricks), "snapshot_bytes": int(i.bytes)}
    res.update(summary(timed(vol, variants, a.reps, a.warmup, after=put_back)))
    res["selected_bricks"] = selected.n_bricks
    res["leaving_bricks"] = {"%d%d%d" % s: k for s, k in left.items()}
    # the same product: paging in bricks of the state itself and putting the state back after every shift left the fused volume
    assert vol.get_distance_data().tobytes() == D.tobytes() and vol.get_weight_data().tobytes() == Wt.tobytes(), "the state differs"
    assert tuple(vol.offset()) == offset
    out = {"tool": "bench_rolling", "width": 640, "height": 480, "seed": "0x%X" % SEED, "frames_fused": a.frames, "reps": a.reps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "size": n, "times": res}
    for o in (base, work, leaving, selected, pages[100], pages[1000], vol):
        o.close()

    if a.parent_tree:
        runs = {"parent": [], "change": []}
        for _ in range(a.ab_rounds):
            for side, tree in (("parent", os.path.abspath(a.parent_tree)), ("change", ROOT)):
                cmd = [sys.executable, os.path.abspath(__file__), "--restore-only", "--tree", tree, "--size", str(n), "--frames", str(a.frames),
                       "--reps", str(a.reps), "--warmup", str(a.warmup)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
                assert r.returncode == 0, r.stdout + r.stderr
                runs[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out["restore_ab"] = ab_summary(runs)
        out["restore_ab"]["rounds"] = a.ab_rounds
    else:
        out["restore_ab"] = "not measured (no --parent-tree)"
    out["note"] = ("host wall-clock of whole calls that end in a device synchronise, medians with [min, max], the variants alternating inside "
                   "every repetition, the volume put back between shifts outside the timed window; snapshot_restore_ms is the floor of a shift "
                   "by construction (a shift is a snapshot, a select when leaving is asked for, and a restore at other coordinates); restore_ab: "
                   "tsdf_volume_restore alone in fresh processes, the parent commit's library and this one alternating; no pass mark was fixed")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
