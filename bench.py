#!/usr/bin/env python3
"""bench.py -- the TSDF hot path on MI355X: bilateral filter -> integrate -> raycast -> normals.

    python bench.py --gpus N --steps K --warmup W

A "step" is one 640x480 depth frame of the synthetic TUM surrogate (tsdf_amd/synth.py) pushed through the
whole path on a 512^3 / 3000 mm volume (BASELINE.json configs[2]); inputs are resident in HBM before the
timed region starts.  N > 1: the volume is split into N Z-slabs, one process per GPU (torch.distributed over
RCCL); every rank integrates its slab (+1 halo plane), ray casts the samples it owns, and one all-gather of
8-byte hit records {k, t} per pixel is merged by a min-k select.  Total work is fixed => "strong".

Rank 0 prints ONE JSON line.  `value` = voxels of the grid pushed through the whole step per second (whole
job).  A plain run does only what that figure needs: set up, warm up, time the K steps (R times, `--repeats`),
write `--dump-outputs`, print the line.  `--full` then goes on with everything else the benchmark measures and
checks, in the same object: per-stage figures (integrate Mvoxels/s, raycast Mrays/s) from untimed replays, the
per-step spread, the roofline of the dominant kernel, the host-buffer / ICP / tracking legs, the parity gate
against the oracle and the CPU baseline (the oracle, timed here on the host cores on a bounded sample).
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 640, 480
HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
SEED = 0x5EED0003            # config 3 stream


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload", choices=("config3", "config4"), default="config3",
                    help="config3 = BASELINE configs[2] (512^3, camera in front of the volume; the metric's configuration); config4 = "
                         "BASELINE configs[3] (1024^3 over the ranks' Z-slabs, camera inside the volume, seed 0x5EED0004, 100-frame stream)")
    ap.add_argument("--grid", type=int, default=None, help="voxels per side (default 512, or 1024 for --workload config4)")
    ap.add_argument("--physical", type=float, default=3000.0)
    ap.add_argument("--stream-frames", type=int, default=None, help="length of the synthetic trajectory (default 200; 100 for config4)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, everything else the benchmark measures and checks: untimed replays for the stage and kernel "
                         "times, the per-step spread, the weight-storage legs, the roofline, the host-buffer / ICP / tracking legs, the parity "
                         "gate, the CPU baseline (N > 1: every rank's times, the single-volume parity replay).  The options below marked "
                         "(--full) only trim or steer that part")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full)")
    ap.add_argument("--no-parity", action="store_true", help="(--full)")
    ap.add_argument("--event-period", type=int, default=0,
                    help="per-stage HIP events inside the TIMED region on every n-th step (0 = none: each record costs a few "
                         "microseconds of stream time).  Stage and kernel times always come from an untimed replay of the same frames "
                         "with every launch bracketed")
    ap.add_argument("--no-overlap", action="store_true", help="N > 1: filter + integrate frame i+1 after, not during, the exchange of frame i; N = 1: the next frame's filter "
                                                                 "after, not during, this frame's ray cast")
    ap.add_argument("--slab-plan", choices=("measured", "model", "uniform"), default="measured",
                    help="N > 1: Z-slab boundaries re-cut from the ranks' measured times on the first frames (default), from a "
                         "work estimate of a small planner volume, or equal plane counts")
    ap.add_argument("--plan-rounds", type=int, default=3, help="--slab-plan measured: rebalancing rounds (each costs a few frames)")
    ap.add_argument("--validate-merge", action="store_true",
                    help="(--full) N > 1: SURVEY.md 8e mode B after the measurements -- every rank all-gathers the distance slabs, casts the "
                         "whole volume the single-volume way and compares its bits with the merged picture (tsdf_slab_validate_merge)")
    ap.add_argument("--one-rank-slab-path", action="store_true",
                    help="--gpus 1 only: run the N > 1 code path (slab volume, slab ray cast, all-gather of the hit records over the "
                         "nccl = RCCL backend, merge) with a world of one rank -- the collective degenerates but RCCL initialises, "
                         "builds a communicator and runs on the box's GPU; what a 1-GPU box can check of the multi-GPU path")
    ap.add_argument("--torch-collective", action="store_true",
                    help="N > 1: the hit records go through torch.distributed.all_gather_into_tensor (the process group's own stream, "
                         "events on either side) instead of ncclAllGather called on the step's own HIP stream (tsdf_amd.multi.StreamAllGather)")
    ap.add_argument("--separate-tile-max", action="store_true",
                    help="integrate computes the depth tile maxima in a launch of its own (tsdf_integrate_device) instead of taking "
                         "them from the bilateral filter's launch (tsdf_bilateral_filter_u16_device_tiles + tsdf_integrate_device_tiles)")
    ap.add_argument("--tum-dir", default=None,
                    help="take the stream from a TUM-layout directory (depth/*.png + ground_truth.txt) through the host library's "
                         "TUMDataLoader instead of synthesising it: the frames tools/kinfu_stream.cpp sees (tools/compare_drivers.sh)")
    ap.add_argument("--cpu-budget-s", type=float, default=20.0, help="(--full)")
    ap.add_argument("--repeats", type=int, default=5,
                    help="the K-step timed region (barrier + synchronise on both sides, MAX over ranks) is run this many times, each on a freshly "
                         "cleared volume fed the same warm-up and the same K frames; ms_per_step / value are the MEDIAN region, every region is "
                         "listed in ms_per_step_runs")
    ap.add_argument("--parity-grid", type=int, default=None,
                    help="(--full) grid of the parity gate (default: the benchmarked grid, first and last timed frame against the oracle)")
    ap.add_argument("--spread-steps", type=int, default=100,
                    help="(--full) steps of the run that times every step on its own (step_ms_spread): at least --steps; 0 = --steps (the "
                         "profiling passes)")
    ap.add_argument("--path-only", action="store_true",
                    help="(--full) only the timed hot path and its roofline (no ICP / tracking / host-buffer legs): what the profiling passes run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy: the vertex and normal maps "
                         "(no-hit NaNs as 0, with a per-pixel validity mask each), and (one volume) a fixed seeded sample of the volume's distances and weights")
    a = ap.parse_args()
    if a.validate_merge and not a.full:
        ap.error("--validate-merge is a check of the --full run")
    if a.grid is None:
        a.grid = 1024 if a.workload == "config4" else 512
    if a.stream_frames is None:
        a.stream_frames = 100 if a.workload == "config4" else 200
    return a


_T0 = time.time()


def trace(msg):
    """BENCH_TRACE=1: wall-clock marks of the run's phases on stderr."""
    if os.environ.get("BENCH_TRACE"):
        print("[bench %8.2f s] %s" % (time.time() - _T0, msg), file=sys.stderr, flush=True)


def main():
    args = parse()
    # stdout carries exactly one JSON line.  Libraries write there too (RCCL prints a version banner on stdout when it builds
    # a communicator): file descriptor 1 is pointed at stderr for the life of the process and the line goes to the saved one.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # (before the HIP runtime starts: RCCL's IPC needs it on this host driver)
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` started plainly (the shape of the driver's N = 1 command): become the launcher -- the same
        # torch.distributed.run command the driver uses, one rank per GPU, rendezvous on 127.0.0.1; rank 0 of it prints the line
        import socket
        with socket.socket() as s_:
            s_.bind(("127.0.0.1", 0))
            port = s_.getsockname()[1]
        os.dup2(json_fd, 1)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        if os.environ.get("BENCH_LAUNCH_DRYRUN") == "1":     # (tests/test_bench_launcher.py: the command, not the run)
            print(json.dumps(cmd))
            return
        # a child process, not an exec: this process has loaded the HIP runtime with torch, and is never replaced
        raise SystemExit(subprocess.call(cmd))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d inside a world of %d ranks" % (args.gpus, world))
    # Debug aid for a 1-GPU box: TSDF_BENCH_SHARE_GPU=1 puts every rank on device 0 and uses gloo for the
    # collective, so the N>1 code path can be exercised (the numbers mean nothing then).
    share = os.environ.get("TSDF_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    elif world > torch.cuda.device_count():
        raise SystemExit("bench.py --gpus %d: this node shows %d GPU(s) (TSDF_BENCH_SHARE_GPU=1 walks the N > 1 path with every rank on "
                         "GPU 0 over gloo; its numbers mean nothing)" % (world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    sharded = world > 1 or args.one_rank_slab_path
    if world == 1 and sharded:   # (a world of one, without torchrun)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if sharded:
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import tsdf_amd
    from tsdf_amd import synth
    import ctypes as C
    from tsdf_amd._capi import check, lib

    check(lib.tsdf_set_device(local_rank))
    n = args.grid
    N_vox = n * n * n
    K, Wu = args.steps, args.warmup
    S_spread = K if args.spread_steps <= 0 else max(K, args.spread_steps)   # steps of the per-step timing run (--full)
    n_frames = (S_spread if args.full else K) + Wu + 1       # (+ 1: the last step announces the next frame)
    inside = args.workload == "config4"
    seed = 0x5EED0004 if inside else SEED

    trace("process group / device ready")
    # ---- inputs: synthetic stream, resident in HBM before timing ---------------------------------
    frames, cams = [], []
    if args.tum_dir:
        loaded, size = tsdf_amd.load_tum_directory(args.tum_dir)
        if not loaded or size != (W, H):
            raise SystemExit("bench.py --tum-dir: %d frames of %s in %s (need %dx%d)" % (len(loaded), size, args.tum_dir, W, H))
        for i in range(n_frames):
            frames.append(loaded[i % len(loaded)][0])
            cams.append(loaded[i % len(loaded)][1])
    if not args.tum_dir:
        # each distinct frame of the trajectory is made once, on a few host threads (numpy leaves the GIL in its array loops; a frame
        # depends on its index alone, so the bits are those of one thread)
        from concurrent.futures import ThreadPoolExecutor
        distinct = sorted({i % args.stream_frames for i in range(n_frames)})
        with ThreadPoolExecutor(max_workers=min(8, len(distinct))) as pool_:
            made = dict(zip(distinct, pool_.map(lambda j: synth.depth_frame(j, args.stream_frames, seed=seed, inside=inside), distinct)))
        for i in range(n_frames):
            d, cam = made[i % args.stream_frames]
            frames.append(d)
            cams.append(cam)
    depth_dev = torch.from_numpy(np.stack(frames).view(np.int16)).cuda()           # (F, H*W) uint16 bits
    filt_dev = torch.empty((H * W,), dtype=torch.int16, device="cuda")
    # the bilateral filter leaves the 16 x 16 tile maxima of its output for integrate's brick culling (one launch fewer per frame;
    # --separate-tile-max: integrate computes them itself from the filtered image, as tsdf_integrate_device does)
    n_tiles = ((W + 15) // 16) * ((H + 15) // 16)
    tmax_dev = [torch.empty((n_tiles,), dtype=torch.int16, device="cuda") for _ in range(2)]
    tiles_of = (lambda j: None) if args.separate_tile_max else (lambda j: tmax_dev[j % 2].data_ptr())
    vert_dev = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    norm_dev = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")

    trace("frames synthesised")
    # ---- volume (whole, or this rank's Z-slab) -----------------------------------------------------
    if not sharded:
        vol = tsdf_amd.TSDFVolume((n, n, n), (args.physical,) * 3)
    else:
        from tsdf_amd.multi import balanced_slab_ranges, plane_costs, refine_slab_ranges, slab_range
        hits_probe = torch.empty((H * W, 2), dtype=torch.float32, device="cuda")    # {k, t} records
        bil0 = tsdf_amd.BilateralFilter(30.0, 4.5)
        rc0 = tsdf_amd.GPURaycaster(W, H)
        s0 = torch.cuda.current_stream()

        def build(plan):
            v = tsdf_amd.TSDFVolume((n, n, n), (args.physical,) * 3, slab=tuple(plan[rank]))
            v.set_stream(s0.cuda_stream)
            return v

        def probe(v):
            """seconds this rank's slab needs for integrate + slab ray cast of a stream frame (3 frames in, then 2 timed)."""
            pf = min(5, n_frames)
            for i in range(pf):
                if i == pf - 2:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s0)
                bil0.filter_device(depth_dev[i].data_ptr(), filt_dev.data_ptr(), W, H, bits=16, stream=s0.cuda_stream, tile_max_ptr=tiles_of(0))
                v.integrate_device(filt_dev.data_ptr(), W, H, cams[i], tile_max_ptr=tiles_of(0))
                rc0.raycast_slab_device(v, cams[i], hits_probe.data_ptr())
            e1.record(s0)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / 2.0

        def gathered(x):
            t = torch.tensor([x], dtype=torch.float64)
            allt = torch.empty((world,), dtype=torch.float64)
            if share:
                dist.all_gather_into_tensor(allt, t)
            else:
                tg, ag = t.cuda(), allt.cuda()
                dist.all_gather_into_tensor(ag, tg)
                allt = ag.cpu()
            return [float(v) for v in allt.tolist()]

        slab_plan = [slab_range(n, world, r) for r in range(world)]
        plan_log = []
        vol = None
        if args.slab_plan == "model":
            # boundaries from a work estimate: a 128-plane planner volume integrates three frames of the stream and says where
            # the updated voxels and the occupied ray-caster bricks are (every rank computes the same plan)
            pick = sorted({0, (Wu + K) // 2, Wu + K - 1})
            costs = plane_costs(lambda g: tsdf_amd.TSDFVolume(g, (args.physical,) * 3), [frames[i] for i in pick], [cams[i] for i in pick], (n, n, n))
            slab_plan = balanced_slab_ranges(costs, world, min_planes=8)
        elif args.slab_plan == "measured":
            # contiguous Z-slabs whose boundaries even out the MEASURED work (still north_star's split, only the cuts move):
            # every rank times integrate + slab cast of its slab on the first frames, the times are all-gathered, each rank's
            # time above the common floor is spread over its planes and the density is re-cut; the best of the plans tried stays
            best = None
            for rnd in range(args.plan_rounds + 1):
                v = build(slab_plan)
                secs = gathered(probe(v))
                plan_log.append({"planes": [int(b_ - a_) for a_, b_ in slab_plan], "ms": [round(x * 1e3, 4) for x in secs]})
                if best is None or max(secs) < best[0]:
                    if best is not None and best[2] is not None:
                        best[2].close()
                    best = (max(secs), [tuple(r_) for r_ in slab_plan], v)
                else:
                    v.close()
                if rnd < args.plan_rounds:
                    slab_plan = refine_slab_ranges(slab_plan, secs, n, min_planes=8)
            slab_plan = best[1]
            best[2].close()          # (a fresh volume below: the probe frames must not stay integrated)
        zb, ze = slab_plan[rank]
        vol = tsdf_amd.TSDFVolume((n, n, n), (args.physical,) * 3, slab=(zb, ze))
        # the frame's collective on the step's own stream (RCCL called directly by the C++ library: tsdf_slab_exchange); torch's
        # collective, through the same object's callback form, if that cannot be set up
        from tsdf_amd.multi import SlabExchange

        def torch_all_gather(mine, allr, stream_ptr):
            on = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.default_stream()
            if share:   # gloo: staged through the host
                h_all = torch.empty(allr.shape, dtype=allr.dtype)
                on.synchronize()
                dist.all_gather_into_tensor(h_all, mine.cpu())
                with torch.cuda.stream(on):
                    allr.copy_(h_all)
            else:
                with torch.cuda.stream(on):     # (torch orders the process group's stream against the current stream)
                    dist.all_gather_into_tensor(allr, mine)

        exch, exch_note = None, "torch.distributed.all_gather_into_tensor (gloo, staged through the host)" if share else "torch.distributed.all_gather_into_tensor"
        if not share and not args.torch_collective:
            try:
                exch = SlabExchange()
                exch_note = "ncclAllGather on the step's stream (tsdf_slab_exchange: librccl, own communicator)"
            except Exception as e_:      # (every rank takes the same branch: the failure modes are a missing library or symbol)
                exch_note += " (direct RCCL unavailable: %s)" % e_
        if exch is None:
            exch = SlabExchange(callback=torch_all_gather)
    stream = torch.cuda.current_stream()
    vol.set_stream(stream.cuda_stream)
    bil = tsdf_amd.BilateralFilter(30.0, 4.5)
    rc = tsdf_amd.GPURaycaster(W, H)
    # The step runs through tsdf_pipeline_step (C++ behind the C ABI, tsdf_amd/csrc/pipeline.hip; tsdf_amd.pipeline.FusionPipeline is
    # its ctypes mirror) -- filter, integrate, ray cast + normals on one stream, and the NEXT
    # frame's filter and brick culling (they depend on nothing before them; the stream's poses are given, as in BASELINE
    # configs[2]) on a second stream of lower priority, released when this frame's integrate is done: they fill the ramp-downs
    # and the latency-bound small kernels of the ray cast (--no-overlap: strictly one after the other).  N > 1: the ray cast is
    # the rank's slab cast, the frame's all-gather and the merge of the ranks' records, all on the step's stream.  Every timed
    # step holds one filter, one integrate, one ray cast (one exchange).
    from tsdf_amd.pipeline import FusionPipeline

    overlap = not args.no_overlap
    pipe = FusionPipeline(vol, bil, rc, W, H, overlap=overlap, exchange=exch if sharded else None,
                          exchange_stream=os.environ.get("TSDF_PIPE_EXCHANGE_STREAM") == "1",
                          tighten_ahead=os.environ.get("TSDF_PIPE_NO_TIGHTEN_AHEAD") != "1")
    stream = pipe.main          # (the volume's stream now)
    if sharded:                 # the pipeline's record buffers, for the stage-by-stage replay
        from tsdf_amd.multi import device_words
        mine_ptr, all_ptr = pipe.hit_buffers()
        hits_mine, hits_all = device_words(mine_ptr, 2 * H * W), device_words(all_ptr, 2 * H * W * world)

    def exchange_hits(on):
        exch.all_gather(hits_mine, hits_all, on.cuda_stream)

    trace("volume and slab plan ready")
    stage_names = ["bilateral", "integrate", "raycast", "exchange", "normals"]
    ev = {s: [] for s in stage_names}

    def step(i, timed, timed_next=False):
        """timed: the replay -- one stage after the other on the step's stream, every stage between two events."""
        cam = cams[i]
        if not timed:
            nxt = i + 1 if i + 1 < n_frames else None
            pipe.step(depth_dev[i].data_ptr(), cam, vert_dev.data_ptr(), norm_dev.data_ptr(),
                      depth_dev[nxt].data_ptr() if nxt is not None else None, cams[nxt] if nxt is not None else None)
            return
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record(stream)
        bil.filter_device(depth_dev[i].data_ptr(), filt_dev.data_ptr(), W, H, bits=16, stream=stream.cuda_stream, tile_max_ptr=tiles_of(0))
        e[1].record(stream)
        vol.integrate_device(filt_dev.data_ptr(), W, H, cam, tile_max_ptr=tiles_of(0))
        e[2].record(stream)
        if not sharded:
            rc.raycast_device(vol, cam, vert_dev.data_ptr(), None if os.environ.get('BENCH_SPLIT_NORMALS') else norm_dev.data_ptr())   # vertices and normals in one go
            e[3].record(stream)
        else:
            rc.raycast_slab_device(vol, cam, hits_mine.data_ptr())
            e[3].record(stream)
            exchange_hits(stream)
            tsdf_amd.merge_hits_normals_device(vol, hits_all.data_ptr(), world, W, H, cam, vert_dev.data_ptr(), norm_dev.data_ptr(), stream.cuda_stream)   # merged vertices and their normals in one go
        e[4].record(stream)
        if os.environ.get('BENCH_SPLIT_NORMALS'):    # (the ray cast, or the merge of the slabs' records, has formed the normals with the vertices)
            tsdf_amd.compute_normals_device(W, H, vert_dev.data_ptr(), norm_dev.data_ptr(), stream.cuda_stream)
        e[5].record(stream)
        ev["bilateral"].append((e[0], e[1]))
        ev["integrate"].append((e[1], e[2]))
        ev["raycast"].append((e[2], e[3]))
        ev["exchange"].append((e[3], e[4]))
        ev["normals"].append((e[4], e[5]))

    def barrier():
        if sharded:
            dist.barrier()

    # The replays below record ~13 events per step; the HIP runtime grows its pool of signals in steps of a few hundred events, and
    # the step that triggers a growth waits ~25 ms for it (seen as one 24.8 ms ray cast among 0.19 ms ones at --steps 40).  Grow it
    # now, outside every measured interval.
    pool = [torch.cuda.Event(enable_timing=True) for _ in range(max(1024, 20 * (K + Wu)))]
    for e_ in pool:
        e_.record(stream)
    torch.cuda.synchronize()
    del pool

    trace("event pool grown")
    # ---- warmup, then the timed region; R times, each on a freshly cleared volume fed the same frames (the spread is the box's noise,
    # not a different workload) --------------------------------------------------------------------------
    period = args.event_period if args.event_period > 0 else 0
    R = max(1, args.repeats)
    runs, run_bits = [], []
    for rep in range(R):
        if rep:
            vol.clear()
        for i in range(Wu):
            step(i, False)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(Wu, Wu + K):
            step(i, period > 0 and (i - Wu) % period == 0, period > 0 and (i + 1 - Wu) % period == 0 and i + 1 < Wu + K)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        elapsed_r = time.perf_counter() - t0
        if sharded:
            t = torch.tensor([elapsed_r], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed_r = float(t.item())
        runs.append(elapsed_r)
        # order-independent, exact: the sum of the 32-bit patterns of every word of the maps, as signed integers (what tools/kinfu_stream.cpp prints)
        run_bits.append((int(vert_dev.view(torch.int32).to(torch.int64).sum().item()), int(norm_dev.view(torch.int32).to(torch.int64).sum().item())))
    elapsed = float(np.median(runs))
    checksum = float(torch.nan_to_num(vert_dev.double(), nan=0.0).sum().item())   # the picture of the last timed frame
    last_vertices = vert_dev.clone()
    bits_v, bits_n = run_bits[-1]
    if args.dump_outputs and rank == 0:      # (before the legs below reuse the maps and the volume)
        dump_outputs(args.dump_outputs, vert_dev, norm_dev, None if sharded else vol)
    ms_per_step = elapsed * 1e3 / K
    value = N_vox * K / elapsed / 1e6

    out = {
        "metric": "Mvoxels/s integrate + Mrays/s raycast, 512^3 grid, 640x480 depth; 1/2/4/8 GPU",
        "value": round(value, 3),
        "unit": "Mvoxels/s",
        "value_definition": "grid voxels pushed through the whole step (bilateral+integrate+raycast+normals) per second",
        "n_gpus": world,
        "steps": K,
        "warmup": Wu,
        "event_period": period,     # HIP events inside the timed region on every n-th step (0 = none)
        "ms_per_step": round(ms_per_step, 4),
        "ms_per_step_is": "median of %d timed regions of %d steps, each on a freshly cleared volume fed the same %d warm-up + %d timed frames" % (R, K, Wu, K),
        "ms_per_step_runs": [round(r_ * 1e3 / K, 4) for r_ in runs],
        "picture_bits_equal_across_runs": bool(all(b_ == run_bits[0] for b_ in run_bits)),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "configs[%d]: %d^3 TSDF over %.0f mm, synthetic TUM-surrogate stream (%d-frame "
                               "trajectory%s, seed 0x%X), 640x480 uint16 depth, bilateral(30,4.5) + integrate + "
                               "raycast + normals per frame" % (3 if inside else 2, n, args.physical, args.stream_frames,
                                                                " inside the volume" if inside else "", seed),
                   "grid": [n, n, n], "image": [W, H], "parallelism": "zslab%d" % world,
                   "overlap": ("bilateral + brick culling of frame i+1 on a lower-priority stream during the ray cast of frame i (tsdf_pipeline_step, C++)"
                               if pipe.overlap else "none"),
                   "depth_tile_maxima": "integrate's own launch" if args.separate_tile_max else "left by the bilateral filter's launch",
                   "collective_backend": (dist.get_backend() if sharded else None), "ranks": (dist.get_world_size() if sharded else 1),
                   "collective": (exch_note if sharded else None)},
        # sum of the finite vertex coordinates of the last frame's picture: equal between runs that differ only in schedule
        "last_frame_vertex_checksum": checksum,
        "last_frame_vertex_bits": bits_v, "last_frame_normal_bits": bits_n,
        "stream": ("TUM directory %s through TUMDataLoader" % args.tum_dir) if args.tum_dir else "synthesised in memory (tsdf_amd/synth.py)",
        "full": args.full,          # false: the headline alone; --full adds the replays, the roofline, the legs and the checks below
    }
    if sharded and rank == 0:
        out["slabs"] = [list(r_) for r_ in slab_plan]
        out["slab_plan"] = {"method": args.slab_plan, "rounds": plan_log}

    trace("timed region done")
    if not args.full:
        finish(out, rank, sharded, pipe, exch if sharded else None, json_fd)
        return
    # ---- untimed replays of the SAME K frames: (1) every stage and every launch of the dominant kernels bracketed with HIP
    # events on the launch stream (K launches timed, none of their cost inside `value`); (2) the voxels each frame updates,
    # counted by the kernel (which voxels a frame updates does not depend on the volume's state: depth > 0 and sdf >= -trunc,
    # src/TSDF/TSDFVolume.cu:355,366 -- so the byte model prices exactly the launches that were timed)
    for s_ in stage_names:
        ev[s_].clear()
    vol.clear()                    # the replay starts from the state the timed regions started from: cleared + the warm-up frames
    for i in range(Wu):
        step(i, False)
    torch.cuda.synchronize()
    vol.set_timing(1)
    for i in range(Wu, Wu + K):
        step(i, True, True)
    torch.cuda.synchronize()
    # (mean over the K replayed steps; a step in which the runtime stalls for tens of milliseconds -- it grows its pools of signals
    # now and then, see above -- is not the stage's time: values beyond 20 x the median are left out and counted)
    stage_outliers = 0

    def stage_mean(pairs):
        nonlocal stage_outliers
        v = np.array([a.elapsed_time(b) for a, b in pairs], np.float64)
        keep = v <= 20.0 * max(float(np.median(v)), 1e-4)
        stage_outliers += int((~keep).sum())
        return float(v[keep].mean())
    stage_ms = {s_: (stage_mean(ev[s_]) if ev[s_] else None) for s_ in stage_names}
    if os.environ.get("BENCH_DEBUG_STAGES"):
        print("raycast stage per step:", [round(a.elapsed_time(b), 3) for a, b in ev["raycast"]], file=sys.stderr)
    kern = {w: vol.kernel_time(w) for w in ("integrate", "raycast", "raycast_tail")}     # (launches, avg ms), kernel only
    vol.set_timing(False)
    vol.set_counting(True)
    U_frames = []
    for i in range(Wu, Wu + K):
        bil.filter_device(depth_dev[i].data_ptr(), filt_dev.data_ptr(), W, H, bits=16, stream=stream.cuda_stream, tile_max_ptr=tiles_of(0))
        vol.integrate_device(filt_dev.data_ptr(), W, H, cams[i], tile_max_ptr=tiles_of(0))
        torch.cuda.synchronize()
        U_frames.append(vol.last_updated_voxels())
    vol.set_counting(False)
    # ---- the same K frames once more with ONE event behind every step (pipelined as in the timed regions; an event costs a few us of
    # stream time, so these are not `value`): what the worst step of the stream costs beside the median -- the periodic rebuild of the
    # ray caster's flags, a widening of the weight storage
    vol.clear()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(S_spread + 1)]
    for m_ in marks:          # (every event recorded once before it counts: the runtime makes an event's signal at its first record, and grows
        m_.record(stream)     # its pool of signals a few hundred at a time -- a stall of 0.1 ms that landed in the first timed step)
    torch.cuda.synchronize()
    for i in range(Wu):       # (the warm-up frames and the timed ones in one go: a stream drained in front of the first timed step would
        step(i, False)        # charge it the host's launch latency -- 0.03 ms that is start-up, not jitter of the stream)
    marks[0].record(stream)
    kinds = []
    for i in range(Wu, Wu + S_spread):
        step(i, False)
        marks[i - Wu + 1].record(stream)
        kinds.append(bool(vol.last_raycast_cell_parallel()) if not sharded else None)   # (a host-side flag of the call just made: nothing waits)
    torch.cuda.synchronize()
    per_step = np.array([marks[i].elapsed_time(marks[i + 1]) for i in range(S_spread)], np.float64)
    worst = np.argsort(per_step)[::-1][:5]
    step_spread = {"median": round(float(np.median(per_step)), 4), "p95": round(float(np.percentile(per_step, 95)), 4),
                   "max": round(float(per_step.max()), 4), "max_over_median": round(float(per_step.max() / np.median(per_step)), 3),
                   "steps": S_spread, "worst_steps": [[int(j), round(float(per_step[j]), 4)] for j in worst],
                   "how": "an event behind every pipelined step of one more run: the %d timed frames%s" % (K, " and the %d that follow them in the stream" % (S_spread - K) if S_spread > K else "")}
    if not sharded:
        # steps whose cast was not the kind most steps took: the chooser's trials of the other cast (raycast.hip: choose_cast -- one after
        # 32 casts, then every 64 ... 4096 where the other cast could win at all): slow steps by design, listed apart
        usual = sum(kinds) * 2 >= len(kinds)
        trials = [j for j, k_ in enumerate(kinds) if k_ != usual]
        rest = np.array([per_step[j] for j in range(S_spread) if j not in trials], np.float64)
        step_spread["cast_kind"] = "cell-parallel" if usual else "march"
        step_spread["chooser_trial_steps"] = trials
        step_spread["max_over_median_without_trials"] = round(float(rest.max() / np.median(rest)), 3) if len(rest) else None
    if os.environ.get("BENCH_DEBUG_STEPS"):
        print("per step ms:", [round(float(x), 4) for x in per_step], file=sys.stderr)
    if S_spread > K:   # (the legs below run on the volume as the K timed frames leave it)
        vol.clear()
    # ---- and once more, pipelined, with the dominant kernels' launches carrying their dispatches' own begin / end timestamps: the kernels
    # as they run in the two-stream step -- the cast beside the next frame's filter and culling: what a rocprofv3 kernel trace of this
    # command sees (profiles/*_kernel_stats.txt) -- beside `avg_launch_ms`, each kernel with nothing beside it
    vol.clear()
    for i in range(Wu):
        step(i, False)
    torch.cuda.synchronize()
    vol.set_timing(1)
    for i in range(Wu, Wu + K):
        step(i, False)
    torch.cuda.synchronize()
    kern_pipelined = {w: vol.kernel_time(w) for w in ("integrate", "raycast", "raycast_tail")}
    vol.set_timing(False)
    # ---- integrate under each way the weights can be stored (weights.hip): 8-bit counts (what the timed frames run on), 16-bit counts
    # (a voxel updated more than 255 times), the reference's fp32 array (after weight_data() / beyond 65535): same frames, same bits
    int_by_storage = {}
    if not sharded:
        for bits in (8, 16, 32):
            vol.clear()
            if vol.weight_storage()[0] <= bits:
                vol.set_weight_storage(bits)
            for i in range(Wu):
                step(i, False)
            torch.cuda.synchronize()
            vol.set_timing(1)
            for i in range(Wu, Wu + K):
                bil.filter_device(depth_dev[i].data_ptr(), filt_dev.data_ptr(), W, H, bits=16, stream=stream.cuda_stream, tile_max_ptr=tiles_of(0))
                vol.integrate_device(filt_dev.data_ptr(), W, H, cams[i], tile_max_ptr=tiles_of(0))
            torch.cuda.synchronize()
            int_by_storage[str(vol.weight_storage()[0])] = round(vol.kernel_time("integrate")[1], 4)
            vol.set_timing(False)
        vol.clear()   # (back to the starting storage for the legs below)
        for i in range(Wu + K):
            step(i, False)
        torch.cuda.synchronize()
    out.update({
        "stage_and_kernel_times_from": "untimed replay of the %d timed frames from the same volume state (cleared + the warm-up frames), one stage "
                                       "after the other (no overlap), every launch bracketed with HIP events on the launch stream" % K,
        "ms_per_step_max": step_spread["max"], "ms_per_step_p95": step_spread["p95"], "step_ms_spread": step_spread,
        "integrate_ms_by_weight_storage": int_by_storage or None,
        "integrate_mvoxels_per_s": round(N_vox / (stage_ms["integrate"] * 1e-3) / 1e6, 1),
        "raycast_mrays_per_s": round(W * H / ((stage_ms["raycast"] + stage_ms["exchange"] + stage_ms["normals"]) * 1e-3) / 1e6, 2),
        "stage_ms": {s: (round(v, 4) if v is not None else None) for s, v in stage_ms.items()},
        "stage_outliers_dropped": stage_outliers,
    })

    trace("replays done")
    # ---- roofline of the dominant kernel (by time): HIP-event durations of the replay, bytes of the same launches ----------
    last = Wu + K                                  # one more frame (untimed legs below)
    U = int(round(float(np.mean(U_frames))))       # voxels updated per launch, mean over the K timed frames (this rank's slab)
    int_bytes = 16 * U + 2 * W * H                 # 16*U + depth frame
    int_ms = kern["integrate"][1] or stage_ms["integrate"]
    int_gbs = int_bytes / (int_ms * 1e-3) / 1e9
    traffic, traffic_meta, activity = load_traffic(args)
    # How the weights are stored decides which kernel ran and what it moves per updated voxel: the algorithmic figure stays SURVEY 8d's
    # (the reference's two fp32 arrays read and written: 16 B); with weights kept as 8- / 16-bit counts the kernel moves 10 / 12 B.
    wbits = vol.weight_storage()[0]
    int_kernel = "integrate_kernel" if wbits == 32 else "integrate_packed_kernel"
    moved_per_voxel = {32: 16, 16: 12, 8: 10}[wbits]
    roof_int = {"kernel": int_kernel, "bound": "hbm", "achieved": round(int_gbs, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(int_gbs / HBM_PEAK_GBS, 5), "traffic": traffic.get(int_kernel),
                "algorithmic_bytes": int_bytes, "avg_launch_ms": round(int_ms, 4), "launches_timed": kern["integrate"][0],
                "avg_launch_ms_pipelined": round(kern_pipelined["integrate"][1], 4),
                "U_voxels_updated": U, "U_min_max": [int(min(U_frames)), int(max(U_frames))], "dense_bytes": 16 * N_vox,
                "weight_storage_bits": wbits, "bytes_moved_per_updated_voxel": moved_per_voxel,
                "moved_bytes_model": moved_per_voxel * U + 2 * W * H,
                "moved_gbs": round((moved_per_voxel * U + 2 * W * H) / (int_ms * 1e-3) / 1e9, 2)}
    roof_int.update(traffic_meta)
    roof_int.update(activity_of(activity, int_kernel))
    if not sharded:
        st = rc.stats(vol, cams[last - 1])             # S samples, T distinct voxels touched at the end state
        ray_bytes = 4 * st["touched"] + 12 * W * H     # 4*T + vertex store (normals kernel: +12*W*H)
        # the march is two kernels (bulk + tail queue); its bytes are priced against their summed duration.  The
        # stage times also hold the occupancy refresh / merge / cull kernels.
        ray_main_ms, ray_tail_ms = kern["raycast"][1], kern["raycast_tail"][1]
        ray_ms = (ray_main_ms + ray_tail_ms) or stage_ms["raycast"]
        ray_gbs = ray_bytes / (ray_ms * 1e-3) / 1e9
        # dominant = the single kernel with the longest average launch IN THE PIPELINED STEP (what the step waits for: the cast runs
        # beside the next frame's filter and culling there, integrate with nothing beside it); the replay's figures -- each kernel
        # alone -- are what `achieved` / `frac` are priced on, and both are in both objects
        pip_ray = max(kern_pipelined["raycast"][1], kern_pipelined["raycast_tail"][1]) or max(ray_main_ms, ray_tail_ms)
        pip_int = kern_pipelined["integrate"][1] or int_ms
        dominant = "raycast" if pip_ray >= pip_int else "integrate"
        cells = vol.last_raycast_cell_parallel()     # which kernels the casts took: scheduling only, the same bits either way
        ray_names = ("cast_cells_kernel", None) if cells else ("process_ray_kernel", "process_ray_tail_kernel")
        roof_ray = {"kernel": "cast_cells_kernel" if cells else "process_ray_kernel + process_ray_tail_kernel",
                    "cast": ("cell-parallel: one wave per flagged brick, every (mixed cell, pixel) pair's samples inside the cell; no ray is marched (raycast_cells.hpp)"
                             if cells else "march: sample ranges with a pass budget + the queue of unfinished stretches"),
                    "bound": "hbm", "achieved": round(ray_gbs, 2), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(ray_gbs / HBM_PEAK_GBS, 5), "traffic": (traffic.get(ray_names[0], 0) + (traffic.get(ray_names[1], 0) if ray_names[1] else 0)) or None,
                    "algorithmic_bytes": ray_bytes, "avg_launch_ms": round(ray_ms, 4), "launches_timed": kern["raycast"][0],
                    "avg_launch_ms_pipelined": round(kern_pipelined["raycast"][1] + kern_pipelined["raycast_tail"][1], 4),
                    "avg_launch_ms_is": "the kernel with nothing beside it (replay, one stage after the other); _pipelined: in the two-stream step, beside the next frame's filter and culling -- what a kernel trace of this command shows",
                    "avg_launch_ms_by_kernel": ({"cast_cells_kernel": round(ray_main_ms, 4)} if cells else
                                                {"process_ray_kernel": round(ray_main_ms, 4), "process_ray_tail_kernel": round(ray_tail_ms, 4)}),
                    "T_voxels_touched": st["touched"], "S_samples": st["samples"],
                    "samples_evaluated_after_exact_skipping": st["evaluated"],
                    "msamples_per_s": round(st["samples"] / (ray_ms * 1e-3) / 1e6, 1),
                    "l2_level_gbs": round(32 * st["samples"] / (ray_ms * 1e-3) / 1e9, 1)}
        roof_ray.update(traffic_meta)
        roof_ray.update(activity_of(activity, ray_names[0]))
    if rank == 0:
        # the fraction against the measured device-to-device copy rate (float4 copy kernel of the library, 1 GiB,
        # best of 5, on the launch stream) as well as the nominal peak
        gbs = C.c_double(0.0)
        check(lib.tsdf_measure_copy_bandwidth(1 << 30, 5, C.c_void_p(stream.cuda_stream), C.byref(gbs)))
        copy_gbs = float(gbs.value)
        # ... and against what integrate's own memory walk reaches when it does nothing but the in-place update of every voxel
        # (read-modify-write of both arrays, brick by brick, no projection): the ceiling of the access shape
        check(lib.tsdf_measure_update_bandwidth(5, C.c_void_p(stream.cuda_stream), C.byref(gbs)))
        update_gbs = float(gbs.value)
        for r_ in ([roof_int] if sharded else [roof_ray, roof_int]):
            r_["measured_copy_gbs"] = round(copy_gbs, 1)
            r_["frac_of_measured_copy"] = round(r_["achieved"] / copy_gbs, 5)
        roof_int["measured_inplace_update_gbs"] = round(update_gbs, 1)
        # (the walk moves what it touches: it is compared with the bytes the kernel MOVES, not with SURVEY 8d's 16 B per voxel)
        roof_int["moved_frac_of_inplace_update"] = round(roof_int["moved_gbs"] / update_gbs, 5)
    if rank == 0 and not sharded:
        out["roofline"] = roof_ray if dominant == "raycast" else roof_int
        out["roofline_other"] = roof_int if dominant == "raycast" else roof_ray
        out["roofline"]["dominant_by"] = "the longest average launch in the pipelined step: %s %.4f ms, %s %.4f ms" % (
            roof_ray["kernel"].split(" ")[0], pip_ray, int_kernel, pip_int)
        if not args.path_only:
            out["host_buffer_api"] = host_api_time(vol, bil, frames, cams, last)
            out["icp"] = icp_tracking(tsdf_amd, synth, depth_dev, frames, stream, not args.no_cpu_baseline)
            out["tracking"] = tracking_loop(tsdf_amd, synth, n, args.physical, args.stream_frames)
        if not args.no_parity:
            out["parity"] = parity_gate(tsdf_amd, frames, cams, args.parity_grid or n, args.physical, Wu, K)
            out["parity"]["note"] = ("GPU vs oracle, bit for bit.  The oracle's integrate / ray-cast legs are a line-by-line restatement "
                                     "(the reference holds no vectors for them: parity unpinned); the 16-bit bilateral follows semantics "
                                     "defined here (the reference's 16-bit path is undefined behaviour), its 8-bit path is pinned on the "
                                     "reference compiled natively")
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(vol, frames[last], cams[last], n, args.physical, args.cpu_budget_s)
    trace("single-GPU extras done")
    if sharded:
        # every rank's stage and kernel times (the step waits for the slowest), and a parity flag: rank 0 replays the whole
        # stream on ONE volume and compares the merged picture of the last timed frame with it, bit for bit
        mine = torch.tensor([stage_ms[s_] or 0.0 for s_ in stage_names] + [kern["integrate"][1], kern["raycast"][1], kern["raycast_tail"][1], float(U)],
                            dtype=torch.float64, device="cuda")
        allr = torch.empty((world, mine.numel()), dtype=torch.float64, device="cuda")
        if share:
            h_all = torch.empty(allr.shape, dtype=allr.dtype)
            dist.all_gather_into_tensor(h_all.view(-1), mine.cpu())
            allr.copy_(h_all)
        else:
            dist.all_gather_into_tensor(allr.view(-1), mine)
        if rank == 0:
            names = stage_names + ["integrate_kernel", "process_ray_kernel", "process_ray_tail_kernel", "U_voxels_updated"]
            out["per_rank_ms"] = {nm: [round(float(v), 4) for v in allr[:, j].tolist()] for j, nm in enumerate(names)}
            out["roofline"] = roof_int
            out["roofline"]["note"] = "rank 0's slab"
            if not args.no_parity:
                whole = tsdf_amd.TSDFVolume((n, n, n), (args.physical,) * 3)
                whole.set_stream(stream.cuda_stream)
                ref_v = torch.empty_like(vert_dev)
                for i in range(Wu + K):
                    bil.filter_device(depth_dev[i].data_ptr(), filt_dev.data_ptr(), W, H, bits=16, stream=stream.cuda_stream)
                    whole.integrate_device(filt_dev.data_ptr(), W, H, cams[i])
                rc.raycast_device(whole, cams[Wu + K - 1], ref_v.data_ptr(), None)
                torch.cuda.synchronize()
                a_, b_ = last_vertices.view(torch.int32), ref_v.view(torch.int32)
                same = bool(((a_ == b_) | (torch.isnan(last_vertices) & torch.isnan(ref_v))).all().item())
                out["parity"] = {"merged_picture_equals_single_volume_replay": same, "frames": Wu + K,
                                 "hits": int((~torch.isnan(ref_v[:, 0])).sum().item()), "pass": same}
                whole.close()

    if sharded:
        # what the communicator itself says (ncclCommCount), so that a run of one rank is not read as a scaling point
        coll = {"ranks_seen": exch.ranks_seen(), "world": world, "how": exch_note}
        if args.validate_merge:
            # mode B: the merged picture of the last pipelined step (volume = cleared + the warm-up and timed frames) against the
            # ordinary cast of the all-gathered distance slabs, on every rank
            torch.cuda.synchronize()
            barrier()
            n_diff = exch.validate_merge(vol, W, H, cams[Wu + K - 1], vert_dev, norm_dev)
            t = torch.tensor([n_diff], dtype=torch.int64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            coll["validate_merge"] = {"mode": "B: all-gather of the distance slabs + the whole volume's ordinary cast on every rank",
                                      "differing_words_max_over_ranks": int(t.item()), "pass": int(t.item()) == 0}
        if rank == 0:
            out["collective"] = coll
    trace("parity replay done")
    finish(out, rank, sharded, pipe, exch if sharded else None, json_fd)


def finish(out, rank, sharded, pipe, exch, json_fd):
    """Rank 0 prints the line on the saved stdout; N > 1: every rank leaves the process group together."""
    if rank == 0:
        def finite(o):      # strict JSON: a non-finite number (an unsampled average, an empty ratio) becomes null
            if isinstance(o, float):
                return o if math.isfinite(o) else None
            if isinstance(o, dict):
                return {k: finite(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return [finite(v) for v in o]
            return o
        os.write(json_fd, (json.dumps(finite(out), allow_nan=False) + "\n").encode())
    if sharded:
        import torch.distributed as dist
        dist.barrier()
        pipe.close()
        if exch is not None:
            exch.close()
        dist.destroy_process_group()


DUMP_SAMPLE = 1 << 21      # voxels of the volume sample --dump-outputs writes (8 MB per array)
DUMP_SEED = 0x5EED00D0


def dump_outputs(d, vert_dev, norm_dev, vol):
    """--dump-outputs: the last timed step's vertex and normal maps and, for one volume, its distances and weights at a fixed
    seeded sample of voxels (the same voxels for the same grid) -- 26 MB in all at 512^3.  Every value written is finite: a map's
    NaNs (no hit, no normal) become 0 and its pixels are told apart by <map>_valid (1 = all three components finite, 0 = not)."""
    os.makedirs(d, exist_ok=True)
    out = {}
    for name, valid_name, m in (("vertices", "vertex_valid", vert_dev), ("normals", "normal_valid", norm_dev)):
        a = m.cpu().numpy()
        ok = np.isfinite(a)
        out[name] = np.where(ok, a, np.float32(0.0))
        out[valid_name] = ok.all(axis=1)
    if vol is not None:
        n = vol.resident_voxels()
        pick = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=min(n, DUMP_SAMPLE), replace=False))
        out["distance_sample"] = vol.get_distance_data()[pick]
        out["weight_sample"] = vol.get_weight_data()[pick]
    for name, a in out.items():
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a, np.float32))


def host_api_time(vol, bil, frames, cams, last):
    """End-to-end time of the reference-shaped blocking calls on HOST buffers (PCIe inclusive): BilateralFilter::filter,
    TSDFVolume::integrate (614 KB up), TSDFVolume::raycast (2 x 3.7 MB down).  Reported beside the resident-in-HBM value,
    never as `value`."""
    reps = 5
    t = {"bilateral": 0.0, "integrate": 0.0, "raycast": 0.0}
    for r in range(reps + 1):
        f = frames[last].copy()
        t0 = time.perf_counter()
        bil.filter(f, W, H)
        t1 = time.perf_counter()
        vol.integrate(f, W, H, cams[last])
        t2 = time.perf_counter()
        vol.raycast(W, H, cams[last])
        t3 = time.perf_counter()
        if r > 0:   # first round warms the staging buffers
            t["bilateral"] += t1 - t0
            t["integrate"] += t2 - t1
            t["raycast"] += t3 - t2
    res = {k: round(v * 1e3 / reps, 4) for k, v in t.items()}
    res["ms_per_frame"] = round(sum(res.values()), 4)
    return res


def icp_tracking(tsdf_amd, synth, depth_dev, frames, stream, with_cpu):
    """Next-row measurement (BASELINE config 5): ICP tracking between two consecutive bilateral-filtered
    frames of the stream -- both pyramids (initICPModel + initICP) and the 19 Gauss-Newton iterations of
    getIncrementalTransformation, device resident.  Not part of `value`.  The oracle's ICP on one host thread beside it."""
    import torch
    bil = tsdf_amd.BilateralFilter(30.0, 4.5)
    a = torch.empty((H * W,), dtype=torch.int16, device="cuda")
    b = torch.empty((H * W,), dtype=torch.int16, device="cuda")
    bil.filter_device(depth_dev[0].data_ptr(), a.data_ptr(), W, H, bits=16, stream=stream.cuda_stream)
    bil.filter_device(depth_dev[1].data_ptr(), b.data_ptr(), W, H, bits=16, stream=stream.cuda_stream)
    icp = tsdf_amd.ICPOdometry(W, H, 331.0, 234.6, 591.1, 590.1)
    icp.set_stream(stream.cuda_stream)
    reps = 20
    for r in range(reps + 3):
        if r == 3:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        icp.init_icp_device(a.data_ptr(), model=True)
        icp.init_icp_device(b.data_ptr())
        T = icp.get_incremental_transformation()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    res = {"ms_per_frame": round(ms, 4), "iterations": [4, 5, 10], "inliers": icp.last_inliers,
           "what": "initICPModel + initICP + getIncrementalTransformation, 640x480, 3 levels"}
    if with_cpu:
        import oracle as O
        fa = a.cpu().numpy().view(np.uint16)
        fb = b.cpu().numpy().view(np.uint16)
        t0 = time.perf_counter()
        To, _, inl = O.icp_incremental_transformation(fb, fa, W, H, 331.0, 234.6, 591.1, 590.1)
        res["cpu_oracle_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["cpu_cores"] = 1
        res["max_abs_pose_difference_vs_oracle"] = float(np.max(np.abs(T - To)))
    return res


def tracking_loop(tsdf_amd, synth, n, physical, stream_frames, n_frames=24):
    """BASELINE configs[4] without the mesh: the closed loop (filter, render the model from the previous pose, ICP,
    integrate) on a fresh volume of the bench size, poses from tracking instead of ground truth.  Reported beside `value`:
    time per frame and how far the tracked trajectory strays from the true one."""
    import torch
    from tsdf_amd.tracking import FrameToModelTracker
    vol = tsdf_amd.TSDFVolume((n, n, n), (physical,) * 3)
    tracker = FrameToModelTracker(vol, W, H, overlap=os.environ.get("TSDF_TRACK_NO_OVERLAP") != "1")
    frames = [synth.depth_frame(i, stream_frames, seed=SEED) for i in range(n_frames)]
    dev = [torch.from_numpy(d.view(np.int16)).cuda() for d, _ in frames]
    worst_t = worst_r = 0.0
    t0 = None
    for i, (d, cam) in enumerate(frames):
        truth = cam.pose().astype(np.float64).reshape(4, 4).T
        if i == 4:                      # the first frames also build the occupancy flags / allocate scratch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        pose = tracker.process_device(dev[i].data_ptr(), initial_pose=truth if i == 0 else None)
        worst_t = max(worst_t, float(np.linalg.norm(pose[:3, 3] - truth[:3, 3])))
        c = (np.trace(pose[:3, :3].T @ truth[:3, :3]) - 1.0) / 2.0
        worst_r = max(worst_r, float(np.arccos(np.clip(c, -1.0, 1.0))))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / (n_frames - 4)
    # ... and the mesh of the tracked model: extract_surface = marching cubes on the device (vertices to the host), beside
    # the host implementation on the downloaded distances (the same vertices, bit for bit: tests/test_parity_marching_cubes.py)
    t1 = time.perf_counter()
    mesh_dev = vol.extract_surface()
    t1b = time.perf_counter()
    dist_host = vol.get_distance_data()
    t2 = time.perf_counter()
    mesh = tsdf_amd.marching_cubes(dist_host, (n, n, n), (physical / n,) * 3)
    t3 = time.perf_counter()
    return {"ms_per_frame": round(ms, 4),
            "mesh": {"extract_surface_device_s": round(t1b - t1, 4), "same_as_host": bool(mesh_dev.shape == mesh.shape and np.array_equal(mesh_dev.view(np.uint32), mesh.view(np.uint32))), "host_download_s": round(t2 - t1b, 3), "host_marching_cubes_s": round(t3 - t2, 3), "triangles": int(mesh.shape[0] // 3)}, "frames": n_frames, "max_translation_error_mm": round(worst_t, 3),
            "max_rotation_error_rad": round(worst_r, 6),
            "what": "bilateral + raycast(prev pose) + render depth + ICP (3 levels, 19 iterations) + integrate per frame (tsdf_tracker_*: the new "
                    "frame's filter and ICP maps on a second stream beside the model ray cast)"}


def kernel_source_sha():
    """SHA-256 over the kernel sources: a committed counter profile only speaks for the code it was taken on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "tsdf_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def load_traffic(args):
    """HBM bytes per launch from the PMC passes (profiles/traffic*.json, written by tools/profile_round.sh from separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same command, averaged over the K timed launches only).  The counters
    cannot be read inside this process, so the figure is reported only when a profile was taken on the same kernel sources
    with the same --steps / --warmup / --grid (one file per profiled configuration); otherwise `traffic` is null and the reason
    is stated."""
    import glob
    meta = {"traffic_source": None}
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "traffic*.json")))
    if not files:
        meta["traffic_note"] = "no counter profile committed"
        return {}, meta, {}
    want = {"steps": args.steps, "warmup": args.warmup, "grid": args.grid, "gpus": args.gpus}
    sha, notes = kernel_source_sha(), []
    for p in files:
        try:
            d = json.load(open(p))
        except Exception:
            notes.append("%s unreadable" % os.path.basename(p))
            continue
        if d.get("bench_args") != want:
            notes.append("%s was taken with %s, this run is %s" % (os.path.basename(p), d.get("bench_args"), want))
            continue
        if d.get("kernel_source_sha") != sha:
            notes.append("%s was taken on other kernel sources (%s)" % (os.path.basename(p), d.get("tag")))
            continue
        meta["traffic_source"] = "profiles/%s (%s: rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, mean over the %d timed launches of the same command)" % (
            os.path.basename(p), d.get("tag"), args.steps)
        return d.get("bytes_per_launch", {}), meta, d.get("activity", {})
    meta["traffic_note"] = "; ".join(notes) + ": not reported"
    return {}, meta, {}


def activity_of(activity, kernel):
    """valu_busy / lanes_active / valu_insts of one kernel from the committed counter pass (tools/rocprof_summary.py activity: one
    rocprofv3 --pmc run of this command on the same kernel sources; null when there is none)."""
    a = activity.get(kernel) or {}
    return {"valu_busy": a.get("valu_busy"), "lanes_active": a.get("lanes_active"), "valu_insts_per_launch": a.get("valu_insts"),
            "counters_are": ("valu_busy = 4 x SQ_ACTIVE_INST_VALU / (launch x 2.4 GHz x 1024 SIMDs), lanes_active = SQ_THREAD_CYCLES_VALU / "
                             "SQ_INSTS_VALU / 64; same profile as `traffic`") if a else None}


def parity_gate(tsdf_amd, frames, cams, n, physical, Wu, K):
    """GPU vs CPU oracle on the BENCHMARKED grid and frames: both replay the warm-up and the K timed frames
    (bilateral -> integrate, host-buffer calls); after the first and after the last timed frame the whole volume is compared bit
    for bit and every 4th image row is ray cast by both.  The oracle is the checker here, nothing it computes is timed or reported
    as a result."""
    import oracle as O
    threads = O.max_threads()
    gv = tsdf_amd.TSDFVolume((n,) * 3, (physical,) * 3)
    ov = O.Volume((n,) * 3, (physical,) * 3)
    bil = tsdf_amd.BilateralFilter(30.0, 4.5)
    row_step = 4
    res = {"grid": n, "frames": Wu + K, "compared_after_frames": [Wu + 1, Wu + K], "ray_rows": "every %dth" % row_step,
           "bilateral_mismatch": 0, "weight_mismatch": 0, "dist_bit_mismatch": 0, "dist_max_rel_err": 0.0,
           "nan_mask_mismatch": 0, "vertex_bit_mismatch": 0, "vertex_max_rel_err": 0.0, "normal_max_abs_err": 0.0, "rays_compared": 0}
    t0 = time.perf_counter()
    for i in range(Wu + K):
        f = frames[i].copy()
        bil.filter(f, W, H)
        fo = O.bilateral_u16(frames[i], W, H, 30.0, 4.5, nthreads=threads).reshape(-1)
        res["bilateral_mismatch"] += int((f != fo).sum())
        gv.integrate(f, W, H, cams[i])
        ov.integrate(fo, W, H, cams[i].inverse_pose(), cams[i].k(), cams[i].kinv(), nthreads=threads)
        if i not in (Wu, Wu + K - 1):
            continue
        gd, gw = gv.get_distance_data(), gv.get_weight_data()
        res["weight_mismatch"] += int((gw != ov.weight).sum())
        res["dist_bit_mismatch"] += int((gd.view(np.uint32) != ov.dist.view(np.uint32)).sum())
        m = ov.weight > 0
        if m.any():
            res["dist_max_rel_err"] = max(res["dist_max_rel_err"], float((np.abs(gd[m] - ov.dist[m]) / np.maximum(np.abs(ov.dist[m]), 1e-6)).max()))
        del gd, gw, m
        V, Nn = gv.raycast(W, H, cams[i])
        Vo, _ = ov.raycast_rows(W, H, cams[i].pose(), cams[i].kinv(), 0, H, row_step, nthreads=threads)
        rows = np.arange(0, H, row_step)
        Vg = V.reshape(H, W, 3)[rows].reshape(-1, 3)
        Vo = np.asarray(Vo, np.float32).reshape(H, W, 3)[rows].reshape(-1, 3)
        res["rays_compared"] += int(Vo.shape[0])
        res["nan_mask_mismatch"] += int((np.isnan(Vg) != np.isnan(Vo)).sum())
        same = (Vg.view(np.uint32) == Vo.view(np.uint32)) | (np.isnan(Vg) & np.isnan(Vo))
        res["vertex_bit_mismatch"] += int((~same).sum())
        ok = ~np.isnan(Vo) & ~np.isnan(Vg)
        if ok.any():
            res["vertex_max_rel_err"] = max(res["vertex_max_rel_err"], float((np.abs(Vg[ok] - Vo[ok]) / np.maximum(np.abs(Vo[ok]), 1e-6)).max()))
        # normals of the compared rows whose lower neighbour row was cast too would need consecutive rows: the oracle's normals of
        # the GPU's own vertex map instead (compute_normals is a function of the vertex map alone, GPURaycaster.cu:393-427)
        No = O.normals(W, H, V)
        okn = np.isfinite(No)
        res["nan_mask_mismatch"] += int((np.isnan(Nn) != np.isnan(No)).sum())
        if okn.any():
            res["normal_max_abs_err"] = max(res["normal_max_abs_err"], float(np.abs(Nn[okn] - No[okn]).max()))
    res["seconds"] = round(time.perf_counter() - t0, 2)
    res["oracle_threads"] = threads
    res["pass_within_1e-4"] = bool(res["weight_mismatch"] == 0 and res["dist_max_rel_err"] <= 1e-4 and res["nan_mask_mismatch"] == 0
                                   and res["vertex_max_rel_err"] <= 1e-4 and res["normal_max_abs_err"] <= 1e-4
                                   and res["bilateral_mismatch"] == 0)
    # the gate is bit for bit: north_star's 1e-4 alone would let a regression of the exact arithmetic through
    res["pass"] = bool(res["pass_within_1e-4"] and res["dist_bit_mismatch"] == 0 and res["vertex_bit_mismatch"] == 0)
    gv.close()
    return res


def cpu_baseline(vol, depth, cam, n, physical, budget_s):
    """The oracle (a port of the reference arithmetic, oracle/tsdf_oracle.c) timed on this box's host cores on a
    bounded sample of the same workload: one frame of bilateral + integrate over the full 512^3 grid and a ray
    cast of every 16th image row against the GPU-built volume state.  Reported only."""
    import oracle as O
    cores = O.max_threads()
    t = time.perf_counter()
    f = O.bilateral_u16(depth, W, H, 30.0, 4.5, nthreads=cores).reshape(-1)
    t_bil = time.perf_counter() - t
    ov = O.Volume((n, n, n), (physical,) * 3)
    ov.set_distance_data(vol.get_distance_data())
    ov.set_weight_data(vol.get_weight_data())
    t = time.perf_counter()
    U = ov.integrate(f, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), nthreads=cores)
    t_int = time.perf_counter() - t
    # single-thread figure on a slab of planes so it stays bounded
    zs = max(1, n // 16)
    t = time.perf_counter()
    ov.integrate(f, W, H, cam.inverse_pose(), cam.k(), cam.kinv(), z_range=(n // 2, n // 2 + zs), nthreads=1)
    t_int1 = (time.perf_counter() - t) * (n / zs)
    # probe with every 64th row, then size the sample to the remaining CPU budget (at least every 16th row)
    t = time.perf_counter()
    ov.raycast_rows(W, H, cam.pose(), cam.kinv(), 0, H, 64, nthreads=cores)
    probe = time.perf_counter() - t
    remaining = max(1.0, budget_s - (t_bil + t_int + t_int1 * zs / n + probe))
    row_step = int(min(16, max(1, math.ceil(64 * probe / remaining))))
    t = time.perf_counter()
    Vs, samples = ov.raycast_rows(W, H, cam.pose(), cam.kinv(), 0, H, row_step, nthreads=cores)
    t_ray = time.perf_counter() - t
    rays = W * len(range(0, H, row_step))
    t_ray_full = t_ray * (W * H / rays)
    step_s = t_bil + t_int + t_ray_full
    # ... and, where oracle/_ref travelled to this box, integrate's loop around the REFERENCE's own compiled world_to_pixel / pixel_to_camera /
    # world_to_camera (oracle/ref_transforms_wrap.cpp; src/Utilities/cuda_coordinate_transforms.cu built with g++), one thread, on a slab of
    # the same grid: what the reference's per-voxel code costs a host core -- reported beside the port's figure, not instead of it (the loop
    # itself and the blend are restated; the reference's kernel file does not compile without Eigen)
    ref_fn = None
    if O.have_ref_transforms():
        zs_r = max(1, n // 32)
        rd = np.full(n * n * zs_r, np.float32(ov.truncation_distance()), np.float32)
        rw = np.zeros_like(rd)
        vs = ov.voxel_size()
        t = time.perf_counter()
        # (a grid of n x n x zs_r voxels with the volume's voxel size, shifted to the middle planes: the same projections as that slab's)
        O.ref_integrate_composed(rd, rw, (n, n, zs_r), vs, ov.truncation_distance(), cam.inverse_pose(), cam.k(), cam.kinv(), f, W, H,
                                 offset_at_clear=(0.0, 0.0, float(vs[2]) * (n // 2)), offset_now=(0.0, 0.0, 0.0))
        ref_fn = round(n * n * zs_r / (time.perf_counter() - t) / 1e6, 2)
    return {"value": round(n ** 3 / step_s / 1e6, 3), "unit": "Mvoxels/s", "cores": cores, "kind": "port",
            "integrate_mvoxels_per_s_1thread_reference_functions": ref_fn,
            "sample": "1 frame: bilateral 640x480 + integrate over the full %d^3 grid (%d voxels updated) + ray cast of "
                      "every %dth row (%d rays, %d samples) scaled to 307200 rays; oracle/tsdf_oracle.c, OpenMP over "
                      "z planes / rows, all %d host threads" % (n, U, row_step, rays, samples, cores),
            "integrate_mvoxels_per_s": round(n ** 3 / t_int / 1e6, 2),
            "integrate_mvoxels_per_s_1thread": round(n ** 3 / t_int1 / 1e6, 2),
            "raycast_mrays_per_s": round(rays / t_ray / 1e6, 4),
            "bilateral_ms": round(t_bil * 1e3, 2),
            "wall_seconds_spent": round(t_bil + t_int + t_int1 * zs / n + probe + t_ray, 2),
            "cpu_seconds_spent": round((t_bil + t_int + probe + t_ray) * cores + t_int1 * zs / n, 1)}


if __name__ == "__main__":
    main()
