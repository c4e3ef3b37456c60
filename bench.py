#!/usr/bin/env python3
"""bench.py — points/sec of the MI355X hierarchy/LOD build (BASELINE.json metric).

Workload at N=1: config 4 — 1B uniform points in [-1000,1000)^3, seed 4, one
input "file" cut into 10 000-point batches (lib.rs:32), generated directly in
HBM before timing.  A step = one full build (point-converter/src/converter.rs
add_points_batch/add_points_in_hierarchy for every batch) from the resident
input to finished cell images in HBM (grid winners, overflow lists, headers'
values, metadata values).  File writing is not part of a step.

Prints ONE JSON line (rank 0).  A plain run (--gpus 1 --steps K --warmup W)
sets up, warms up, times the K steps and prints the line; --dump-outputs DIR
also writes the cloud of the last timed step (dump_outputs).  Extra objects:
  roofline     — dominant kernel (dense slab kernel, k_slab): algorithmic
                 bytes (32 B per arrival it processes) / its
                 summed HIP-event duration on the engine stream, taken from
                 the timed steps themselves;
  cpu_baseline — with --full only: the C oracle (sequential restatement, 1
                 thread, in memory = SURVEY §8d mode (B)) on a bounded sample
                 of the same workload at its density (config 4: the points of
                 one level-1 cell; --cpu-full: every level-0 part of the whole
                 run, summed), and speedup_vs_cpu; --cpu-mode-a beside it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "point-cloud_amd"))

HBM_PEAK_GBS = 8000.0      # MI355X spec (MI355X_MICROARCH.md: 8.0 TB/s; 6.29 measured)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=1_000_000_000)
    ap.add_argument("--kind", type=int, default=0,
                    help="0 uniform (config 4), 2 Gaussian mixture (config 3, SURVEY 8d), 1 clustered blobs")
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--cpu-sample", type=int, default=20_000_000, help="oracle prefix sample (points); 0 = skip")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--cpu-full", action="store_true",
                    help="cpu_baseline = mode (B) over the WHOLE workload, per level-0 part, summed (minutes of CPU)")
    ap.add_argument("--cpu-mode-a", action="store_true",
                    help="also time SURVEY 8d mode (A): the oracle with the reference's LRU-100 cell cache and "
                         ".bin write-back (converter.rs:92,160-216); full run up to 10M points, else a prefix "
                         "capped at --cpu-cap seconds")
    ap.add_argument("--cpu-cap", type=float, default=60.0, help="mode (A) time cap (s) beyond 10M points")
    ap.add_argument("--exchange", action="store_true",
                    help="N > 1: every rank holds a key range of the input in HBM and the step routes it to the "
                         "level-0 owners over RCCL (shard_build); default: the input partitioned by owner at load "
                         "(owner_partition), no data exchange in the step")
    ap.add_argument("--merge-prior", type=int, default=0,
                    help="config 5: merge --points new points (seed --seed) into a cloud built from this many "
                         "config-4 points (seed 4); 0 = fresh build")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure, everything else this bench measures: the CPU baselines "
                         "(cpu_baseline from --cpu-sample / --cpu-full, --cpu-mode-a) and the speed-ups against "
                         "them; without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step built (dump_outputs) to DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if (args.cpu_full or args.cpu_mode_a) and not args.full:
        ap.error("--cpu-full and --cpu-mode-a are measured with --full")
    return args


def host_cpu():
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"nproc": os.cpu_count(), "model": model}


def cpu_full_mode_b(args):
    """SURVEY.md §8d mode (B), in-memory, FULL run: the sequential oracle converts
    every level-0 subtree of the whole workload (oracle/digest_main.c, one process
    per level-0 cell, global 10 000-point batches); only the conversion is timed
    (the generator is not) and the single-thread times are summed, since level-0
    subtrees are independent.  Minutes of CPU: not part of the default run."""
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "build/orc_digest"])
    exe = os.path.join(ROOT, "oracle", "build", "orc_digest")
    streams = [str(args.seed), str(args.kind), str(args.points)]

    def part(p):
        out = subprocess.run([exe, str(p), "8"] + streams, capture_output=True, text=True, check=True).stdout
        return [json.loads(x) for x in out.splitlines() if '"summary"' in x][-1]["convert_seconds"]
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        secs = list(ex.map(part, range(8)))
    tot = sum(secs)
    return dict({"value": args.points / tot, "unit": "points/s", "cores": 1, "kind": "port",
                 "sample": f"mode (B) full run: all {args.points} points, 8 level-0 parts converted separately "
                           f"(sum of single-thread conversion times {tot:.1f} s; per part {[round(x, 1) for x in secs]})"},
                **host_cpu())


def cpu_mode_a(args):
    """SURVEY.md §8d mode (A), the faithful reference configuration: the sequential
    C restatement with the reference's LRU cache of 100 cells (converter.rs:92),
    every evicted cell written to a .bin file on the local disk and read back when
    touched again (converter.rs:160-216), 10 000-point batches.  Up to 10M points
    the whole run; beyond, the prefix converted within --cpu-cap seconds (points/s
    over that prefix).  Timed like the reference's "Finished converting" log
    (lib.rs:56-59): the final flush of the cached cells (converter.rs:241-246) is
    reported apart.  Config 5: the existing cloud (converted untimed, in memory,
    and written to the directory) is read lazily from disk, as the reference does."""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from oracle_ctypes import Oracle, synth
    tmp = tempfile.mkdtemp(prefix="pcc_mode_a_", dir="/tmp")
    try:
        if args.merge_prior:   # the existing cloud: a config-4 prefix, same size ratio as the run
            n0 = min(args.merge_prior, 10 * 10_000_000)
            o = Oracle()
            for a in range(0, n0, 1_000_000):
                o.add_file(synth(4, 0, min(1_000_000, n0 - a), first=a))
            o.write(tmp)
            o.close()
        full = args.points <= 10_000_000
        cap = float("inf") if full else args.cpu_cap
        o = Oracle()
        o.set_lru(tmp, 100)
        done, conv = 0, 0.0
        chunk = 1_000_000
        while done < args.points and conv < cap:
            m = min(chunk, args.points - done)
            pts = synth(args.seed, args.kind, m, first=done)
            for b in range(0, m, 10_000):
                t0 = time.perf_counter()
                o.add_batch(pts[b:b + 10_000])
                conv += time.perf_counter() - t0
                done += min(10_000, m - b)
                if conv >= cap:
                    break
        st = o.lru_stats()
        t0 = time.perf_counter()
        o.write(tmp)
        flush = time.perf_counter() - t0
        err = o.error
        o.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    what = "whole run" if done == args.points else f"prefix of {done} of {args.points} points ({cap:.0f} s cap)"
    return dict({"value": done / conv, "unit": "points/s", "cores": 1, "kind": "port", "mode": "A",
                 "sample": f"mode (A): {what}, seed {args.seed}, sequential C restatement with the LRU-100 cell cache "
                           f"and .bin write-back to local disk ({st['evictions']} evictions, {st['loads']} reloads), "
                           f"conversion {conv:.1f} s, final flush {flush:.1f} s (not in the rate, as lib.rs:56-59)"
                           + (f"; existing cloud of {n0} config-4 points read lazily from disk" if args.merge_prior else ""),
                 "points_reached": done, "flush_s": flush, "error": err}, **host_cpu())


# full-run mode (B) measurement of config 4 on the GPU box (bench.py --cpu-full, round 2)
FULL_MODE_B = os.path.join(ROOT, "profiles", "r2_cpu_full_mode_b_1b.json")


def cpu_baseline(args):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from oracle_ctypes import Oracle, synth
    if args.kind == 0 and not args.merge_prior:
        # Uniform workload: the points of the whole run that fall in one level-1
        # cell, [0, 500)^3, at the run's density (N / 64 points).  A point's path
        # (slot competition, bucket spills, 4 levels at N = 1e9) depends only on the
        # points around it, so this keeps the full run's depth per point, unlike a
        # prefix of the stream, which has fewer levels per point.
        n = args.points // 64
        pts = synth(args.seed, 0, n, lo=0.0, ext=500.0)
        o = Oracle()
        t0 = time.perf_counter()
        o.add_file(pts)
        dt = time.perf_counter() - t0
        lv = o.hierarchies
        o.close()
        rec = dict({"value": n / dt, "unit": "points/s", "cores": 1, "kind": "port",
                    "sample": f"{n} uniform points (seed {args.seed}) in the level-1 cell [0,500)^3 at the density of "
                              f"the full {args.points}-point run ({lv} levels, as the full run), sequential C "
                              f"restatement (oracle/pcc_oracle.c, in-memory cells = mode (B), 10 000-point "
                              f"batches), {dt:.1f} s"}, **host_cpu())
        # the sample is friendlier than the whole run: state the full run's rate beside it
        try:
            with open(FULL_MODE_B) as f:
                fb = json.load(f)
            if args.points == 1_000_000_000 and args.seed == 4 and "config4" in fb["config"]["workload"]:
                full = fb["cpu_baseline"]["value"]
                rec["full_run_mode_b"] = {"value": full, "source": os.path.relpath(FULL_MODE_B, ROOT),
                                          "sample_over_full": rec["value"] / full,
                                          "note": "all 1e9 points through mode (B) on the GPU box's host, "
                                                  "8 level-0 parts timed separately and summed"}
        except (OSError, ValueError, KeyError):
            pass
        return rec
    if args.kind == 0 and args.merge_prior:
        # Config 5's shape at the full run's density: the existing cloud's and the
        # new points' share of one level-1 cell, [0, 500)^3 (1/64 of each, the
        # same depth per point and the same old:new ratio); the existing cloud is
        # converted untimed, the merge of the new points is timed
        n0, n = args.merge_prior // 64, args.points // 64
        o = Oracle()
        o.add_file(synth(4, 0, n0, lo=0.0, ext=500.0))
        pts = synth(args.seed, 0, n, lo=0.0, ext=500.0)
        t0 = time.perf_counter()
        o.add_file(pts)
        dt = time.perf_counter() - t0
        lv = o.hierarchies
        o.close()
        return dict({"value": n / dt, "unit": "points/s", "cores": 1, "kind": "port",
                     "sample": f"merge of {n} uniform points (seed {args.seed}) into an in-memory cloud of {n0} "
                               f"(seed 4), both in the level-1 cell [0,500)^3 at the full run's density ({lv} levels), "
                               f"sequential C restatement (oracle/pcc_oracle.c, 10 000-point batches), {dt:.1f} s"},
                    **host_cpu())
    n = min(args.cpu_sample, args.points)
    pts = synth(args.seed, args.kind, n)
    o = Oracle()
    if args.merge_prior:   # untimed existing cloud: a prefix of the config-4 stream, 5x the timed sample
        o.add_file(synth(4, 0, min(args.merge_prior, 5 * n)))
    t0 = time.perf_counter()
    o.add_file(pts)
    dt = time.perf_counter() - t0
    o.close()
    if args.merge_prior:
        return dict({"value": n / dt, "unit": "points/s", "cores": 1, "kind": "port",
                     "sample": f"merge of the first {n} points of the seed-{args.seed} stream into an in-memory cloud "
                               f"of the first {min(args.merge_prior, 5 * n)} config-4 points, sequential C restatement "
                               f"(oracle/pcc_oracle.c, 10 000-point batches), {dt:.1f} s"}, **host_cpu())
    return dict({"value": n / dt, "unit": "points/s", "cores": 1, "kind": "port",
                 "sample": f"first {n} points of the same seed-{args.seed} stream through the sequential C restatement "
                           f"(oracle/pcc_oracle.c, in-memory cells, 10 000-point batches), {dt:.1f} s"}, **host_cpu())


METRIC = "points/sec converted (octree+LOD build), 1B synthetic pts, 1/2/4/8 MI355X"


def _latest_pmc():
    """The newest round's committed PMC summary (profiles/rNN_pmc_traffic_1b.json),
    its final-tree pass (rNN_final_pmc_traffic_1b.json) first."""
    import glob
    import re as _re

    def rank(path):
        m = _re.match(r"r(\d+)", os.path.basename(path))
        return (int(m.group(1)) if m else 0, "_final_" in os.path.basename(path), path)
    c = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_1b.json")), key=rank)
    return c[-1] if c else os.path.join(ROOT, "profiles", "r1_pmc_traffic_1b.json")


PMC_SUMMARY = _latest_pmc()


def pmc_traffic(workload):
    """HBM bytes per launch of k_slab (dense slabs) from the committed rocprofv3 PMC summary
    (scripts/pmc.sh + scripts/pmc_summary.py: 2 x FETCH_SIZE + WRITE_SIZE, per
    MI355X_MICROARCH.md), only when it was measured on this exact workload."""
    try:
        with open(PMC_SUMMARY) as f:
            pm = json.load(f)
    except (OSError, ValueError):
        return None, None
    if pm.get("workload") != workload:
        return None, None
    return pm["dense_kernel"]["hbm_bytes_per_launch"], os.path.relpath(PMC_SUMMARY, ROOT)


def workload_name(args):
    """BASELINE.json config label of a fresh build: configs 1/2/4 are the uniform
    clouds of 100k / 10M / 1B points, config 3 the 100M Gaussian mixture; any
    other size or kind is named by what it is."""
    if args.kind == 0:
        cfg = {100_000: "config1: ", 10_000_000: "config2: ", 1_000_000_000: "config4: "}.get(args.points, "")
        return cfg + "%d uniform points in [-1000,1000)^3, seed %d" % (args.points, args.seed)
    if args.kind == 2:
        cfg = "config3: " if args.points == 100_000_000 else ""
        return cfg + "%d Gaussian-mixture points (32 clusters, SURVEY 8d), seed %d" % (args.points, args.seed)
    return "clustered blobs: %d points, seed %d" % (args.points, args.seed)


def record(args, n_gpus, ms, st_levels, st_cells, st_slabs, arrivals, k, dense_ms, parallelism):
    """The one JSON line (rank 0).  roofline: dense slab kernel k_slab,
    algorithmic bytes = 32 B per arrival it processed over its
    HIP-event time on the engine stream (rank 0's engine when N > 1)."""
    dense_arr = k["dense_arrivals"]
    achieved = 32.0 * dense_arr / (dense_ms / 1e3) / 1e9 if dense_ms > 0 else 0.0
    whole = 32.0 * arrivals / (ms / 1e3) / 1e9
    workload = workload_name(args)
    if args.merge_prior:
        workload = ("config5: +%d %s points (seed %d) merged into the %d-point config-4 cloud (seed 4)" %
                    (args.points, "uniform" if args.kind == 0 else "clustered", args.seed, args.merge_prior))
    traffic, tsrc = pmc_traffic(workload)
    return {
        "metric": METRIC,
        "value": args.points / (ms / 1e3),
        "unit": "points/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic (counter-hash generator in HBM, SURVEY.md §8d)",
        "config": {"workload": workload,
                   "batch": 10000, "levels": st_levels, "cells": st_cells, "slabs": st_slabs,
                   "arrivals_W": arrivals, "parallelism": parallelism},
        "roofline": {"bound": "hbm", "kernel": "k_slab (dense slabs)", "achieved": achieved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                     "traffic_unit": "HBM bytes per launch (2 x FETCH_SIZE + WRITE_SIZE)", "traffic_source": tsrc,
                     "alg_bytes_per_launch": 32.0 * k["dense_arrivals"] / max(k["dense_launches"], 1),
                     "alg_bytes_per_arrival": 32, "kernel_ms_per_step": dense_ms,
                     "whole_build_alg_GBs": whole, "whole_build_frac": whole / HBM_PEAK_GBS,
                     "limiter": "instruction issue in the phases between the two barriers of each 1024-arrival "
                                "step, not HBM: 100 more dependent VALU per wave and step cost +4.4 ms over the "
                                "three dense launches, 100 more SALU +6.0 ms (profiles/r5_salu_valu_probe.txt); one "
                                "1024-thread workgroup per CU (13.6-14.9 resident waves of 16, "
                                "profiles/r6_final_pmc_sq_1b.json), 43-46 % of wave-cycles waiting (DESIGN.md §4)"},
        "stage_ms": k,
    }


DUMP_SAMPLE_BYTES = 40 << 20   # aimed size of the two point samples together (the files stay under 64 MB)
DUMP_LIMIT_BYTES = 64_000_000


def _sample_mask(pts, rate):
    """Which points of a POINT_DTYPE array belong to the sample: a hash of the
    coordinates' bits falls on a multiple of `rate`.  It depends on the point
    alone, not on where the build stored it."""
    import numpy as np
    if rate <= 1:
        return np.ones(len(pts), dtype=bool)
    w = pts.view(np.uint32).reshape(-1, 4)
    h = w[:, 0] * np.uint32(0x9E3779B1)
    h ^= w[:, 1] * np.uint32(0x85EBCA77)
    h ^= w[:, 2] * np.uint32(0xC2B2AE3D)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x2C1B3C6D)
    h ^= h >> np.uint32(12)
    return h % np.uint32(rate) == 0


def _rows(pts, cell):
    """POINT_DTYPE records as float32 rows (cell row, x, y, z, r, g, b, a)."""
    import numpy as np
    out = np.empty((len(pts), 8), dtype=np.float32)
    out[:, 0] = cell
    out[:, 1], out[:, 2], out[:, 3] = pts["x"], pts["y"], pts["z"]
    out[:, 4:] = pts["rgba"]
    return out


def dump_outputs(conv, st, out_dir):
    """--dump-outputs: the cloud the last timed build left in the converter, as a
    caller receives it from pcc_visit_cells, in four float arrays:

      stats.npy   (14,) f64  number_of_points, hierarchies, levels, cells, slabs, arrivals, grid_points,
                             kept_points, bbox_min[3], bbox_max[3]
      cells.npy   (C, 51) f64, EVERY cell, ordered by (hierarchy, x, y, z): those 4, total_number_of_points,
                             number_of_points, number_of_overflow_points, size, sub_cell_size, pos[3],
                             entries, 8 x (child x, y, z, count; -1 past `entries`), then the sums of x, y, z
                             over all its grid points and over all its overflow points (f64 sums of the f32
                             values: they cover the points outside the samples)
      grid.npy    (G, 8) f32  sample of the grid points: row of cells.npy, x, y, z, r, g, b, a; a cell's
                             rows sorted by the points' bits (the grid's order is unspecified, pcconv.h)
      overflow.npy (K, 8) f32 sample of the overflow lists, same columns, in stored order (entry after
                             entry, each list as stored: cell.rs:108-153 keeps arrival order)

    The samples are the points whose coordinate hash falls on a multiple of a
    rate fixed by the cloud's size (all points when they fit), so two builds of
    the same input yield the same rows."""
    import numpy as np
    import pcconv
    total = int(st["grid_points"]) + int(st["kept_points"])
    rate = max(1, -(-total * 32 // DUMP_SAMPLE_BYTES))
    heads, grids, overs = [], [], []

    def visit(ptr):
        v = pcconv.CellView.from_address(ptr)
        row = [v.hierarchy, v.x, v.y, v.z, v.total_number_of_points, v.number_of_points,
               v.number_of_overflow_points, v.size, v.sub_cell_size, *v.pos, v.entries]
        g = v.grid_points()
        lists = v.overflow()
        for e in range(8):
            row += [*lists[e][0], 0 if lists[e][1] is None else len(lists[e][1])] if e < len(lists) else [-1] * 4
        kept = [l for _, l in lists if l is not None]
        o = np.concatenate(kept) if kept else np.empty(0, dtype=pcconv.POINT_DTYPE)
        row += [float(p[a].sum(dtype=np.float64)) for p in (g, o) for a in "xyz"]
        heads.append(row)
        g = g[_sample_mask(g, rate)]
        w = g.view(np.uint32).reshape(-1, 4)
        grids.append(g[np.lexsort((w[:, 3], w[:, 2], w[:, 1], w[:, 0]))])
        overs.append(o[_sample_mask(o, rate)])
        return 0

    conv.visit_cells(visit)
    cells = np.asarray(heads, dtype=np.float64).reshape(-1, 51)
    order = np.lexsort((cells[:, 3], cells[:, 2], cells[:, 1], cells[:, 0]))
    arrays = {
        "stats": np.asarray([st[k] for k in ("number_of_points", "hierarchies", "levels", "cells", "slabs", "arrivals",
                                             "grid_points", "kept_points")] + st["bbox_min"] + st["bbox_max"],
                            dtype=np.float64),
        "cells": cells[order],
        "grid": np.concatenate([_rows(grids[k], i) for i, k in enumerate(order)] or [np.empty((0, 8), np.float32)]),
        "overflow": np.concatenate([_rows(overs[k], i) for i, k in enumerate(order)] or [np.empty((0, 8), np.float32)]),
    }
    size = sum(a.nbytes for a in arrays.values())
    if size > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {size} bytes, over the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main_sharded(args, rank, world):
    """N > 1: one rank per GPU (torchrun), level-0 cells sharded, RCCL exchange."""
    import torch
    import torch.distributed as dist
    from pcconv.dist import HipShardOps, TorchComm, key_range, shard_build
    import pcconv
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # RCCL writes its version banner to fd 1 at communicator creation: route fd 1
    # to stderr for the run and keep the real stdout for the one JSON line
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    # PCC_BENCH_BACKEND=gloo: this path with several ranks on ONE GPU (RCCL refuses
    # two ranks on one device), collectives through host memory -- a rehearsal of
    # the N > 1 line, never a measurement of it
    backend = os.environ.get("PCC_BENCH_BACKEND", "nccl")
    if backend == "gloo":
        local %= max(1, torch.cuda.device_count())
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if backend == "gloo":
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=dev)
    cdev = dev if backend != "gloo" else torch.device("cpu")
    comm = TorchComm(cdev)
    a, b = key_range(args.points, rank, world)
    pts = torch.empty((b - a, 4), dtype=torch.int32, device=dev)
    pcconv.synth_device(pts.data_ptr(), a, b - a, args.seed, args.kind, -1000.0, 2000.0, local)
    torch.cuda.synchronize()
    ops = HipShardOps(local, batch_size=10_000)
    ops.conv.set_profiling(True)
    files = [args.points]
    for _ in range(args.warmup):
        shard_build(comm, ops, pts, a, files)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prof = []
    for _ in range(args.steps):
        res = shard_build(comm, ops, pts, a, files)
        prof.append(ops.conv.kernel_times())
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=cdev)
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    ms = 1000.0 * float(el.item()) / args.steps
    st = res.local
    tot = torch.tensor([st["levels"], st["cells"], st["slabs"], st["arrivals"], res.recv_points], dtype=torch.int64,
                       device=cdev)
    per = [torch.zeros_like(tot) for _ in range(world)]
    dist.all_gather(per, tot)
    stage = shard_build(comm, ops, pts, a, files, sync=torch.cuda.synchronize).ms   # untimed split
    ops.close()
    if rank == 0:
        per = [p.tolist() for p in per]
        k = prof[-1]
        dense_ms = sum(p["dense_ms"] for p in prof) / len(prof)
        rec = record(args, world, ms, max(p[0] for p in per), sum(p[1] for p in per), sum(p[2] for p in per),
                     sum(p[3] for p in per), k, dense_ms, f"level-0 cell sharding over {world} ranks ("
                     + ("grouped RCCL point-to-point exchange)" if backend != "gloo" else "gloo rehearsal on one GPU)"))
        if backend == "gloo":
            rec["note"] = "REHEARSAL: ranks share one GPU, collectives over gloo (host); not a multi-GPU measurement"
        rec["sharding"] = {"points_per_rank": [p[4] for p in per], "stage_ms_rank0": stage, "comm_backend": backend,
                           "hierarchies": res.summary["hierarchies"], "plan": res.plan,
                           "phases_rank0": res.local.get("phases")}
        json_out.write(json.dumps(rec) + "\n")
        json_out.flush()
    dist.destroy_process_group()


def main_owner(args, rank, world):
    """N > 1 (default): one rank per GPU (torchrun), the input partitioned by
    level-0 owner at load (pcconv.dist.owner_partition: every rank generates the
    synthetic input piece by piece on its GPU, as it would decode a file, and
    keeps its own cells' points; untimed, as the N = 1 line's input).  The timed
    step is owner_build: each rank builds its own level-0 subtrees with the
    global batch structure, then one all-reduce of the hierarchy count."""
    import torch
    import torch.distributed as dist
    from pcconv.dist import HipShardOps, TorchComm, owner_build, owner_partition
    import pcconv
    local = int(os.environ.get("LOCAL_RANK", "0"))
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")   # (RCCL's banner goes to fd 1: see main_sharded)
    os.dup2(2, 1)
    backend = os.environ.get("PCC_BENCH_BACKEND", "nccl")
    if backend == "gloo":
        local %= max(1, torch.cuda.device_count())
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if backend == "gloo":
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=dev)
    cdev = dev if backend != "gloo" else torch.device("cpu")
    comm = TorchComm(cdev)
    piece = 1 << 26
    buf = torch.empty((piece, 4), dtype=torch.int32, device=dev)

    def pieces():
        for a in range(0, args.points, piece):
            m = min(piece, args.points - a)
            pcconv.synth_device(buf.data_ptr(), a, m, args.seed, args.kind, -1000.0, 2000.0, local)
            yield buf.narrow(0, 0, m), a

    ops = HipShardOps(local, batch_size=10_000)
    ops.conv.set_profiling(True)
    files = [args.points]
    t_load = time.perf_counter()
    shard = owner_partition(comm, ops, pieces, files)
    torch.cuda.synchronize()
    load_ms = (time.perf_counter() - t_load) * 1e3
    del buf
    for _ in range(args.warmup):
        owner_build(comm, ops, shard)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prof = []
    for _ in range(args.steps):
        res = owner_build(comm, ops, shard)
        prof.append(ops.conv.kernel_times())
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=cdev)
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    ms = 1000.0 * float(el.item()) / args.steps
    st = res.local
    tot = torch.tensor([st["levels"], st["cells"], st["slabs"], st["arrivals"], res.recv_points], dtype=torch.int64,
                       device=cdev)
    per = [torch.zeros_like(tot) for _ in range(world)]
    dist.all_gather(per, tot)
    ops.close()
    if rank == 0:
        per = [p.tolist() for p in per]
        k = prof[-1]
        dense_ms = sum(p["dense_ms"] for p in prof) / len(prof)
        rec = record(args, world, ms, max(p[0] for p in per), sum(p[1] for p in per), sum(p[2] for p in per),
                     sum(p[3] for p in per), k, dense_ms, f"level-0 cell ownership over {world} ranks, input "
                     "partitioned by owner at load (no data exchange in the step)"
                     + (" -- gloo rehearsal on one GPU" if backend == "gloo" else ""))
        if backend == "gloo":
            rec["note"] = "REHEARSAL: ranks share one GPU, collectives over gloo (host); not a multi-GPU measurement"
        rec["sharding"] = {"points_per_rank": [p[4] for p in per], "comm_backend": backend,
                           "load": "owner_partition: each rank generates the whole synthetic input in 64 Mi-point "
                                   "pieces and keeps its own level-0 cells' points (untimed, %.0f ms on rank 0: %s)"
                                   % (load_ms, {k_: round(v, 1) for k_, v in shard.ms.items()}),
                           "owned_cells_rank0": shard.owned_cells}
        json_out.write(json.dumps(rec) + "\n")
        json_out.flush()
    dist.destroy_process_group()


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if args.dump_outputs and (world > 1 or os.environ.get("PCC_BENCH_OWNER") == "1"
                              or os.environ.get("PCC_BENCH_SHARDED") == "1"):
        sys.exit("bench.py: --dump-outputs writes the single-GPU build's cloud; the N > 1 paths keep theirs per rank")
    # (PCC_BENCH_OWNER=1: the owner path at N = 1 too, its RCCL calls on one rank -- a check)
    if (world > 1 or os.environ.get("PCC_BENCH_OWNER") == "1") and not args.exchange and not args.merge_prior:
        args.gpus = world
        main_owner(args, rank, world)
        return
    if world > 1 or os.environ.get("PCC_BENCH_SHARDED") == "1":   # the env var: sharded path at N=1 (check)
        args.gpus = world
        main_sharded(args, rank, world)
        return
    import pcconv
    import tempfile
    tmp = tempfile.mkdtemp(prefix="pcc_bench_")
    conv = pcconv.Converter(tmp, batch_size=10_000, device=0)
    if args.merge_prior:   # config 5: the existing cloud is built (untimed) and adopted in memory
        prior = pcconv.Converter(tempfile.mkdtemp(prefix="pcc_prior_"), batch_size=10_000, device=0)
        prior.add_synthetic(4, 0, args.merge_prior)
        prior.build()
        conv.adopt_prior(prior)
        prior.close()
    conv.add_synthetic(args.seed, args.kind, args.points)
    conv.set_profiling(True)
    for _ in range(args.warmup):
        conv.build()
    prof = []
    # exactly K steps between two points where the device is idle (build()
    # synchronises the engine stream before it returns); the per-step HIP-event
    # read-back stays inside the bracket
    t0 = time.perf_counter()
    for _ in range(args.steps):
        st = conv.build()
        prof.append(conv.kernel_times())
    el = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(conv, st, args.dump_outputs)
    conv.close()
    ms = 1000.0 * el / args.steps
    dense_ms = sum(p["dense_ms"] for p in prof) / len(prof)
    res = record(args, 1, ms, st["levels"], st["cells"], st["slabs"], st["arrivals"], prof[-1], dense_ms,
                 "single GPU")
    if args.full and args.cpu_full:
        res["cpu_baseline"] = cpu_full_mode_b(args)
        res["speedup_vs_cpu"] = res["value"] / res["cpu_baseline"]["value"]
    elif args.full and args.cpu_sample > 0:
        res["cpu_baseline"] = cpu_baseline(args)
        res["speedup_vs_cpu"] = res["value"] / res["cpu_baseline"]["value"]
    if args.cpu_mode_a:
        res["cpu_baseline_mode_a"] = cpu_mode_a(args)
        res["speedup_vs_mode_a"] = res["value"] / res["cpu_baseline_mode_a"]["value"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
