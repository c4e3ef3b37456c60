#!/usr/bin/env python3
"""pcc_pass_select against pcc_shard_route on one 16M-point device piece.

Uniform points over the default grid (8 level-0 cells), the cells mapped onto 4
passes / 4 ranks by the same table.  Select does strictly less work than the
route (one destination, no key array, at most the same bytes), so the gate is:
the median of 5 timed select calls (after warm-up, alternating with the route)
must not exceed the route's median by more than the route's own min-to-max
spread.  Both calls end in a device synchronise, so a host clock times them.

    python scripts/passes_select_probe.py --out profiles/passes_select_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud_amd"))

import pcconv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "passes_select_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("passes_select_probe: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    n = a.points
    pts = torch.empty((n, 4), dtype=torch.int32, device=dev)
    out = torch.empty((n, 4), dtype=torch.int32, device=dev)
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    table = torch.tensor([c % 4 for c in range(8)], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pcconv.synth_device(pts.data_ptr(), 0, n, 7, 0)
    grid = pcconv.shard_grid_from_bbox([-1000.0] * 3, [999.0] * 3)
    rel = np.arange(0, n + 1, 10_000, dtype=np.uint64)   # the batch starts of a 10 000-point batching

    def t_select(boundaries=rel):
        t0 = time.perf_counter()
        kept, _ = pcconv.pass_select(pts.data_ptr(), n, grid, table.data_ptr(), 0, out.data_ptr(), n, boundaries)
        return (time.perf_counter() - t0) * 1e3, kept

    def t_route():
        t0 = time.perf_counter()
        counts = pcconv.shard_route(pts.data_ptr(), n, 0, grid, table.data_ptr(), 4, out.data_ptr(), keys.data_ptr())
        return (time.perf_counter() - t0) * 1e3, counts

    for _ in range(a.warmup):
        t_select()
        t_select(())
        t_route()
    sel, bare, rte, kept, counts = [], [], [], 0, []
    for _ in range(a.repeats):   # alternating, so that all see the same machine
        ms, kept = t_select()    # as the conversion calls it: with the piece's batch starts (the gated figure)
        sel.append(ms)
        ms, _ = t_select(())     # compaction alone
        bare.append(ms)
        ms, counts = t_route()
        rte.append(ms)
    assert kept == counts[0], (kept, counts)
    sel_med, rte_med = statistics.median(sel), statistics.median(rte)
    rte_spread = max(rte) - min(rte)
    res = {
        "device": torch.cuda.get_device_name(0),
        "points": n, "kept": kept, "boundaries": int(len(rel)), "repeats": a.repeats, "warmup": a.warmup,
        "select_ms": sel, "route_ms": rte,
        "select_median_ms": sel_med, "route_median_ms": rte_med,
        "select_spread_ms": max(sel) - min(sel), "route_spread_ms": rte_spread,
        "select_no_boundaries_ms": bare, "select_no_boundaries_median_ms": statistics.median(bare),
        # 16 B read twice (count, scatter) + 16 B written per kept point
        "select_gb_per_s": (32 * n + 16 * kept) / (sel_med * 1e-3) / 1e9,
        # the route also writes every point and a 4-byte key for each
        "route_gb_per_s": (32 * n + 20 * n) / (rte_med * 1e-3) / 1e9,
        "gate": "select_median_ms <= route_median_ms + route_spread_ms",
        "gate_passed": bool(sel_med <= rte_med + rte_spread),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if res["gate_passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
