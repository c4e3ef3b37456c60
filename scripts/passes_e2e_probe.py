#!/usr/bin/env python3
"""Multi-pass conversion end to end on a 50M-point binary PLY (recorded, no gate).

The same file through pcc_convert_files (the plain conversion, whose code this
feature does not change) and through pcc_convert_files_passes with a cap that
gives 1 pass and one that gives 4, each into a fresh directory.  The expected
cost of the passes path is 1 + passes reads of the file; the per-stage host
times come from pcc_pass_report.

    python scripts/passes_e2e_probe.py --out profiles/passes_e2e_probe.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud_amd"))

import pcconv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--tmp", default=None, help="directory for the PLY and the outputs (default: a temporary one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "passes_e2e_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("passes_e2e_probe: no GPU (there is nothing to measure on a CPU)")
    n = a.points
    td = tempfile.mkdtemp(prefix="passes_e2e_", dir=a.tmp)
    try:
        # uniform in [-1000, 1000)^3 (8 level-0 cells of about n/8), generated on the device
        dev = torch.device("cuda", 0)
        t = torch.empty((n, 4), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        pcconv.synth_device(t.data_ptr(), 0, n, 11, 0)
        pts = t.cpu().numpy().view(pcconv.POINT_DTYPE).reshape(-1)
        del t
        torch.cuda.empty_cache()
        ply = os.path.join(td, "cloud.ply")
        pcconv.write_ply(ply, pts)
        grid = pcconv.shard_grid_from_bbox([-1000.0] * 3, [999.0] * 3)
        ids = [np.floor(pts[k] / np.float32(1000.0)).astype(np.int64) + 1 for k in "xyz"]
        hist = np.bincount((ids[0] * 2 + ids[1]) * 2 + ids[2], minlength=grid.ncells)
        del pts, ids
        two = np.sort(hist)[::-1]
        cap4 = int(two[0] + two[1])        # two of the eight cells per pass: 4 passes
        runs = {}

        def timed(name, **kw):
            out = os.path.join(td, name)
            t0 = time.perf_counter()
            rep = pcconv.convert_from_paths([ply], out, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            with open(os.path.join(out, "metadata.json")) as f:
                meta = json.load(f)
            runs[name] = {"wall_ms": wall, "report": rep, "number_of_points": meta.get("number_of_points")}
            shutil.rmtree(out)

        timed("warmup_plain")              # first use: code objects, allocations, the page cache of the PLY
        timed("plain")
        timed("passes_1", max_resident_points=n)
        timed("passes_4", max_resident_points=cap4)
        runs.pop("warmup_plain")
        assert runs["passes_1"]["report"]["passes"] == 1 and runs["passes_4"]["report"]["passes"] == 4
        res = {"device": torch.cuda.get_device_name(0), "points": n, "ply_bytes": os.path.getsize(ply),
               "level0_cells": hist.tolist(), "cap_for_4_passes": cap4, "runs": runs,
               "note": "plain = pcc_convert_files, unchanged by this feature; wall_ms is a host clock around the "
                       "whole call (read, upload, build, cell files, metadata.json); expected reads of the file: "
                       "1 + passes"}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
    finally:
        shutil.rmtree(td, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
