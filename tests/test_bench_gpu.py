"""bench.py --dump-outputs: the arrays written for a built converter against
the C oracle's cloud of the same input (headers bit-exact, grid membership,
overflow lists in stored order), and the sample of a cloud too large to write
whole as a subset of it."""
import struct

import numpy as np
import pytest

from canon import read_dir_fast
from gpu_util import pcconv, run_oracle
from oracle_ctypes import synth
from test_bench_cpu import _bench

pytestmark = pytest.mark.gpu

CFG = {"sub_grid_dimension": 16, "cell_point_overflow_limit": 100}   # several levels and kept lists at 200k points
N = 200_003


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """(bench module, whole dump, sampled dump, oracle cells) of one build."""
    b = _bench()
    base = tmp_path_factory.mktemp("dump")
    pts = synth(7, 0, N)
    err, _ = run_oracle(str(base / "oracle"), [pts], cfg=CFG)
    assert err == 0
    conv = pcconv.Converter(str(base / "gpu"), config=CFG)
    try:
        conv.add_points(pts)
        st = conv.build()
        b.dump_outputs(conv, st, str(base / "whole"))
        keep = b.DUMP_SAMPLE_BYTES
        b.DUMP_SAMPLE_BYTES = 32 * N // 40
        try:
            b.dump_outputs(conv, st, str(base / "sample"))
        finally:
            b.DUMP_SAMPLE_BYTES = keep
    finally:
        conv.close()
    load = lambda d: {k: np.load(str(base / d / (k + ".npy"))) for k in ("stats", "cells", "grid", "overflow")}
    return b, st, load("whole"), load("sample"), read_dir_fast(str(base / "oracle"))[0]


def _recs(rows):
    """float32 rows (x, y, z, r, g, b, a) back to 16-byte point records."""
    p = np.zeros(len(rows), dtype=pcconv.POINT_DTYPE)
    p["x"], p["y"], p["z"] = rows[:, 0], rows[:, 1], rows[:, 2]
    p["rgba"] = rows[:, 3:].astype(np.uint8)
    return p


def test_dump_is_the_oracles_cloud(dumps):
    _, st, w, _, ref = dumps
    assert w["stats"].dtype == np.float64 and w["cells"].dtype == np.float64
    assert w["grid"].dtype == np.float32 and w["overflow"].dtype == np.float32
    assert list(w["stats"][:8]) == [st[k] for k in ("number_of_points", "hierarchies", "levels", "cells", "slabs",
                                                    "arrivals", "grid_points", "kept_points")]
    cells = w["cells"]
    assert len(cells) == len(ref) and len(w["grid"]) == st["grid_points"] and len(w["overflow"]) == st["kept_points"]
    assert st["kept_points"] > 0 and st["levels"] > 1
    ids = [tuple(int(v) for v in c[:4]) for c in cells]
    assert ids == sorted(ref)
    go = np.concatenate([[0], np.cumsum(cells[:, 5])]).astype(np.int64)
    oo = np.concatenate([[0], np.cumsum(cells[:, 6])]).astype(np.int64)
    for i, c in enumerate(cells):
        hdr, grid, buckets = ref[ids[i]]
        total, number, overflow, size, sub, px, py, pz = struct.unpack("<III5f", hdr)
        assert [c[4], c[5], c[6]] == [total, number, overflow]
        assert np.float32(c[7:12]).tobytes() == np.float32([size, sub, px, py, pz]).tobytes()
        g = w["grid"][go[i]:go[i + 1]]
        assert (g[:, 0] == i).all()
        assert np.sort(_recs(g[:, 1:]).view("V16")).tobytes() == grid
        o = w["overflow"][oo[i]:oo[i + 1]]
        assert (o[:, 0] == i).all()
        assert abs(c[45:48] - g[:, 1:4].sum(axis=0, dtype=np.float64)).max() <= 1e-6 * max(1, len(g))
        assert abs(c[48:51] - o[:, 1:4].sum(axis=0, dtype=np.float64)).max() <= 1e-6 * max(1, len(o))
        got, at = [], 0
        for e in range(int(c[12])):
            child, n = tuple(int(v) for v in c[13 + 4 * e:16 + 4 * e]), int(c[16 + 4 * e])
            got.append((child, None if n == 0 else _recs(o[at:at + n, 1:]).tobytes()))
            at += n
        assert at == len(o) and (c[13 + 4 * int(c[12]):45] == -1).all()
        assert tuple(sorted(got, key=lambda t: t[0])) == buckets


def test_sampled_dump_is_a_subset_in_the_same_order(dumps):
    b, _, w, s, _ = dumps
    assert (s["stats"] == w["stats"]).all() and (s["cells"] == w["cells"]).all()
    rate = -(-N * 32 // (32 * N // 40))
    assert rate > 1
    for name in ("grid", "overflow"):
        keep = b._sample_mask(_recs(w[name][:, 1:]), rate)
        assert 0 < keep.sum() < len(w[name])
        assert s[name].tobytes() == w[name][keep].tobytes()
