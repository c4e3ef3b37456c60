"""Multi-pass conversion, host side (no GPU): the pass plan (pcc_pass_plan) is
first-fit decreasing over the level-0 cells' point counts -- heaviest first,
ties by cell id, each cell into the lowest-numbered pass that still has room --
and the new entry points are exported without an ABI bump."""
import errno
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud_amd"))

import pcconv  # noqa: E402


def ffd(w, cap):
    """First-fit decreasing, restated: (pass of each cell, passes)."""
    w = np.asarray(w, dtype=np.uint64)
    order = sorted(range(len(w)), key=lambda i: (-int(w[i]), i))
    load, out = [], np.zeros(len(w), dtype=np.uint32)
    for i in order:
        if w[i] == 0:
            continue
        for p, l in enumerate(load):
            if l + int(w[i]) <= cap:
                break
        else:
            load.append(0)
            p = len(load) - 1
        load[p] += int(w[i])
        out[i] = p
    return out, max(1, len(load))


def histograms():
    rng = np.random.default_rng(17)
    yield np.array([5, 0, 5, 5, 0, 3, 3, 3, 2], dtype=np.uint64), 8          # ties and empty cells
    yield np.array([7], dtype=np.uint64), 7
    yield np.zeros(6, dtype=np.uint64), 4                                     # nothing at all
    for k in range(12):
        n = int(rng.integers(1, 400))
        w = rng.integers(0, 1000, n).astype(np.uint64)
        w[rng.random(n) < 0.3] = 0                                            # empty cells
        if n > 4:
            w[rng.integers(0, n, n // 4)] = w[rng.integers(0, n)]             # ties
        if w.max() == 0:
            w[0] = 1
        yield w, int(w.max()) + int(rng.integers(0, 3000))
    yield (rng.integers(1, 2**40, 64).astype(np.uint64)), 2**41               # counts beyond 32 bits


@pytest.mark.parametrize("case", list(histograms()), ids=lambda c: f"n{len(c[0])}cap{c[1]}")
def test_pass_plan_is_first_fit_decreasing(case):
    w, cap = case
    got, npasses = pcconv.pass_plan(w, cap)
    want, wpasses = ffd(w, cap)
    assert npasses == wpasses
    assert np.array_equal(got, want)
    # every pass within the cap; every non-empty cell in exactly one pass below npasses; empty cells in pass 0
    load = np.bincount(got, weights=w.astype(np.float64), minlength=npasses)
    assert load.max() <= cap
    assert got.max() < npasses and np.all(got[w == 0] == 0)
    if w.sum():
        assert set(got[w > 0]) == set(range(npasses))
    again, n2 = pcconv.pass_plan(w, cap)
    assert n2 == npasses and np.array_equal(again, got)                       # deterministic


def test_pass_plan_cap_edges():
    w = np.array([10, 0, 40, 40, 7, 0, 3], dtype=np.uint64)
    got, npasses = pcconv.pass_plan(w, 40)                                    # cap == the heaviest cell
    assert npasses == 3 and np.array_equal(got, ffd(w, 40)[0])
    with pytest.raises(pcconv.PccError) as e:                                 # one below it
        pcconv.pass_plan(w, 39)
    assert e.value.code == -errno.E2BIG
    assert "40" in str(e.value) and "cell 2" in str(e.value)                  # the first heaviest cell and its count
    for cap in (100, 101, 2**63):                                             # at or above the total: one pass
        got, npasses = pcconv.pass_plan(w, cap)
        assert npasses == 1 and not got.any()
    with pytest.raises(pcconv.PccError) as e:
        pcconv.pass_plan(w, 0)
    assert e.value.code == -errno.EINVAL


def test_new_symbols_exported_without_an_abi_bump():
    lib = pcconv.lib()
    for name in ("pcc_pass_plan", "pcc_pass_select", "pcc_convert_files_passes"):
        assert name in pcconv.EXPORTS and hasattr(lib, name)
    assert lib.pcc_abi_version() == pcconv.ABI_VERSION == 2
    import ctypes as C
    assert C.sizeof(pcconv.PassReport) == 64 and C.sizeof(pcconv.Stats) == 128 and C.sizeof(pcconv.Options) == 24


def test_convert_passes_refuses_bad_arguments_without_device_work(tmp_path):
    """The refusals that need no device: a zero cap, and a merge into a
    directory that already holds cell files."""
    out = tmp_path / "o"
    with pytest.raises(pcconv.PccError) as e:
        pcconv.convert_from_paths([], str(out), max_resident_points=0)
    assert e.value.code == -errno.EINVAL
    (out / "h_0").mkdir(parents=True)
    (out / "h_0" / "c_0_0_0.bin").write_bytes(b"")
    with pytest.raises(pcconv.PccError) as e:
        pcconv.convert_from_paths([], str(out), max_resident_points=10)
    assert e.value.code == -errno.ENOTSUP
    assert not (out / "metadata.json").exists()
