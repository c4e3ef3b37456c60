"""bench.py's JSON line (the driver's contract): the keys, types and the two
extra objects, built by record() from synthetic stage numbers (no GPU)."""
import importlib.util
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(HERE, "..", "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _line(world):
    b = _bench()
    sys.argv = ["bench.py"]
    args = b.parse()
    k = {"dense_arrivals": 2_780_291_831, "small_arrivals": 209_765_606, "dense_launches": 3, "small_launches": 4,
         "level0_ms": 16.5, "dense_ms": 33.5, "small_ms": 3.4, "bucket_ms": 1.3, "next_ms": 0.4}
    return args, b.record(args, world, 55.5, 4, 4680, 898_651, 2_990_057_437, k, 33.5,
                          "single GPU" if world == 1 else f"level-0 cell sharding over {world} ranks")


def test_record_has_the_contract_keys():
    args, r = _line(1)
    for key, typ in [("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int),
                     ("warmup", int), ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str),
                     ("dtype", str), ("data", str), ("config", dict), ("roofline", dict)]:
        assert isinstance(r[key], typ), key
    assert "vs_baseline" in r and r["vs_baseline"] is None
    assert r["value"] == args.points / 0.0555
    assert r["scaling"] in ("weak", "strong") and r["higher_is_better"] is True
    assert "workload" in r["config"] and "model" not in r["config"]
    rf = r["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s"
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert abs(rf["achieved"] - 32.0 * 2_780_291_831 / 0.0335 / 1e9) < 1e-6


def _parse(*argv):
    b = _bench()
    sys.argv = ["bench.py", *argv]
    return b.parse()


def test_plain_run_measures_only_the_headline():
    a = _parse("--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = _parse("--full", "--cpu-mode-a", "--dump-outputs", "d")
    assert a.full and a.cpu_mode_a and a.cpu_sample > 0 and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [("--cpu-full",), ("--cpu-mode-a",), ("--steps", "0")])
def test_arguments_that_cannot_be_honoured_are_refused(argv):
    with pytest.raises(SystemExit):
        _parse(*argv)


def test_sample_mask_depends_on_the_point_alone():
    import numpy as np
    b = _bench()
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "u1", (4,))])
    rng = np.random.RandomState(1)
    p = np.zeros(200_000, dtype=dt)
    for a in "xyz":
        p[a] = rng.uniform(-1000, 1000, len(p)).astype(np.float32)
    p["rgba"] = rng.randint(0, 256, (len(p), 4))
    assert b._sample_mask(p, 1).all()
    m = b._sample_mask(p, 50)
    assert 0.8 * len(p) / 50 < m.sum() < 1.2 * len(p) / 50   # 4000 expected, sd 63
    perm = rng.permutation(len(p))
    assert (b._sample_mask(p[perm], 50) == m[perm]).all()
    r = b._rows(p[m], 3)
    assert r.dtype == np.float32 and r.shape == (m.sum(), 8) and (r[:, 0] == 3).all()
    assert (r[:, 1] == p[m]["x"]).all() and (r[:, 4:] == p[m]["rgba"]).all()


def test_record_for_several_ranks():
    _, r = _line(8)
    assert r["n_gpus"] == 8
    assert r["value"] > 0
