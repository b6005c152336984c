"""CPU: bench.py --dump-outputs writes each result array as float64 .npy with every value exact, long arrays as a
fixed sample, within its size budget and identically from run to run."""
import os

import numpy as np

import bench


def load(d, name):
    return np.load(os.path.join(d, name + ".npy"))


def test_dump_outputs_exact_and_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 3 * 1000)   # 1000 elements per array for three arrays
    rng = np.random.default_rng(7)
    arrays = {"off": np.arange(1000, dtype=np.uint64) << np.uint64(33),   # u64 offsets past 2^32, below 2^53
              "arena": np.arange(5003, dtype=np.int32) * 3 - 5,           # strictly increasing: value -> position
              "dep_txn": rng.integers(0, 1 << 32, 4097, dtype=np.uint64).astype(np.uint32)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    names = sorted(arrays)
    assert sorted(os.listdir(a)) == sorted([n + ".npy" for n in names] + ["sizes.npy"])
    total = 0
    for n in names:
        x, y = load(a, n), load(b, n)
        assert x.dtype == np.float64 and np.array_equal(x, y)
        assert len(x) == min(len(arrays[n]), 1000)
        total += x.nbytes
    assert total <= bench.DUMP_BYTES
    assert np.array_equal(load(a, "sizes"), np.array([5003, 4097, 1000], np.float64))
    # the short array whole and exact
    assert np.array_equal(load(a, "off").astype(np.uint64), arrays["off"])
    # a sampled one: elements of its array at non-decreasing positions that spread over the whole array
    s = load(a, "arena")
    pos = (s + 5) / 3
    assert np.array_equal(pos, np.round(pos)) and pos.min() >= 0 and pos.max() < 5003
    assert np.all(np.diff(pos) >= 0) and pos.min() < 500 and pos.max() > 4500 and len(np.unique(pos)) > 800
    # both sampled arrays of different lengths are sampled on their own length
    d = load(a, "dep_txn")
    assert np.all(np.isin(d, arrays["dep_txn"].astype(np.float64)))
    # another value at a sampled position shows in the dump
    changed = dict(arrays, arena=arrays["arena"].copy())
    changed["arena"][int(pos[0])] += 1
    bench.dump_outputs(b, changed)
    assert not np.array_equal(s, load(b, "arena"))


def test_dump_outputs_wide_values_split(tmp_path):
    """64-bit values float64 cannot hold go out as two exact 32-bit halves; a change in the lowest bit shows."""
    wide = np.array([0, 1, (1 << 53) + 1, (1 << 64) - 1, 0x0123456789ABCDEF], np.uint64)
    signed = np.array([-(1 << 62) - 1, 5], np.int64)
    small = np.array([0, (1 << 53) - 1], np.uint64)
    d = str(tmp_path / "d")
    bench.dump_outputs(d, {"wide": wide, "signed": signed, "small": small})
    assert sorted(os.listdir(d)) == ["signed_hi.npy", "signed_lo.npy", "sizes.npy", "small.npy", "wide_hi.npy",
                                     "wide_lo.npy"]
    hi, lo = load(d, "wide_hi").astype(np.uint64), load(d, "wide_lo").astype(np.uint64)
    assert np.array_equal((hi << np.uint64(32)) | lo, wide)
    hi, lo = load(d, "signed_hi").astype(np.uint64), load(d, "signed_lo").astype(np.uint64)
    assert np.array_equal(((hi << np.uint64(32)) | lo).view(np.int64), signed)
    assert np.array_equal(load(d, "small").astype(np.uint64), small)
    e = str(tmp_path / "e")
    bench.dump_outputs(e, {"wide": wide ^ np.uint64(1), "signed": signed, "small": small})
    assert not np.array_equal(load(d, "wide_lo"), load(e, "wide_lo"))
    assert np.array_equal(load(d, "wide_hi"), load(e, "wide_hi"))
