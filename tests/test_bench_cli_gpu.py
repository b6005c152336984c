"""GPU: bench.py's command line at reduced size. A plain run prints the headline fields only and --dump-outputs writes
each config's result arrays (names, and lengths that agree with the offsets and with the result line); --full keeps
the roofline and the further legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "cpu_baseline", "cfk_apply", "cfk_steady", "keydeps_mixed", "partial_deps", "kernels_ms_per_step"}


def bench_line(*args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        *args], capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def dump(d):
    names = sorted(f[:-4] for f in os.listdir(d) if f != "sizes.npy")
    arrays = {n: np.load(os.path.join(d, n + ".npy")) for n in names}
    assert all(a.dtype == np.float64 for a in arrays.values())
    sizes = dict(zip(names, np.load(os.path.join(d, "sizes.npy")).astype(np.int64)))
    # an array is whole up to its share of the dump's budget and a sample of that length beyond it (the per-txn
    # offsets and levels that the checks below read whole are far below it at these sizes)
    cap = bench.DUMP_BYTES // 8 // len(names)
    assert {n: len(arrays[n]) for n in names} == {n: min(sizes[n], cap) for n in names}
    return arrays, sizes


def check_plain(line):
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["higher_is_better"] is True


@pytest.mark.gpu
def test_plain_config2_dump(tmp_path):
    line, _ = bench_line("--scale", "0.02", "--dump-outputs", str(tmp_path))
    check_plain(line)
    a, n = dump(str(tmp_path))
    assert sorted(a) == ["arena", "arena_off", "dep_txn", "kd_off", "key_idx", "u_off"]
    nt = line["config"]["n_txn_per_gpu"]
    assert nt == 20_000 and n["arena_off"] == n["kd_off"] == n["u_off"] == nt + 1
    assert (a["arena_off"][-1], a["kd_off"][-1], a["u_off"][-1]) == (n["arena"], n["key_idx"], n["dep_txn"])
    assert n["arena"] == n["key_idx"] + line["config"]["dep_edges_per_gpu"] and line["config"]["dep_edges_per_gpu"] > 0
    # ms_per_step is printed to 3 decimals: value agrees with it within that rounding
    assert line["value"] == pytest.approx(line["config"]["pairs_per_gpu"] / (line["ms_per_step"] / 1e3),
                                          rel=1e-3 / line["ms_per_step"] + 1e-6)


@pytest.mark.gpu
def test_plain_config4_dump(tmp_path):
    line, _ = bench_line("--config", "4", "--scale", "0.005", "--dump-outputs", str(tmp_path))
    check_plain(line)
    a, n = dump(str(tmp_path))
    assert sorted(a) == ["arena", "arena_off", "dep_txn", "range_id", "rd_off", "rng_end", "rng_start", "u_off"]
    nt = line["config"]["n_txn_per_gpu"]
    assert nt == 100_000 and n["arena_off"] == n["rd_off"] == n["u_off"] == nt + 1
    assert (a["arena_off"][-1], a["rd_off"][-1], a["u_off"][-1]) == (n["arena"], n["range_id"], n["dep_txn"])
    assert n["arena"] == n["range_id"] + line["config"]["dep_entries_per_gpu"]
    assert n["rng_start"] == n["rng_end"] > 0 and np.all(a["rng_start"] <= a["rng_end"])
    assert a["range_id"].max() < n["rng_start"]


@pytest.mark.gpu
def test_plain_config5_dump(tmp_path):
    line, _ = bench_line("--config", "5", "--scale", "0.125", "--dump-outputs", str(tmp_path))
    check_plain(line)
    a, n = dump(str(tmp_path))
    assert sorted(a) == ["k2v", "k2v_off", "key_code", "key_off", "level", "n_levels", "order", "txn_rank", "val_off"]
    nt = line["config"]["n_txn_per_gpu"]
    assert nt == 2048 and n["key_off"] == n["val_off"] == n["k2v_off"] == nt + 1 and n["level"] == n["order"] == nt
    assert (a["key_off"][-1], a["val_off"][-1], a["k2v_off"][-1]) == (n["key_code"], n["txn_rank"], n["k2v"])
    assert n["k2v"] == n["key_code"] + line["config"]["merged_entries_per_gpu"]
    assert a["n_levels"].tolist() == [line["config"]["levels"]] and a["level"].max() == line["config"]["levels"] - 1
    assert sorted(a["order"].tolist()) == list(range(nt))


@pytest.mark.gpu
def test_full_keeps_roofline_and_kernels():
    line, err = bench_line("--scale", "0.02", "--full", "--no-cpu", env={"ACC_BENCH_KERNELS": "1"})
    assert HEADLINE <= set(line) and "only matter with --full" not in err
    assert line["roofline"]["device_kernel_ms_per_step"] > 0 and line["roofline"]["dominant_kernel"]["name"]
    assert line["kernels_ms_per_step"] and "cpu_baseline" not in line


@pytest.mark.gpu
def test_plain_names_ignored_full_only_knobs():
    line, err = bench_line("--scale", "0.02", "--no-cpu", env={"ACC_BENCH_KERNELS": "1"})
    check_plain(line)
    note = [ln for ln in err.splitlines() if "only matter with --full" in ln]
    assert len(note) == 1 and "--no-cpu" in note[0] and "ACC_BENCH_KERNELS" in note[0]
