"""Host side of acc_cfk_map_reduce_full (no GPU): the ctypes mirror of acc_cfk_recovery_in against the header's
declaration, the export, acc_opts left as it was, and the Python entry points' signatures."""
import ctypes as C
import inspect
import re
from pathlib import Path

from accord_amd import _lib as L
from accord_amd.deps import CfkStore, ReplicaStore

HEADER = (Path(__file__).resolve().parent.parent / "include" / "accord_amd.h").read_text()


def test_cfk_recovery_in_layout_matches_the_header():
    body = re.search(r"typedef struct acc_cfk_recovery_in \{(.*?)\} acc_cfk_recovery_in;", HEADER, re.S).group(1)
    names = []
    for decl in re.findall(r"([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        names += [part.split()[-1].strip("*") for part in decl.split(",")]   # `type a, b;` -> a, b
    assert names == [f[0] for f in L.CfkRecoveryIn._fields_]
    # u32 x2 | u64 x2 | three pointers | five pointers | u32 | u8 x4 | i32 | tail padding to 8
    offsets = dict(n_query=0, mem=4, n_pairs=8, n_ranges=16, test_txn=24, key_off=48, key_code=56, rng_off=64, rng_start=72,
                   rng_end=80, end_inclusive=88, started_at=92, test_dep=93, test_status=94, flags=95, test_kinds=96)
    assert {n: getattr(L.CfkRecoveryIn, n).offset for n in names} == offsets
    assert C.sizeof(L.CfkRecoveryIn) == 104
    # the call-wide tests are exactly acc_recovery_in's
    for f in ("started_at", "test_dep", "test_status", "flags", "test_kinds"):
        assert dict(L.CfkRecoveryIn._fields_)[f] is dict(L.RecoveryIn._fields_)[f]


def test_export_and_prototype():
    assert "acc_cfk_map_reduce_full" in L.EXPORTS
    assert re.search(r"int\s+acc_cfk_map_reduce_full\(acc_ctx \*ctx, acc_cfk \*cfk, const acc_cfk_recovery_in \*q,\s*"
                     r"acc_keydeps_view \*out_view\);", HEADER)


def test_opts_keeps_its_size():
    assert C.sizeof(L.Opts) == 24
    assert [f[0] for f in L.Opts._fields_][-1] == "cfq_wave_cap"


def test_python_entry_points():
    p = inspect.signature(CfkStore.map_reduce_full).parameters
    assert list(p) == ["self", "queries", "started_at", "test_dep", "test_status", "test_kinds", "executes_after", "end_inclusive"]
    assert p["test_kinds"].default == -1 and p["executes_after"].default is False and p["end_inclusive"].default == 1
    for name in ("queries", "started_at", "test_dep", "test_status"):
        assert p[name].default is inspect.Parameter.empty
    assert list(inspect.signature(ReplicaStore.begin_recovery).parameters) == ["self", "queries"]
    # the four scans begin_recovery runs are the four of BeginRecovery.java:334, 348, 365, 378
    assert L.RECOVERY_SCANS["acceptedOrCommittedStartedBeforeWithoutWitnessing"] == (
        L.ACC_STARTED_BEFORE, L.ACC_DEP_WITHOUT, L.ACC_STATUS_IS_PROPOSED, True)
    assert L.RECOVERY_SCANS["stableStartedBeforeAndWitnessed"] == (L.ACC_STARTED_BEFORE, L.ACC_DEP_WITH, L.ACC_STATUS_IS_STABLE, False)
