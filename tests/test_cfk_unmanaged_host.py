"""Host side of acc_cfk_register_unmanaged / acc_cfk_notify_unmanaged / acc_cfk_unmanaged_view (no GPU): the ctypes
mirrors against the header's declarations, the exports and prototypes, the constants, the Python entry points'
signatures, and the constants the tests name against the kernel source."""
import ctypes as C
import inspect
import re
from pathlib import Path

import cfk_unmanaged_cases as UC
import cfk_unmanaged_model as UM
from accord_amd import _lib as L
from accord_amd.deps import CfkStore, ReplicaStore
from test_cfk_redundant_host import HEADER, header_fields

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "cassandra-accord_amd" / "csrc"


def offsets(struct, names):
    return {n: getattr(struct, n).offset for n in names}


def test_unmanaged_in_layout_matches_the_header():
    names = header_fields("acc_cfk_unmanaged_in")
    assert names == [f[0] for f in L.CfkUnmanagedIn._fields_]
    # u32 x2 | u64 x2 | two acc_ts_cols (3 pointers each) | 3 pointers | acc_ts_cols | u32, padding to 8
    assert offsets(L.CfkUnmanagedIn, names) == dict(mem=0, n_waiters=4, n_pairs=8, n_deps=16, txn_id=24, execute_at=48, key_off=72,
                                                    key=80, dep_off=88, deps=96, tier=120)
    assert C.sizeof(L.CfkUnmanagedIn) == 128


def test_unmanaged_out_and_table_layouts_match_the_header():
    names = header_fields("acc_cfk_unmanaged_out")
    assert names == [f[0] for f in L.CfkUnmanagedOut._fields_]
    assert offsets(L.CfkUnmanagedOut, names) == dict(n_pairs=0, n_inserted=8, outcome=16, until=24)
    assert C.sizeof(L.CfkUnmanagedOut) == 48
    names = header_fields("acc_cfk_unmanaged_table")
    assert names == [f[0] for f in L.CfkUnmanagedTable._fields_]
    assert offsets(L.CfkUnmanagedTable, names) == dict(n_rec=0, n_deps=8, key=16, pending=24, until=32, txn_id=56, execute_at=80,
                                                       dep_off=104, deps=112)
    assert C.sizeof(L.CfkUnmanagedTable) == 136


def test_notify_in_and_events_layouts_match_the_header():
    names = header_fields("acc_cfk_unmanaged_notify_in")
    assert names == [f[0] for f in L.CfkUnmanagedNotifyIn._fields_]
    assert offsets(L.CfkUnmanagedNotifyIn, names) == dict(mem=0, n_keys=4, key_code=8)
    assert C.sizeof(L.CfkUnmanagedNotifyIn) == 16
    names = header_fields("acc_cfk_unmanaged_events")
    assert names == [f[0] for f in L.CfkUnmanagedEvents._fields_]
    assert offsets(L.CfkUnmanagedEvents, names) == dict(n_events=0, n_rec=4, ev_kind=8, ev_flags=16, ev_key=24, ev_txn=32, ev_until=56)
    assert C.sizeof(L.CfkUnmanagedEvents) == 80


def test_exports_prototypes_and_constants():
    protos = {
        "acc_cfk_register_unmanaged": r"\(acc_ctx \*ctx, acc_cfk \*cfk, const acc_cfk_unmanaged_in \*in, acc_cfk_unmanaged_out \*out\);",
        "acc_cfk_notify_unmanaged":
            r"\(acc_ctx \*ctx, acc_cfk \*cfk, const acc_cfk_unmanaged_notify_in \*in, acc_cfk_unmanaged_events \*out\);",
        "acc_cfk_unmanaged_view": r"\(acc_ctx \*ctx, acc_cfk \*cfk, acc_cfk_unmanaged_table \*out\);"}
    for name, args in protos.items():
        assert name in L.EXPORTS
        assert re.search(r"int\s+%s%s" % (name, args), HEADER), name
    define = lambda name: int(re.search(r"#define %s\s+(\w+)" % name, HEADER).group(1).rstrip("u"), 0)  # noqa: E731
    for name in ("ACC_UNM_COMMIT", "ACC_UNM_APPLY", "ACC_UNM_READY", "ACC_UNM_PENDING_COMMIT", "ACC_UNM_PENDING_APPLY",
                 "ACC_UNM_TIER_LANE", "ACC_UNM_TIER_WAVE", "ACC_UNM_EV_TO_APPLY", "ACC_UNM_EV_RELEASE"):
        assert define(name) == getattr(L, name)
    assert (UM.COMMIT, UM.APPLY) == (L.ACC_UNM_COMMIT, L.ACC_UNM_APPLY)
    assert (UM.READY, UM.PENDING_COMMIT, UM.PENDING_APPLY) == (L.ACC_UNM_READY, L.ACC_UNM_PENDING_COMMIT, L.ACC_UNM_PENDING_APPLY)
    assert (UM.EV_TO_APPLY, UM.EV_RELEASE) == (L.ACC_UNM_EV_TO_APPLY, L.ACC_UNM_EV_RELEASE)


def test_named_kernel_constants_and_build_list():
    src = (CSRC / "cfkunmanaged.hip").read_text()
    assert int(re.search(r"constexpr uint32_t UM_LANE_MAX = (\d+);", src).group(1)) == UC.UM_LANE_MAX
    assert "namespace um" in src
    mk = (ROOT / "cassandra-accord_amd" / "Makefile").read_text()
    assert "csrc/cfkunmanaged.hip" in mk and "csrc/cfkunmanaged.hpp" in mk


def test_the_header_no_longer_leaves_unmanaged_records_out():
    block = HEADER[HEADER.index("acc_cfk_notify reads the key-major state"):HEADER.index("#define ACC_NOTIFY_WAITING_TO_EXECUTE")]
    assert "Out of scope: Unmanaged" not in block and "acc_cfk_register_unmanaged" in block


def test_python_entry_points():
    p = inspect.signature(CfkStore.register_unmanaged).parameters
    assert list(p) == ["self", "waiters", "tier"] and p["tier"].default == 0
    p = inspect.signature(CfkStore.notify_unmanaged).parameters
    assert list(p) == ["self", "keys"] and p["keys"].default is None
    assert list(inspect.signature(CfkStore.unmanaged).parameters) == ["self"]
    assert list(inspect.signature(ReplicaStore.register_unmanaged).parameters) == ["self", "waiters"]
    p = inspect.signature(ReplicaStore.notify_unmanaged).parameters
    assert list(p) == ["self", "keys"] and p["keys"].default is None
    assert list(inspect.signature(ReplicaStore.preaccept_batch).parameters)[-1] == "notify"
