"""Host side of acc_waiting_* (no GPU): the ctypes mirrors against the header's declarations, the exports and prototypes,
the constants, the Python entry points' signatures, and the constants the tests name against the kernel source."""
import ctypes as C
import inspect
import re
from pathlib import Path

import waiting_cases as WC
import waiting_model as WM
from accord_amd import _lib as L
from accord_amd.deps import ReplicaStore, WaitingStore
from test_cfk_redundant_host import HEADER, header_fields

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "cassandra-accord_amd" / "csrc"


def check(struct, name, offsets, size):
    names = header_fields(name)
    assert names == [f[0] for f in struct._fields_], name
    assert {n: getattr(struct, n).offset for n in names} == offsets, name
    assert C.sizeof(struct) == size, name


def test_register_layouts_match_the_header():
    # u32 x2 | u64 x2 | two acc_ts_cols | 4 pointers | acc_ts_cols | pointer | u32, padding to 8
    check(L.WaitingRegisterIn, "acc_waiting_register_in",
          dict(mem=0, n_waiters=4, n_keys=8, n_deps=16, txn_id=24, execute_at=48, key_off=72, key=80, key_wait=88, dep_off=96,
               dep=104, dep_wait=128, tier=136), 144)
    check(L.WaitingRegisterOut, "acc_waiting_register_out", dict(n_waiters=0, reserved=4, waiting=8, execute_at_least=16), 40)


def test_notify_and_erase_layouts_match_the_header():
    check(L.WaitingNotifyIn, "acc_waiting_notify_in",
          dict(mem=0, n_changed=4, changed=8, n_rel=32, tier=36, rel_txn=40, rel_key=64, rel_flags=72, rel_until=80), 104)
    check(L.WaitingNotifyOut, "acc_waiting_notify_out",
          dict(n_ready=0, reserved=4, n_changed=8, ready_rec=16, ready_txn=24, ready_execute_at_least=48), 72)
    check(L.WaitingEraseIn, "acc_waiting_erase_in", dict(mem=0, n_ids=4, txn_id=8), 32)


def test_table_layout_matches_the_header():
    check(L.WaitingTable, "acc_waiting_table",
          dict(n_rec=0, reserved=4, n_keys=8, n_deps=16, txn_id=24, execute_at=48, execute_at_least=72, flags=96, key_off=104,
               key=112, key_wait=120, dep_off=128, dep=136, dep_state=160, n_wait_dep=168, n_wait_key=176, next_waiting_on=184), 192)


def test_exports_prototypes_and_constants():
    protos = {
        "acc_waiting_create": r"int\s+acc_waiting_create\(acc_ctx \*ctx, acc_waiting \*\*out\);",
        "acc_waiting_destroy": r"void\s+acc_waiting_destroy\(acc_waiting \*w\);",
        "acc_waiting_register": r"int\s+acc_waiting_register\(acc_ctx \*ctx, acc_waiting \*w, acc_rcmd \*rcmd, "
                                r"const acc_waiting_register_in \*in,\s+acc_waiting_register_out \*out\);",
        "acc_waiting_notify": r"int\s+acc_waiting_notify\(acc_ctx \*ctx, acc_waiting \*w, acc_rcmd \*rcmd, "
                              r"const acc_waiting_notify_in \*in,\s+acc_waiting_notify_out \*out\);",
        "acc_waiting_erase": r"int\s+acc_waiting_erase\(acc_ctx \*ctx, acc_waiting \*w, const acc_waiting_erase_in \*in\);",
        "acc_waiting_view": r"int\s+acc_waiting_view\(acc_ctx \*ctx, acc_waiting \*w, acc_waiting_table \*out\);"}
    for name, proto in protos.items():
        assert name in L.EXPORTS
        assert re.search(proto, HEADER), name
    define = lambda name: int(re.search(r"#define %s\s+(\w+)" % name, HEADER).group(1).rstrip("u"), 0)  # noqa: E731
    for name in ("ACC_WT_NOT_WAITING", "ACC_WT_WAITING", "ACC_WT_APPLIED_OR_INVALIDATED", "ACC_WT_AWAITS_ONLY_DEPS",
                 "ACC_WT_RANGE_DOMAIN", "ACC_WT_REL_KEY", "ACC_WT_NONE", "ACC_WT_TIER_LANE", "ACC_WT_TIER_WAVE"):
        assert define(name) == getattr(L, name), name
    assert (WM.NOT_WAITING, WM.WAITING, WM.APPLIED_OR_INVALIDATED) == (L.ACC_WT_NOT_WAITING, L.ACC_WT_WAITING,
                                                                        L.ACC_WT_APPLIED_OR_INVALIDATED)
    assert (WM.AWAITS_ONLY_DEPS, WM.RANGE_DOMAIN, WM.NONE) == (L.ACC_WT_AWAITS_ONLY_DEPS, L.ACC_WT_RANGE_DOMAIN, L.ACC_WT_NONE)


def test_named_kernel_constants_and_build_list():
    src = (CSRC / "waiting.hip").read_text()
    lane_max = int(re.search(r"constexpr uint32_t WT_LANE_MAX = (\d+);", src).group(1))
    assert {lane_max - 1, lane_max, lane_max + 1} <= set(WC.EDGE_DEPS)
    assert "namespace wt" in src
    mk = (ROOT / "cassandra-accord_amd" / "Makefile").read_text()
    assert "csrc/waiting.hip" in mk


def test_the_header_states_the_scope():
    block = HEADER[HEADER.index("Execution readiness from a resident WaitingOn store"):HEADER.index("#define ACC_WT_NOT_WAITING")]
    for text in ("removeRedundantDependencies", "isFullyPreBootstrapOrStale", "checkState (:793)", "progress log",
                 "SimpleBitSet.java:404-407", "descending slot order", "the convention for Erased"):
        assert text in block, text


def test_python_entry_points():
    assert list(inspect.signature(WaitingStore.__init__).parameters) == ["self", "ctx", "rcmd"]
    p = inspect.signature(WaitingStore.register).parameters
    assert list(p) == ["self", "waiters", "tier", "device"] and p["tier"].default == 0 and p["device"].default is False
    p = inspect.signature(WaitingStore.notify).parameters
    assert list(p) == ["self", "changed", "releases", "tier", "device"]
    assert p["changed"].default is None and p["releases"].default is None
    assert list(inspect.signature(WaitingStore.erase).parameters) == ["self", "ids", "device"]
    assert list(inspect.signature(WaitingStore.view).parameters) == ["self"]
    assert callable(WaitingStore.bitsets)
    assert list(inspect.signature(ReplicaStore.register_waiting).parameters) == ["self", "waiters"]
    p = inspect.signature(ReplicaStore.notify_waiting).parameters
    assert list(p) == ["self", "changed", "releases"] and p["changed"].default is None and p["releases"].default is None
    p = inspect.signature(ReplicaStore.execution_step).parameters
    assert list(p) == ["self", "keys", "changed"] and p["keys"].default is None and p["changed"].default is None
