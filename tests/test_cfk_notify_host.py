"""Host side of acc_cfk_notify (no GPU): the ctypes mirrors against the header's declarations, the export and prototype,
the constants, the Python entry points' signatures, and the constants the tests name against the kernel source."""
import ctypes as C
import inspect
import re
from pathlib import Path

import cfk_notify_cases as NC
import cfk_notify_model as NM
from accord_amd import _lib as L
from accord_amd.deps import CfkStore, ReplicaStore
from test_cfk_redundant_host import HEADER, header_fields

CSRC = Path(__file__).resolve().parent.parent / "cassandra-accord_amd" / "csrc"


def test_notify_in_layout_matches_the_header():
    names = header_fields("acc_cfk_notify_in")
    assert names == [f[0] for f in L.CfkNotifyIn._fields_]
    # u32 x2 | pointer | u32, padding to 8
    assert {n: getattr(L.CfkNotifyIn, n).offset for n in names} == dict(mem=0, n_keys=4, key_code=8, tier=16)
    assert C.sizeof(L.CfkNotifyIn) == 24


def test_notify_view_layout_matches_the_header():
    names = header_fields("acc_cfk_notify_view")
    assert names == [f[0] for f in L.CfkNotifyView._fields_]
    offsets = dict(n_keys=0, n_txn=4, n_events=8, min_uncommitted=16, next=24, next_write=32, ev_off=40, ev_entry=48, ev_txn=56,
                   ev_pos=64, ev_kind=72, rel_keys=80)
    assert {n: getattr(L.CfkNotifyView, n).offset for n in names} == offsets
    assert C.sizeof(L.CfkNotifyView) == 88


def test_export_prototype_and_constants():
    assert "acc_cfk_notify" in L.EXPORTS
    assert re.search(r"int\s+acc_cfk_notify\(acc_ctx \*ctx, acc_cfk \*cfk, const acc_cfk_notify_in \*in, acc_cfk_notify_view \*out\);",
                     HEADER)
    define = lambda name: int(re.search(r"#define %s\s+(\w+)" % name, HEADER).group(1).rstrip("u"), 0)  # noqa: E731
    for name in ("ACC_NOTIFY_WAITING_TO_EXECUTE", "ACC_NOTIFY_RELEASE", "ACC_NOTIFY_NONE", "ACC_NOTIFY_TIER_LANE",
                 "ACC_NOTIFY_TIER_WAVE", "ACC_NOTIFY_TIER_SORT"):
        assert define(name) == getattr(L, name)
    assert (NM.WAITING_TO_EXECUTE, NM.RELEASE, NM.NONE) == (L.ACC_NOTIFY_WAITING_TO_EXECUTE, L.ACC_NOTIFY_RELEASE, L.ACC_NOTIFY_NONE)


def test_named_kernel_constants():
    src = (CSRC / "cfknotify.hip").read_text()
    const = lambda name, text: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))  # noqa: E731
    for name in ("NT_LANE_MAX", "NT_LANE_FORCE_MAX", "NT_WAVE_MAX"):
        assert const(name, src) == getattr(NC, name)
    # the u32 scan tile: BLOCK threads x 32 items (csrc/prims.hpp, scan_multi; csrc/ctx.hpp, BLOCK)
    assert re.search(r"constexpr int ITEMS = sizeof\(T\) == 8 \? 16 : 32;", (CSRC / "prims.hpp").read_text())
    assert re.search(r"constexpr int BLOCK = 256;", (CSRC / "ctx.hpp").read_text())
    assert NC.SCAN_TILE == 256 * 32


def test_python_entry_points():
    p = inspect.signature(CfkStore.notify).parameters
    assert list(p) == ["self", "keys", "tier"] and p["keys"].default is None and p["tier"].default == 0
    p = inspect.signature(ReplicaStore.notify).parameters
    assert list(p) == ["self", "keys"] and p["keys"].default is None
    p = inspect.signature(ReplicaStore.preaccept_batch).parameters
    assert list(p)[-1] == "notify" and p["notify"].default is False
