"""Host side of the range-command store's state columns and recovery scans (acc_rcmd_update_cmds, acc_rcmd_state_view,
acc_rcmd_map_reduce_full; no GPU): the ctypes mirrors against the header's field lists, offsets and sizes, the exports
and prototypes, the structs existing tests pin left as they were, and the Python model of the store
(rcmd_state_model.py) against the hand-worked table."""
import ctypes as C
import re

import numpy as np

import oracle
import rcmd_state_model as M
from accord_amd import _lib as L
from recovery_cases import rangedeps_as_dict
from test_rcmd_host import HEADER, field_names


def test_rcmd_cmd_updates_layout_matches_the_header():
    S = L.RcmdCmdUpdates
    assert field_names("acc_rcmd_cmd_updates") == [f[0] for f in S._fields_]
    # the fields of acc_rcmd_updates first, at its offsets
    for (name, _), (name2, _) in zip(L.RcmdUpdates._fields_, S._fields_):
        assert name == name2 and getattr(L.RcmdUpdates, name).offset == getattr(S, name).offset
    assert S.execute_at.offset == 72 and S.status.offset == 96 and S.n_deps.offset == 104 and S.dep_off.offset == 112
    assert S.dep_txn.offset == 120 and S.dep_start.offset == 144 and S.dep_end.offset == 152 and S.dep_is_key.offset == 160
    assert C.sizeof(S) == 168


def test_rcmd_state_layout_matches_the_header():
    S = L.RcmdState
    assert field_names("acc_rcmd_state") == [f[0] for f in S._fields_]
    assert S.n_cmd.offset == 0 and S.n_deps.offset == 8 and S.execute_at.offset == 16 and S.status.offset == 40
    assert S.flags.offset == 48 and S.dep_off.offset == 56 and S.dep_txn.offset == 64 and S.dep_start.offset == 88
    assert S.dep_end.offset == 96 and S.dep_is_key.offset == 104
    assert C.sizeof(S) == 112


def test_exports_and_prototypes():
    for n in ("acc_rcmd_update_cmds", "acc_rcmd_state_view", "acc_rcmd_map_reduce_full"):
        assert n in L.EXPORTS
        assert re.search(r"\b%s\(" % n, HEADER)
    assert re.search(r"int\s+acc_rcmd_update_cmds\(acc_ctx \*ctx, acc_rcmd \*store, const acc_rcmd_cmd_updates \*updates\);", HEADER)
    assert re.search(r"int\s+acc_rcmd_state_view\(acc_ctx \*ctx, acc_rcmd \*store, acc_rcmd_state \*out\);", HEADER)
    # the scan takes the query struct of acc_cfk_map_reduce_full: one query batch serves both halves of mapReduceFull
    assert re.search(r"int\s+acc_rcmd_map_reduce_full\(acc_ctx \*ctx, acc_rcmd \*store, const acc_cfk_recovery_in \*q,\s*"
                     r"acc_rangedeps_view \*out_view\);", HEADER)


def test_pinned_structs_are_untouched():
    assert C.sizeof(L.RcmdUpdates) == 72
    assert C.sizeof(L.RcmdTable) == 96
    assert C.sizeof(L.Opts) == 24


def test_keep_deps_flag():
    assert re.search(r"#define\s+ACC_RCMD_KEEP_DEPS\s+8u", HEADER) and L.ACC_RCMD_KEEP_DEPS == 8
    assert len({L.ACC_RCMD_ERASED, L.ACC_RCMD_HAS_DEPS, L.ACC_RCMD_HISTORICAL, L.ACC_RCMD_KEEP_DEPS}) == 4
    assert re.search(r"historicalRangeCommands stay unmodelled", HEADER)


def test_model_on_the_hand_worked_table():
    """The model fed the hand-worked rows in two batches (the second out of TxnId order) holds the table the oracle
    reads, and the oracle over it gives the nine answers derived by hand in rcmd_state_model.handmade."""
    cmds, q, expected = M.handmade()
    m = M.StateModel(0)
    m.apply(M.updates_from_cmds(cmds, [1]))
    m.apply(M.updates_from_cmds(cmds, [2, 0]))
    got = m.cmds()
    for k, v in cmds.items():
        np.testing.assert_array_equal(got[k], v, err_msg=k)
    assert len(expected) == 9
    for (sa, td, ts, after), want in expected.items():
        res = oracle.map_reduce_full_ranges(got, q, sa, td, ts, -1, after)
        assert rangedeps_as_dict(res, 0) == want, (sa, td, ts, after)


def test_model_state_rules():
    """KEEP_DEPS, erasure and plain updates in the model, on one TxnId listed several times"""
    cmds, _, _ = M.handmade()
    m = M.StateModel(0)
    u = M.updates_from_cmds(cmds, [0, 0], flags=[L.ACC_RCMD_KEEP_DEPS, L.ACC_RCMD_HAS_DEPS | L.ACC_RCMD_KEEP_DEPS], status=[1, 2])
    m.apply(u)                                                  # KEEP_DEPS on a new command: no deps, HAS_DEPS clear
    s = m.state_cols()
    assert s["status"].tolist() == [2] and s["flags"].tolist() == [0] and s["dep_off"].tolist() == [0, 0]
    m.apply(M.updates_from_cmds(cmds, [0]))                     # deps arrive
    m.apply(M.updates_from_cmds(cmds, [0], flags=[L.ACC_RCMD_KEEP_DEPS], status=[7]))
    s = m.state_cols()
    assert s["status"].tolist() == [7] and s["flags"].tolist() == [L.ACC_RCMD_HAS_DEPS] and s["dep_off"].tolist() == [0, 1]
    plain = {k: v for k, v in M.updates_from_cmds(cmds, [0, 1]).items() if k in ("msb", "lsb", "node", "rng_off", "rng_start", "rng_end")}
    m.apply(dict(plain, flags=np.zeros(2, np.uint8)))           # plain: the stored state stays, the new row is NotDefined
    s = m.state_cols()
    assert s["status"].tolist() == [7, 0] and s["dep_off"].tolist() == [0, 1, 1]
    assert (int(s["xmsb"][1]), int(s["xlsb"][1]), int(s["xnode"][1])) == tuple(int(cmds[k][1]) for k in ("txn_msb", "txn_lsb", "txn_node"))
    m.apply(M.updates_from_cmds(cmds, [0, 0], flags=[L.ACC_RCMD_ERASED, L.ACC_RCMD_HAS_DEPS], status=[9, 3]))
    s = m.state_cols()                                          # erased: its own status, no deps; the later update ignored
    assert s["status"].tolist() == [9, 0] and s["flags"].tolist() == [L.ACC_RCMD_ERASED, 0] and s["dep_off"].tolist() == [0, 0, 0]
    assert m.stats["erased_ignored"] == 1
