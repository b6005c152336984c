"""A plain-Python model of the range-command store with each command's state (acc_rcmd_update_cmds), and what the
recovery scans over it must give: test_rcmd_gpu.Model (the ranges fold) plus the state rules of the header, per TxnId
in array order:
  status, executeAt   those of the last update that carried state (an update after erasure changes nothing);
  deps, HAS_DEPS      those of the last update without ACC_RCMD_KEEP_DEPS; an erasing update drops them;
  plain update        a new row starts at status 0, executeAt = its raw TxnId, no deps; an existing row keeps its state.
The expected side of every scan is oracle.map_reduce_full_ranges over cmds() (rows in TxnId order, erased rows flagged
and without ranges, no historical rows) with is_range = the query's domain bit."""
import numpy as np

import oracle
from accord_amd import _lib as L
from accord_amd.deps import mixed_queries_from_preaccept
from recovery_cases import rangedeps_as_dict
from test_rcmd_gpu import Model, ident

ERASED, HAS_DEPS, KEEP_DEPS = L.ACC_RCMD_ERASED, L.ACC_RCMD_HAS_DEPS, L.ACC_RCMD_KEEP_DEPS
DEP_COLS = (("dep_msb", np.uint64), ("dep_lsb", np.uint64), ("dep_node", np.int32), ("dep_start", np.uint64),
            ("dep_end", np.uint64), ("dep_is_key", np.uint8))
STATE_FIELDS = ("xmsb", "xlsb", "xnode", "status", "flags", "dep_off") + tuple(k for k, _ in DEP_COLS)
TABLE_FIELDS = ("msb", "lsb", "node", "flags", "rng_off", "rng_start", "rng_end", "dict_start", "dict_end")


class StateModel(Model):
    def __init__(self, end_inclusive):
        super().__init__(end_inclusive)
        self.state = {}   # identity -> dict(status, ex, hd, deps[(m, l, n, s, e, k)])

    def apply(self, upd):
        carries = upd.get("status") is not None
        erased = {k: c[1] for k, c in self.cmd.items()}
        flags = upd["flags"] if upd.get("flags") is not None else np.zeros(len(upd["msb"]), np.uint8)
        for u in range(len(upd["msb"])):
            t = (int(upd["msb"][u]), int(upd["lsb"][u]), int(upd["node"][u]))
            if not t[1] & 1:
                continue
            k = ident(t)
            s = self.state.setdefault(k, dict(status=0, ex=t, hd=0, deps=[]))
            if erased.get(k):
                continue
            if carries:
                s["status"] = int(upd["status"][u])
                s["ex"] = t if upd.get("xmsb") is None else (int(upd["xmsb"][u]), int(upd["xlsb"][u]), int(upd["xnode"][u]))
            f = int(flags[u])
            if f & ERASED:
                erased[k] = True
                s["deps"], s["hd"] = [], 0
            elif carries and not f & KEEP_DEPS:
                a, b = (int(upd["dep_off"][u]), int(upd["dep_off"][u + 1])) if upd.get("dep_off") is not None else (0, 0)
                s["deps"] = [tuple(int(upd[c][j]) for c, _ in DEP_COLS) for j in range(a, b)]
                s["hd"] = f & HAS_DEPS
        # the ranges fold knows ERASED alone
        super().apply(dict(upd, flags=np.asarray(flags, np.uint8) & np.uint8(ERASED)))

    def keys(self):
        return sorted(self.cmd, key=lambda k: (k[0], k[1], k[2]))

    def table(self):
        t = super().table()
        t["flags"] = t["flags"] | np.array([self.state[k]["hd"] for k in self.keys()], np.uint8)
        return t

    def state_cols(self):
        rows = [self.state[k] for k in self.keys()]
        out = dict(xmsb=np.array([r["ex"][0] for r in rows], np.uint64), xlsb=np.array([r["ex"][1] for r in rows], np.uint64),
                   xnode=np.array([r["ex"][2] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.uint8),
                   flags=self.table()["flags"],
                   dep_off=np.concatenate([[0], np.cumsum([len(r["deps"]) for r in rows])]).astype(np.uint32))
        deps = [d for r in rows for d in r["deps"]]
        for i, (c, dt) in enumerate(DEP_COLS):
            out[c] = np.array([d[i] for d in deps], dt)
        return out

    def cmds(self):
        """the model as the table oracle.map_reduce_full_ranges reads"""
        return cmds_of(self.table(), self.state_cols(), self.ei)


def cmds_of(tab, st, end_inclusive):
    c = dict(end_inclusive=end_inclusive, txn_msb=tab["msb"], txn_lsb=tab["lsb"], txn_node=tab["node"], exe_msb=st["xmsb"],
             exe_lsb=st["xlsb"], exe_node=st["xnode"], status=st["status"], flags=st["flags"], rng_off=tab["rng_off"],
             rng_start=tab["rng_start"], rng_end=tab["rng_end"], dep_off=st["dep_off"])
    for k, _ in DEP_COLS:
        c[k] = st[k]
    return c


def assert_store(store, model, msg=""):
    tab, st = store.table(), store.state()
    want_t, want_s = model.table(), model.state_cols()
    for f in TABLE_FIELDS:
        np.testing.assert_array_equal(tab[f], want_t[f], err_msg=f"{msg}: table {f}")
    for f in STATE_FIELDS:
        np.testing.assert_array_equal(st[f], want_s[f], err_msg=f"{msg}: state {f}")
    return tab, st


def domain_queries(q):
    """recovery queries (msb, lsb, node, is_range, part_*) with each X's domain bit set to its is_range: the domain bit
    is outside Timestamp.compareTo, and the resident entry reads it as the participants' domain"""
    lsb = (np.asarray(q["lsb"], np.uint64) & ~np.uint64(1)) | np.asarray(q["is_range"], np.uint64)
    return dict(q, lsb=lsb)


def mixed(q):
    """the same queries as the dict RangeCmdStore.map_reduce_full takes"""
    return mixed_queries_from_preaccept(q)


def as_txn_dicts(res, nq, tab):
    ids = list(zip(tab["msb"].tolist(), tab["lsb"].tolist(), tab["node"].tolist()))
    return [{r: [ids[i] for i in deps] for r, deps in rangedeps_as_dict(res, i_q).items()} for i_q in range(nq)]


def expect(cmds, q, params, test_kinds=-1):
    sa, td, ts, after = params
    tab = dict(msb=cmds["txn_msb"], lsb=cmds["txn_lsb"], node=cmds["txn_node"])
    return as_txn_dicts(oracle.map_reduce_full_ranges(cmds, q, sa, td, ts, test_kinds, after), len(q["msb"]), tab)


def check_scan(store, model_cmds, q, params, test_kinds=-1, msg=""):
    """one scan of the resident store against the oracle over the model; returns the per-query dicts"""
    sa, td, ts, after = params
    got = store.map_reduce_full(mixed(q), sa, td, ts, test_kinds=test_kinds, executes_after=after)
    tab = dict(msb=model_cmds["txn_msb"], lsb=model_cmds["txn_lsb"], node=model_cmds["txn_node"])
    g = as_txn_dicts(got, len(q["msb"]), tab)
    want = expect(model_cmds, q, params, test_kinds)
    assert g == want, f"{msg}: params {params} kinds {test_kinds}"
    assert [int(x) for x in np.diff(got.u_off.astype(np.int64)) > 0] == [int(bool(w)) for w in want], msg
    return g


def updates_from_cmds(cmds, rows, flags=None, status=None):
    """rows of an oracle-layout table as one RangeCmdStore.update batch with state columns, in the order given"""
    rows = [int(r) for r in rows]
    ro, do = cmds["rng_off"].astype(np.int64), cmds["dep_off"].astype(np.int64)
    rsel = np.concatenate([np.arange(ro[r], ro[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    dsel = np.concatenate([np.arange(do[r], do[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    csum = lambda off: np.concatenate([[0], np.cumsum([off[r + 1] - off[r] for r in rows])]).astype(np.uint32)  # noqa: E731
    upd = dict(msb=cmds["txn_msb"][rows], lsb=cmds["txn_lsb"][rows], node=cmds["txn_node"][rows],
               flags=cmds["flags"][rows] if flags is None else np.asarray(flags, np.uint8),
               rng_off=csum(ro), rng_start=cmds["rng_start"][rsel], rng_end=cmds["rng_end"][rsel],
               status=cmds["status"][rows] if status is None else np.asarray(status, np.uint8),
               xmsb=cmds["exe_msb"][rows], xlsb=cmds["exe_lsb"][rows], xnode=cmds["exe_node"][rows], dep_off=csum(do))
    for k, _ in DEP_COLS:
        upd[k] = cmds[k][dsel]
    return upd


def handmade():
    """recovery_cases.range_recovery_handmade() without its historical row: T2, T4, T6 at table indices 0, 1, 2 and
    X = hlc 5, a Write over [0, 100), StartInclusive, its domain bit set (it lists a range). The nine answers by hand:
      0  T2  Accepted,  executeAt T2,     [10, 20), deps {X: key 15}
      1  T4  Committed, executeAt hlc 9,  [30, 40), no deps
      2  T6  Stable,    executeAt T6,     [10, 20), deps {X: range [0, 12)}
    all Writes (witnessedBy(Write) holds them all), all with HAS_DEPS."""
    from recovery_cases import range_recovery_handmade
    c, q, _ = range_recovery_handmade()
    keep = [0, 2, 3]
    cmds = dict(end_inclusive=c["end_inclusive"])
    for k in ("txn_msb", "txn_lsb", "txn_node", "exe_msb", "exe_lsb", "exe_node", "status", "flags", "rng_start", "rng_end"):
        cmds[k] = c[k][keep]                                   # one range per row
    cmds["rng_off"] = np.array([0, 1, 2, 3], np.uint32)
    cmds["dep_off"] = np.array([0, 1, 1, 2], np.uint32)        # the historical row held no deps
    for k, _ in DEP_COLS:
        cmds[k] = c[k]
    q = domain_queries(q)
    expected = {
        # T2 executes before X (executeAt >= X fails under WITHOUT); T4: Committed, X not in its deps, executes at 9 > 5
        (0, 1, 1, True): {(30, 40): [1]},
        # after X only T6, which is Stable, not Accepted / PreCommitted / Committed
        (1, 1, 1, False): {},
        # T6: Stable, executeAt T6 >= X, X's range [0, 12) intersects [10, 20); T2 executes before X, T4 is not Stable
        (2, 0, 2, False): {(10, 20): [2]},
        # before X: T2 executes before X, T4 is not Stable
        (0, 0, 2, False): {},
        # the only Stable command witnessed X
        (2, 1, 2, False): {},
        # no test but the kind: every command, per range
        (2, 2, 0, False): {(10, 20): [0, 2], (30, 40): [1]},
        (0, 2, 0, False): {(10, 20): [0], (30, 40): [1]},
        (1, 2, 0, False): {(10, 20): [2]},
        # T2 witnessed X but executes before it; T4 holds no deps of X
        (0, 0, 1, False): {},
    }
    return cmds, q, expected


ALL_PARAMS =[(sa, td, ts, after) for sa in range(3) for td in range(3) for ts in range(3) for after in (False, True)]
