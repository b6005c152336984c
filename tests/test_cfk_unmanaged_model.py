"""The host model of the Unmanaged pending records (cfk_unmanaged_model) pinned by literals worked by hand from
local/CommandsForKey.java, and the case families' conditions (cfk_unmanaged_cases.run_model). No GPU.

Key 500 holds Writes A < B < C < D (hlc 4, 8, 12, 16; executeAt = TxnId unless said). Waiters have hlc 23."""
import numpy as np
import pytest

import cfk_cases as CC
import cfk_unmanaged_cases as UC
import cfk_unmanaged_model as UM
import oracle
from cfk_unmanaged_cases import APPLIED, COMMITTED, EPHEMERAL_READ, EXCLUSIVE_SYNC_POINT, PRE, READ, STABLE, SYNC_POINT, ts

A, B, C, D, X = ts(4), ts(8), ts(12), ts(16), ts(6)
SP = ts(23, SYNC_POINT, 1, 1)
ESP = ts(23, EXCLUSIVE_SYNC_POINT, 1, 1)
RR = ts(23, READ, 1, 1)


def cfk(rows, pending=(), bound=UM.ZERO):
    """rows: [(raw id, status, raw executeAt or None)]"""
    return UM.Cfk(500, [UM.Info(t, st, t if x is None else x, []) for t, st, x in rows], list(pending), bound)


def ids(c):
    return [(t.raw_id, t.status) for t in c.txns]


BASE = [(A, APPLIED, None), (B, COMMITTED, None), (C, PRE, None)]


def test_compare_to():
    """:155-162: COMMIT before APPLY whatever the timestamps; then waitingUntil; then txnId"""
    c1, c2 = UM.Unmanaged(UM.COMMIT, SP, D), UM.Unmanaged(UM.COMMIT, ESP, C)
    a1, a2 = UM.Unmanaged(UM.APPLY, SP, A), UM.Unmanaged(UM.APPLY, ts(27, SYNC_POINT, 1, 1), A)
    assert c1.compare_to(a1) == -1 and a1.compare_to(c1) == 1
    assert c2.compare_to(c1) == -1 and a1.compare_to(a2) == -1 and a2.compare_to(a1) == 1 and a1.compare_to(a1) == 0


def test_each_outcome():
    c = cfk(BASE)
    # [A]: A is APPLIED and executes before the waiter: readyToExecute stays -> removeWaitingOn
    n, oc, until, ins = c.register_unmanaged(SP, SP, [A])
    assert (n is c, oc, until, ins) == (True, UM.READY, UM.ZERO, [])
    # [A, B]: B is COMMITTED, not APPLIED: not ready, waitingToApply, executesAt = max(A, B) = B
    n, oc, until, ins = c.register_unmanaged(SP, SP, [A, B])
    assert (oc, until, ins, ids(n)) == (UM.PENDING_APPLY, B, [], ids(c))
    assert [r.row() for r in n.unmanageds] == [(UM.APPLY, B, SP, None, ())]
    # [A, B, C]: C is PREACCEPTED: neither; the record waits for the commit of the last dep
    n, oc, until, ins = c.register_unmanaged(SP, SP, [A, B, C])
    assert (oc, until, ins) == (UM.PENDING_COMMIT, C, [])
    assert [r.row() for r in n.unmanageds] == [(UM.COMMIT, C, SP, SP, (A, B, C))]
    # [A, X]: X (hlc 6) is absent: missing, inserted as TRANSITIVELY_KNOWN between A and B with executeAt = TxnId
    n, oc, until, ins = c.register_unmanaged(SP, SP, [A, X])
    assert (oc, until, ins) == (UM.PENDING_COMMIT, X, [X])
    assert ids(n) == [(A, APPLIED), (X, UM.TK), (B, COMMITTED), (C, PRE)] and n.txns[1].raw_x == X and n.txns[1].missing == []
    # no deps at all: i == size, removeWaitingOn
    assert c.register_unmanaged(SP, SP, [])[1] == UM.READY
    # a key without a CommandsForKey: everything is missing
    n, oc, until, ins = cfk([]).register_unmanaged(SP, SP, [A, B])
    assert (oc, until, ins, ids(n)) == (UM.PENDING_COMMIT, B, [A, B], [(A, UM.TK), (B, UM.TK)])


def test_awaits_only_deps_against_the_execute_at_filter():
    """B is COMMITTED with executeAt 30, past the waiter's 23. A range Read ignores it (:1434: executeAt >= its own) and
    is ready; an ExclusiveSyncPoint awaitsOnlyDeps and waits for its application, until B's executeAt (not its TxnId)"""
    x30 = ts(30, 0, 1)
    c = cfk([(A, APPLIED, None), (B, COMMITTED, x30)])
    assert c.register_unmanaged(RR, RR, [A, B])[1] == UM.READY
    n, oc, until, _ = c.register_unmanaged(ESP, ESP, [A, B])
    assert (oc, until) == (UM.PENDING_APPLY, x30)
    # an EphemeralRead awaitsOnlyDeps too; INVALID_OR_TRUNCATED counts as applied
    er = ts(23, EPHEMERAL_READ, 1, 0)
    assert c.register_unmanaged(er, er, [A, B])[1] == UM.PENDING_APPLY
    assert cfk([(A, UC.INVALID, None)]).register_unmanaged(ESP, ESP, [A])[1] == UM.READY
    # a STABLE dep below the waiter's executeAt holds a Read as well
    assert cfk([(A, STABLE, None)]).register_unmanaged(RR, RR, [A])[1:3] == (UM.PENDING_APPLY, A)


def test_dep_equal_to_the_bound_stays():
    """shardRedundantBefore = B: txnIds.find(B) lands on B itself, A below it is skipped"""
    c = cfk([(B, PRE, None), (C, PRE, None)], bound=UM.order(*B))
    assert c.register_unmanaged(SP, SP, [A])[1] == UM.READY            # nothing at or above the bound
    n, oc, until, ins = c.register_unmanaged(SP, SP, [A, B])
    assert (oc, until, ins) == (UM.PENDING_COMMIT, B, [])              # B stays and is uncommitted; A is not missing
    n, oc, until, ins = c.register_unmanaged(SP, SP, [X, B])
    assert ins == []                                                   # an absent dep below the bound is not inserted


def test_update_pending():
    rec = UM.Unmanaged(UM.COMMIT, SP, ts(40), SP, [A, B, ts(40)])
    # the walk stops at the key's last entry: the dep past it (hlc 40) is ignored (:1352)
    assert cfk([(A, APPLIED, None), (B, APPLIED, None)]).update_pending(rec) is None
    got = cfk([(A, APPLIED, None), (B, STABLE, None)]).update_pending(rec)
    assert got.row() == (UM.APPLY, B, SP, None, ())
    # no COMMITTED check (:1360): an uncommitted dep below the waiter's executeAt counts as not applied
    assert cfk([(A, APPLIED, None), (B, PRE, None)]).update_pending(rec).waiting_until == B
    # a dep that is absent while a later entry exists: illegalState (:1356)
    with pytest.raises(UM.IllegalState):
        cfk([(A, APPLIED, None), (C, APPLIED, None)]).update_pending(rec)
    # deps below the current bound are skipped; none left: released
    assert cfk([(C, PRE, None)], bound=UM.order(*ts(44))).update_pending(rec) is None
    # the executeAt filter: a Read ignores B at 30
    rd = UM.Unmanaged(UM.COMMIT, RR, B, RR, [A, B])
    assert cfk([(A, APPLIED, None), (B, STABLE, ts(30, 0, 1))]).update_pending(rd) is None


def test_notify_thresholds_are_exclusive():
    commit_at_c = UM.Unmanaged(UM.COMMIT, SP, C, SP, [A, B, C])
    commit_at_b = UM.Unmanaged(UM.COMMIT, ts(27, SYNC_POINT, 1, 1), B, ts(27, SYNC_POINT, 1, 1), [A, B])
    # minUncommitted = C: Tc = C. The record waiting until C stays (waiting_until == Tc); the one until B is re-evaluated:
    # A applied, B committed -> APPLY until B. next = B (C > B's executeAt), Ta = B: waiting_until == Ta stays.
    c = cfk(BASE, [commit_at_b, commit_at_c])
    n, ev = c.notify_and_update_pending()
    assert ev == [(UM.EV_TO_APPLY, 1, commit_at_b.txn_id, B)]
    assert [r.row()[:3] for r in n.unmanageds] == [(UM.COMMIT, C, SP), (UM.APPLY, B, commit_at_b.txn_id)]
    assert n.notify_and_update_pending()[1] == []
    # B applies: next = null, minUncommitted = C != null: the APPLY arm does not run, nothing is released
    c2 = UM.Cfk(500, cfk([(A, APPLIED, None), (B, APPLIED, None), (C, PRE, None)]).txns, n.unmanageds)
    n2, ev = c2.notify_and_update_pending()
    assert ev == [] and len(n2.unmanageds) == 2
    # C commits with D live: minUncommitted = null, Tc = MAX: the COMMIT record is re-evaluated -> APPLY until C;
    # next = C, Ta = C: the record until B is released (flag 0), the one until C == Ta stays
    c3 = UM.Cfk(500, cfk([(A, APPLIED, None), (B, APPLIED, None), (C, COMMITTED, None), (D, STABLE, None)]).txns, n2.unmanageds)
    n3, ev = c3.notify_and_update_pending()
    assert sorted(ev) == sorted([(UM.EV_TO_APPLY, 1, SP, C), (UM.EV_RELEASE, 0, commit_at_b.txn_id, B)])
    assert [r.row()[:3] for r in n3.unmanageds] == [(UM.APPLY, C, SP)]
    # everything applied: next = null, minUncommitted = null: Ta = MAX releases the rest
    c4 = UM.Cfk(500, cfk([(A, APPLIED, None), (B, APPLIED, None), (C, APPLIED, None), (D, APPLIED, None)]).txns, n3.unmanageds)
    n4, ev = c4.notify_and_update_pending()
    assert ev == [(UM.EV_RELEASE, 0, SP, C)] and n4.unmanageds == []


def test_commit_record_released_or_moved():
    rec = UM.Unmanaged(UM.COMMIT, SP, B, SP, [A, B])
    # every dep applied at the re-evaluation: released straight from COMMIT; it never had an APPLY waiting_until
    n, ev = cfk([(A, APPLIED, None), (B, APPLIED, None)], [rec]).notify_and_update_pending()
    assert ev == [(UM.EV_RELEASE, 1, SP, UM.ZERO)] and n.unmanageds == []
    # B STABLE: moves to APPLY until B; next = B, Ta = B's executeAt == waiting_until: it stays
    n, ev = cfk([(A, APPLIED, None), (B, STABLE, None)], [rec]).notify_and_update_pending()
    assert ev == [(UM.EV_TO_APPLY, 1, SP, B)] and [r.row()[:3] for r in n.unmanageds] == [(UM.APPLY, B, SP)]
    # an ExclusiveSyncPoint waits until the greatest executeAt among its unapplied deps: B bumped to 10
    rec2 = UM.Unmanaged(UM.COMMIT, ESP, B, ESP, [A, B])
    n, ev = cfk([(A, APPLIED, None), (B, STABLE, ts(10, 0, 1)), (D, STABLE, None)], [rec2]).notify_and_update_pending()
    assert ev == [(UM.EV_TO_APPLY, 1, ESP, ts(10, 0, 1))]
    # a key whose entries all left the state: minUncommitted = next = null, both thresholds are Timestamp.MAX
    apply_rec = UM.Unmanaged(UM.APPLY, RR, D)
    n, ev = cfk([], [rec, apply_rec]).notify_and_update_pending()
    assert sorted(ev) == sorted([(UM.EV_RELEASE, 1, SP, UM.ZERO), (UM.EV_RELEASE, 0, RR, D)]) and n.unmanageds == []


@pytest.mark.parametrize("seed", UC.SEEDS)
def test_family_conditions_and_registration_order(seed):
    """every family shows each outcome, each event kind, a created key and a shared missing dep (asserted by
    run_model); pairwise sequential registration equals registration of the same pairs in reversed order"""
    case = UC.family(seed)
    steps = UC.run_model(case, oracle.cfk_apply)
    assert [s[0] for s in steps] == ["register", "apply_deps", "notify", "apply_deps", "notify", "redundant_before", "notify"]
    assert all(len(s[4]) > 0 for s in steps if s[0] == "notify")
    base = oracle.cfk_apply(CC.empty_snapshot(), case["base"])
    fwd, rev = UM.Store(base), UM.Store(base)
    a, b = fwd.register(case["waiters"]), rev.register(case["waiters"], reverse=True)
    np.testing.assert_array_equal(a["outcome"], b["outcome"])
    assert a["until"] == b["until"] and a["n_inserted"] == b["n_inserted"]
    assert UM.comparable(fwd.records()) == UM.comparable(rev.records())
    sa, sb = fwd.state(), rev.state()
    for f in sa:
        np.testing.assert_array_equal(sa[f], sb[f], err_msg=f)


def test_wide_case_meets_its_shape():
    base, w = UC.wide_case((0, 1, UC.UM_LANE_MAX, UC.UM_LANE_MAX + 1, 63, 64, 65, 1000))
    assert list(np.diff(w["dep_off"])) == [0, 1, UC.UM_LANE_MAX, UC.UM_LANE_MAX + 1, 63, 64, 65, 1000]
    st = UM.Store(oracle.cfk_apply(CC.empty_snapshot(), base))
    r = st.register(w)
    assert list(r["outcome"][:2]) == [UM.READY, UM.READY] and (r["outcome"][2:] == UM.PENDING_COMMIT).all() and r["n_inserted"] > 100
