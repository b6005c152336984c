"""The notify model (cfk_notify_model.py) pinned by literals worked from the Java, its closed form checked against it on
random and adversarial states, and the conditions of the case builders (cfk_notify_cases.py) that the GPU tests of
acc_cfk_notify rest on. No GPU."""
import functools

import numpy as np
import pytest

import cfk_cases as CC
import cfk_notify_cases as NC
import cfk_notify_model as NM
import oracle

TK, HIST, PRE, ACC, COMMITTED, STABLE, APPLIED, INVALID = range(8)
W_, R_, S_, X_ = 1, 0, 3, 4
ALL = NM.FIELDS + ("ev_expect", "ev_missing", "held") + NM.VIEW_FIELDS
STATE_FIELDS = ("key", "ent_off", "emsb", "elsb", "enode", "xmsb", "xlsb", "xnode", "status", "miss_off", "mmsb", "mlsb", "mnode")


def same(state, keys=None):
    m, c = NM.model(state, keys), NM.closed_form(state, keys)
    for f in ALL:
        np.testing.assert_array_equal(c[f], m[f], err_msg=f)
    return m


# ---------------------------------------------------------------- literals

def test_literal_abcd():
    state = CC.empty_snapshot()
    for upd, want_state, rows in NC.literal_abcd():
        state = oracle.cfk_apply(state, upd)
        for f in STATE_FIELDS:     # the update (CommandsForKey.update) leaves exactly the state the literal speaks of
            np.testing.assert_array_equal(state[f], want_state[f], err_msg=f)
        m = same(state)
        assert NC.rows_as_hlc(state, m) == rows
    # D is held in the first state: expect 2 (B and C) against missingCount 1
    first = NM.Cfk(NM.key_infos(NC.literal_abcd()[0][1], 0))
    events, held = first.notify(NM.ANY_GLOBALLY_VISIBLE, 0, len(first.committed))
    assert [(t.entry, k, ex, mc) for t, k, _, ex, mc in events] == [(1, NM.RELEASE, 0, 0)] and [t.entry for t in held] == [3]
    second = NM.model(NC.literal_abcd()[1][1])
    assert (int(second["ev_expect"][0]), int(second["ev_missing"][0])) == (1, 1)
    np.testing.assert_array_equal(second["rel_keys"], [0, 0, 0, 1])


def test_literal_kinds():
    for upd, want_state, rows in NC.literal_kinds():
        state = oracle.cfk_apply(CC.empty_snapshot(), upd)
        for f in STATE_FIELDS:
            np.testing.assert_array_equal(state[f], want_state[f], err_msg=f)
        assert NC.rows_as_hlc(state, same(state)) == rows


def test_reference_windows_are_prefixes():
    """a scan from `next` gives the full scan's events (APPLIED entries pass the counters), and a window ending at an
    executeAt gives a prefix of them in committed[] order"""
    for seed in range(20):
        state = random_state(seed, n_keys=1)
        cfk = NM.Cfk(NM.key_infos(state, 0))
        full, _ = cfk.notify(NM.ANY_GLOBALLY_VISIBLE, 0, len(cfk.committed))
        first_live = next((i for i, t in enumerate(cfk.committed) if t.status != APPLIED), len(cfk.committed))
        for end in range(first_live, len(cfk.committed) + 1):
            part, _ = cfk.notify(NM.ANY_GLOBALLY_VISIBLE, first_live, end)
            assert part == full[:len(part)] and all(p < end for _, _, p, _, _ in part)
            assert len(part) == sum(p < end for _, _, p, _, _ in full)


def test_illegal_kinds():
    for kind in (NM.EPHEMERAL_READ, NM.LOCAL_ONLY):
        state = NC.state_of({500: [(4, kind, STABLE, None, [])]})
        with pytest.raises(NM.IllegalState):
            NM.model(state)
        with pytest.raises(NM.IllegalState):
            NM.closed_form(state)


# ---------------------------------------------------------------- the closed form against the model

def random_state(seed, n_keys=4):
    """states no update stream need reach: any status anywhere, executeAts at, between and on other TxnIds, tied, and
    below minUncommitted; missing[] any sorted subset of the lower ids"""
    rng = np.random.default_rng(1000 + seed)
    keys = {}
    for k in range(n_keys):
        n = int(rng.integers(0, 40))
        p_applied = rng.choice([0.0, 0.3, 0.7])
        rows = []
        for i in range(n):
            kind = int(rng.choice([R_, W_, S_, X_], p=[0.35, 0.45, 0.1, 0.1]))
            r = rng.random()
            st = APPLIED if r < p_applied else int(rng.choice([TK, HIST, PRE, ACC, COMMITTED, STABLE, INVALID],
                                                              p=[0.06, 0.03, 0.08, 0.08, 0.2, 0.5, 0.05]))
            xh = None
            if st >= ACC and rng.random() < 0.5:
                b = 4 * i + 4 + 4 * int(rng.integers(-3, 9))
                xh = max(2, b + int(rng.choice([0, 2])))           # on another entry's hlc, or between two
            lower = [4 * j + 4 for j in range(i)]
            miss = sorted(int(x) for x in rng.choice(lower, size=int(rng.integers(0, min(len(lower), 6) + 1)), replace=False)) \
                if lower and st >= ACC and st != INVALID else []
            rows.append((4 * i + 4, kind, st, xh, miss))
        keys[100 + 10 * k] = rows
    return NC.state_of(keys)


@pytest.mark.parametrize("block", range(10))
def test_closed_form_random(block):
    for seed in range(25 * block, 25 * block + 25):     # 250 states
        state = random_state(seed)
        same(state)
        same(state, np.array([90, 100, 115, 120, 900], np.uint64))


def test_closed_form_adversarial():
    ties = {500: [(4, W_, STABLE, 20, []), (8, R_, STABLE, 20, []), (12, W_, COMMITTED, 20, []), (16, S_, STABLE, None, [])]}
    on_id = {500: [(4, W_, STABLE, 12, []), (8, W_, PRE, None, []), (12, W_, STABLE, None, [8]), (16, R_, STABLE, 8, [])]}
    below_min = {500: [(4, W_, PRE, None, []), (8, W_, STABLE, 2, []), (12, R_, STABLE, None, [4])]}
    tk_below = {500: [(4, W_, TK, None, []), (8, R_, HIST, None, []), (12, W_, STABLE, None, [4, 8]), (16, W_, STABLE, None, [])]}
    no_unc = {500: [(4, W_, APPLIED, None, []), (8, W_, STABLE, 14, []), (12, R_, STABLE, None, [])]}
    applied = {500: [(4, W_, APPLIED, 10, []), (8, R_, APPLIED, None, []), (12, W_, INVALID, None, [])], 510: []}
    got = [same(NC.state_of(s)) for s in (ties, on_id, below_min, tk_below, no_unc, applied)]
    # a few of them worked by hand
    # ties: committed[] = [S 16, W 4, R 8, W 12] (the tie stays in TxnId order); S and W 4 expect 0, R 8 expects the write
    assert NC.rows_as_hlc(NC.state_of(ties), got[0]) == (None, 16, 4, [(4, NM.RELEASE, 1), (12, NM.WAITING_TO_EXECUTE, 3),
                                                                        (16, NM.RELEASE, 0)])
    # tk_below: W 12 expects the TRANSITIVELY_KNOWN write and the HISTORICAL read below it, both in its missing[]
    assert NC.rows_as_hlc(NC.state_of(tk_below), got[3]) == (4, None, None, [(12, NM.RELEASE, 0)])
    assert len(got[5]["ev_entry"]) == 0 and list(got[5]["next"]) == [NM.NONE, NM.NONE]
    both = dict(ties)
    both.update({510: on_id[500], 520: below_min[500], 530: tk_below[500], 540: no_unc[500], 550: applied[500]})
    same(NC.state_of(both))


# ---------------------------------------------------------------- the case builders

@functools.lru_cache(maxsize=None)
def chain(seed):
    """[(batch, state after it)] of frontier_case(seed)"""
    state, out = CC.empty_snapshot(), []
    for part in NC.batches(NC.frontier_case(seed)):
        state = oracle.cfk_apply(state, part)
        out.append((part, state))
    return out


@pytest.mark.parametrize("seed", NC.SEEDS)
def test_frontier_case_conditions(seed):
    for part, state in chain(seed):
        m = same(state)
        fig = NC.conditions(state, m)
        assert fig["events"] > 0


def test_cfk_case_will_not_do():
    """the existing generator's lifecycles leave most txns COMMITTED: few releases, most STABLE entries held"""
    state = oracle.cfk_apply(CC.empty_snapshot(), CC.cfk_case(1))
    m = same(state)
    assert 4 * int((m["ev_kind"] == NM.RELEASE).sum()) < int((state["status"] == STABLE).sum())


TIER_SHAPES = [(1, 0, 1), (63, 1, 5), (64, NC.NT_LANE_MAX, 20), (65, NC.NT_LANE_MAX + 1, 64), (255, NC.NT_LANE_FORCE_MAX, 65),
               (256, NC.NT_LANE_FORCE_MAX + 1, 0), (257, 100, 1)]


def test_segments_case_shapes():
    state = oracle.cfk_apply(CC.empty_snapshot(), NC.segments_case(3, TIER_SHAPES))
    np.testing.assert_array_equal(np.diff(state["ent_off"].astype(np.int64)), [n for n, _, _ in TIER_SHAPES])
    eo = state["ent_off"].astype(np.int64)
    for k, (_, nb, live) in enumerate(TIER_SHAPES):
        seg = slice(int(eo[k]), int(eo[k + 1]))
        st = state["status"][seg]
        com = (st >= COMMITTED) & (st <= APPLIED)
        bumped = (state["xlsb"][seg] != state["elsb"][seg]) | (state["xnode"][seg] != state["enode"][seg])
        assert int((com & bumped).sum()) == nb and int(((st == COMMITTED) | (st == STABLE)).sum()) == live
    same(state)
