"""CPU: the independent pointwise model of the LatestDeps merge (tests/latest_model.py) against the restatement
(oracle/latest.py), which is the bit-for-bit checker of acc_latest_deps_merge and shares its structure with the host
fold in csrc/latest.hip.

  * exhaustive: every ordered pair of replies of at most two intervals over a 4-point grid, entries from ALPHABET,
    and every pair followed by a seeded third reply (a coalesced run keeps its first entry; which one that was only
    shows when a later reply is reduced against it);
  * the seeded groups of every family the GPU parity tests run (latest_cases.py), down to the merged deps;
  * hand-worked literals: the expected maps were written out from the Java text, not taken from either
    implementation, and both implementations must give them.
"""
import itertools

import numpy as np
import pytest

import latest
import latest_cases as LC
import latest_model as M

U, P, C, E, K, N = range(6)
B0, B1 = (1, 5 << 16, 1), (1, 6 << 16, 1)


def oracle_map(replies):
    starts, values = latest.fold_group(replies)
    return [(starts[i], starts[i + 1], v.known, tuple(v.ballot), v.coord, tuple(v.merge))
            for i, v in enumerate(values) if v is not None]


def model_map(replies):
    return [(s, e, v.known, v.ballot, v.coord, v.merge) for s, e, v in M.fold(replies)]


def oracle_select(replies, commit, local):
    try:
        return latest.items_of(latest.fold_group(replies), commit, local)
    except latest.InvalidKnownDeps:
        return "invalid"


def model_select(replies, commit, local):
    try:
        return M.select(M.fold(replies), commit, local)
    except M.InvalidKnownDeps:
        return "invalid"


def assert_same(replies):
    assert model_map(replies) == oracle_map(replies), replies
    for commit, local in ((False, False), (True, False), (True, True)):
        assert model_select(replies, commit, local) == oracle_select(replies, commit, local), (replies, commit, local)


# ---------------------------------------------------------------- exhaustive

# phases 0, 1, 2 and 4, each with both ballots; coordinatedDeps null, 1, 2; localDeps null, 3, 4. Entries 2/3, 4/5 and
# 6/7 tie in phase with different ballots; 4 and 6 (and 1 and 5 and 7) carry the same ids in different phases, so a run
# of them coalesces and hides a phase
ALPHABET = ((U, B0, -1, 3), (U, B1, 2, -1), (P, B0, 1, 3), (P, B1, 2, 4), (C, B0, 1, -1), (C, B1, 2, -1), (K, B0, 1, -1),
            (K, B1, 2, -1))
GRID = (0, 1, 2, 3)


def all_replies():
    spans = [(s, e) for s in GRID for e in GRID if s < e]
    out = [[]]
    out += [[(s, e) + x] for s, e in spans for x in ALPHABET]
    out += [[a + x, b + y] for a in spans for b in spans if a[1] <= b[0] for x in ALPHABET for y in ALPHABET]
    return out


def test_alphabet_and_universe():
    assert {x[0] for x in ALPHABET} == {0, 1, 2, 4} and {x[1] for x in ALPHABET} == {B0, B1}
    assert {x[2] for x in ALPHABET} == {-1, 1, 2} and {x[3] for x in ALPHABET} == {-1, 3, 4}
    assert len(all_replies()) == 1 + 6 * 8 + 5 * 64


def test_every_pair_of_small_replies_and_a_third():
    reps = all_replies()
    rng = np.random.default_rng(7)
    third = rng.integers(0, len(reps), size=len(reps) * len(reps))
    coalesced = reduced = 0
    for n, (a, b) in enumerate(itertools.product(reps, reps)):
        m2 = M.fold2(M.as_map(a), M.as_map(b))
        mm = [(s, e, v.known, v.ballot, v.coord, v.merge) for s, e, v in m2]
        assert mm == oracle_map([a, b]), (a, b)
        coalesced += len(a) + len(b) > len(m2) > 0
        reduced += any(len(v.merge) > 1 for _, _, v in m2)
        if n % 4 == 0:      # one pair in four goes on to a third reply, and to the selection: about 34,000 triples
            assert_same([a, b, reps[third[n]]])
    assert coalesced > 1000 and reduced > 1000


# ---------------------------------------------------------------- the families of the GPU parity tests

def _scenarios():
    out = {"five": LC.five_items, "timestamps": LC.real_timestamps}
    for commit in (False, True):
        for n in (1, 4, 5, 300):
            out[f"wave-{n}-{commit}"] = lambda n=n, commit=commit: LC.past_one_wave(n, commit)
        for ei in (True, False):
            out[f"bounds-{commit}-{ei}"] = lambda commit=commit, ei=ei: LC.on_bounds(commit, ei)
        out[f"wide-{commit}"] = lambda commit=commit: LC.wide_values(commit)
        out[f"sparse-{commit}"] = lambda commit=commit: LC.sparse(commit)
    return out


SCENARIOS = _scenarios()     # name -> builder of every parity case of test_latest_scale_gpu.py


def check_model_vs_oracle(sc):
    """the folded maps, the items, sufficientFor and the merged deps of one scenario: model == oracle"""
    for replies in sc["groups"]:
        assert model_map(replies) == oracle_map(replies)
    m = M.latest_deps_merge(sc["groups"], sc["kh"], sc["rh"], sc["end_inclusive"], sc["commit"], sc["txn_ids"], sc["execute_ats"])
    assert [x["use_local"] for x in m] == (sc["equal"] if sc["commit"] else [False] * len(m))
    o = latest.latest_deps_merge(sc["groups"], sc["kh"], sc["rh"], sc["end_inclusive"], sc["commit"],
                                 [x["use_local"] for x in m])
    assert [x["items"] for x in m] == o["items"] and [x["sufficient"] for x in m] == o["sufficient"]
    for g, x in enumerate(m):
        assert M.decode_half(o["key"], g, False) == x["key"], g
        assert M.decode_half(o["range"], g, True) == x["range"], g
    return m, o


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_family_model_vs_oracle(name):
    check_model_vs_oracle(SCENARIOS[name]())


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("phases", [[0, 1], [0, 1, 2, 4], [0, 1, 2, 3, 4, 5]])
def test_dense_seeded_groups(seed, phases):
    """a narrow key line (span 30), so that most intervals overlap and touch; phases 3 and 5 make selections raise"""
    for replies in LC.groups(100 + seed, 60, 6, phases, span=30):
        assert_same(replies)


def test_timestamp_order_and_identity():
    """Timestamp.java:209-217 (compareTo) and :244-249 (equals)"""
    assert M.ts_compare(((1 << 63) + 1, 0, 0), (1, 0, 0)) > 0             # Long.compareUnsigned(msb)
    assert M.ts_compare((1, 0, -1), (1, 0, 1)) < 0                        # Integer.compare(node)
    assert M.ts_compare((1, (5 << 16) | 0x8001, 1), (1, 5 << 16, 1)) == 0  # flags outside IDENTITY_FLAGS
    assert M.ts_compare((1, (5 << 16) | 0x2, 1), (1, 5 << 16, 1)) > 0
    assert M.ts_compare((1, 1 << 63, 1), (1, 5 << 16, 1)) > 0             # lsb >>> 16 is never negative
    for g in range(12):
        t, x, same = LC.timestamp_variants(g)
        assert M.use_local(t, x) is same and (M.ts_compare(t, x) == 0) is same


# ---------------------------------------------------------------- hand-worked literals

def both(replies):
    m = model_map(replies)
    assert m == oracle_map(replies)
    return m


def both_select(replies, commit, local=False):
    r = model_select(replies, commit, local)
    assert r == oracle_select(replies, commit, local)
    return r


def test_literal_arguments_as_passed():
    """MergeEntry.reduce, LatestDeps.java:266-270: the lambda reads the outer a and b, not the (v1, v2) that
    AbstractEntry.reduce :83-92 swapped: a Proposed reply over an Unknown accumulator gives Unknown, the accumulator's
    ballot and coordinatedDeps, and both merge lists, accumulator first"""
    r = [[(0, 10, U, B0, 3, 1)], [(0, 10, P, B1, 5, 2)]]
    assert both(r) == [(0, 10, U, B0, 3, (1, 2))]
    assert both_select(r, False) == ([(1, 0, 10), (2, 0, 10)], [])
    assert both(r[::-1]) == [(0, 10, P, B1, 5, (2, 1))]
    assert both_select(r[::-1], False) == ([(5, 0, 10)], [])


def test_literal_known_against_known():
    """AbstractEntry.reduce :81-82: Phase.Execute does not tieBreakWithBallot (Status.java:105), so c == 0, nothing is
    swapped and the accumulated entry is returned whatever the ballots"""
    for lo, hi in ((B0, B1), (B1, B0)):
        assert both([[(0, 10, K, lo, 1, -1)], [(0, 10, K, hi, 2, -1)]]) == [(0, 10, K, lo, 1, ())]


TIE_BREAKS = [   # (lower, higher) by Timestamp.compareTo :209-217
    ((1, 5 << 16, 1), ((1 << 63) + 1, 5 << 16, 1)),       # msb only, >= 2^63: Long.compareUnsigned
    (((1 << 63) - 1, 5 << 16, 1), (1 << 63, 5 << 16, 1)),
    ((1, 5 << 16, -1), (1, 5 << 16, 1)),                  # node sign only: Integer.compare
    ((1, 5 << 16, -(1 << 31)), (1, 5 << 16, -1)),
]
TIES = [((1, 5 << 16, 1), (1, (5 << 16) | 0x8001, 1)), ((1, (5 << 16) | 0x7FE0, 1), (1, 5 << 16, 1))]   # not in IDENTITY_LSB


@pytest.mark.parametrize("lo,hi", TIE_BREAKS)
def test_literal_ballot_tie_break(lo, hi):
    """AbstractEntry.reduce :82-88: in Phase.Accept and Phase.Commit the higher ballot wins. Committed: the winner is
    returned (:95). Proposed: the winner only decides that merge.apply runs (:91-92), and MergeEntry's lambda builds
    from the arguments as passed either way."""
    for a, b in ((lo, hi), (hi, lo)):
        win = 2 if b == hi else 1
        assert both([[(0, 10, C, a, 1, -1)], [(0, 10, C, b, 2, -1)]]) == [(0, 10, C, hi, win, ())]
        assert both([[(0, 10, P, a, 1, 3)], [(0, 10, P, b, 2, 4)]]) == [(0, 10, P, a, 1, (3, 4))]


@pytest.mark.parametrize("x,y", TIES)
def test_literal_ballot_tie(x, y):
    """ballots that differ only outside IDENTITY_LSB compare 0 (Timestamp.java:213-214): no swap, `a` wins"""
    for a, b in ((x, y), (y, x)):
        assert both([[(0, 10, C, a, 1, -1)], [(0, 10, C, b, 2, -1)]]) == [(0, 10, C, a, 1, ())]


def test_literal_coalescing_keeps_the_first_phase():
    """AbstractIntervalBuilder.append, ReducingIntervalMap.java:554-557 with tryMergeEqual, LatestDeps.java:401-419,
    returning `a`: the tail entry stays. (10, 20] is Committed under B1 in the second reply but is held by the Known
    entry after coalescing, so a Committed reply under a higher ballot does not displace it."""
    B2 = (1, 7 << 16, 1)
    r = [[(0, 10, K, B0, 9, -1)], [(10, 20, C, B1, 9, -1)]]
    assert both(r) == [(0, 20, K, B0, 9, ())]
    assert both(r + [[(10, 20, C, B2, 7, -1)]]) == [(0, 20, K, B0, 9, ())]
    # the same three replies with the Committed one first: it is the run's first entry, and B2 beats B1 on (10, 20]
    r = [[(0, 10, C, B1, 9, -1)], [(10, 20, K, B0, 9, -1)]]
    assert both(r) == [(0, 20, C, B1, 9, ())]
    assert both(r + [[(10, 20, C, B2, 7, -1)]]) == [(0, 10, C, B1, 9, ()), (10, 20, C, B2, 7, ())]


def test_literal_gap_blocks_coalescing():
    """append :540-547: a null entry goes in where prevEnd < start, and :554 does not merge across it"""
    assert both([[(0, 10, K, B0, 9, -1)], [(11, 20, C, B1, 9, -1)]]) == [(0, 10, K, B0, 9, ()), (11, 20, C, B1, 9, ())]


def test_literal_pass_through():
    """mergeIntervals :204-207: an empty left returns the right map itself and an empty right the left; only a fold of
    two non-empty maps rebuilds (and coalesces) them"""
    first = [(0, 10, U, B0, -1, 1), (10, 20, U, B1, -1, 1)]
    two = [(0, 10, U, B0, -1, (1,)), (10, 20, U, B1, -1, (1,))]
    assert both([first]) == two
    assert both([[], first, []]) == two
    assert both_select([first], False) == ([(1, 0, 10), (1, 10, 20)], [])
    assert both([first, [(30, 40, U, B0, -1, 2)]]) == [(0, 20, U, B0, -1, (1,)), (30, 40, U, B0, -1, (2,))]
    assert both([[(30, 40, U, B0, -1, 2)], first]) == [(0, 20, U, B0, -1, (1,)), (30, 40, U, B0, -1, (2,))]


def test_literal_erased_under_known():
    """forCommit :374-375 throws for the entries that are left after the fold, not for the replies': an Erased
    interval that a Known one covers is gone (reduce :81-95, Known > Erased), one that is partly covered is not"""
    r = [[(0, 10, E, B0, 1, -1)], [(0, 10, K, B0, 2, -1)]]
    assert both(r) == [(0, 10, K, B0, 2, ())]
    assert both_select(r, True) == ([(2, 0, 10)], [(0, 10)])
    r = [[(0, 10, E, B0, 1, -1)], [(0, 5, K, B0, 2, -1)]]
    assert both(r) == [(0, 5, K, B0, 2, ()), (5, 10, E, B0, 1, ())]
    assert both_select(r, True) == "invalid"
    for known in (C, E, K, N):      # forProposal :344-345
        assert both_select([[(0, 10, known, B0, 1, 2)]], False) == "invalid"
    assert both_select([[(0, 10, P, B0, -1, 2)]], False) == "invalid"     # :342 getter.apply(null, slice)
    assert both_select([[(0, 10, P, B0, -1, 2)]], True, False) == ([], [])   # :367-368 returns before it


def test_literal_commit_sufficient_for():
    """mergeCommit :321-325: forCommit runs for the KeyDeps and again for the RangeDeps, adding every range twice;
    Ranges.of (AbstractRanges.java:688-693, MERGE_OVERLAPPING: :730-734 merges only where prev.end > next.start)
    drops the copies and keeps ranges that touch apart"""
    r = [[(0, 10, K, B0, 1, -1), (10, 20, U, B0, -1, 2), (30, 40, C, B0, 3, -1)]]
    assert both_select(r, True, False) == ([(1, 0, 10), (3, 30, 40)], [(0, 10), (30, 40)])
    assert both_select(r, True, True) == ([(1, 0, 10), (2, 10, 20), (3, 30, 40)], [(0, 10), (10, 20), (30, 40)])
    assert M.ranges_of([(0, 10), (0, 10), (10, 20), (10, 20), (15, 30)]) == [(0, 10), (10, 30)]
