"""GPU parity for acc_latest_deps_merge where test_latest_gpu.py does not reach: objects and slices past one 64-lane
trip of k_ld_gather / k_ld_half and item counts past one block of k_ld_sizes; both end_inclusive senses with keys and
ranges on the interval bounds; any-u64 keys, bounds and ballots at the edges of the unsigned / signed orders;
txnId.equals(executeAt) from real timestamps; null halves, groups without replies, replies without intervals, no
groups; the objects in device memory; one Context across calls and across a refused call; every refusal.

Every parity case is checked twice: bit for bit against oracle/latest.py (test_latest_gpu.check), and as decoded maps
plus sufficientFor against the independent model (latest_model.py), which is also what gives the oracle its use_local
flags. The cases are the scenarios of latest_cases.py; test_latest_model.py runs the same ones on the CPU. Each family
asserts its own precondition from its inputs or from the model, never from what the library returned."""
import ctypes as C

import numpy as np
import pytest

import latest
import latest_cases as LC
import latest_model as M
from test_latest_gpu import FIELDS, check

pytestmark = pytest.mark.gpu

WAVES, BLOCK = 4, 256       # csrc/ctx.hpp: k_ld_gather / k_ld_half take WAVES items per block, k_ld_sizes BLOCK


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def run(c, sc, kh="kh", rh="rh", **kw):
    from accord_amd.deps import latest_deps_merge
    return latest_deps_merge(c, sc["groups"], sc[kh] if isinstance(kh, str) else kh, sc[rh] if isinstance(rh, str) else rh,
                             end_inclusive=sc["end_inclusive"], commit=sc["commit"], txn_ids=sc["txn_ids"],
                             execute_ats=sc["execute_ats"], **kw)


def expect(sc, kh="kh", rh="rh"):
    """(model result per group, oracle result): the oracle's use_local flags are the model's Timestamp.equals"""
    k, r = sc[kh] if isinstance(kh, str) else kh, sc[rh] if isinstance(rh, str) else rh
    m = M.latest_deps_merge(sc["groups"], k, r, sc["end_inclusive"], sc["commit"], sc["txn_ids"], sc["execute_ats"])
    o = latest.latest_deps_merge(sc["groups"], k, r, sc["end_inclusive"], sc["commit"], [x["use_local"] for x in m])
    return m, o


def assert_parity(got, m, o):
    check(got, o)
    assert len(m) == len(got["sufficient"])
    for g, x in enumerate(m):
        assert got["sufficient"][g] == x["sufficient"], g
        assert M.decode_half(got["key"], g, False) == x["key"], g
        assert M.decode_half(got["range"], g, True) == x["range"], g


def parity(c, sc, **kw):
    m, o = expect(sc, **kw)
    got = run(c, sc, **kw)
    assert_parity(got, m, o)
    return m, got


def sizes(objs):
    return [int(x) for x in np.diff(objs["key_off"].astype(np.int64))], [int(x) for x in np.diff(objs["val_off"].astype(np.int64))]


# ---------------------------------------------------------------- 1. past one wave

@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("n_items", [1, WAVES, WAVES + 1, 300])
def test_past_one_wave(ctx, n_items, commit):
    sc = LC.past_one_wave(n_items, commit)
    for objs in (sc["kh"], sc["rh"]):
        nk, nv = sizes(objs)
        assert sorted(nk) == sorted(LC.WAVE_COUNTS) and max(nk) >= 129
        assert all(v >= 130 for k, v in zip(nk, nv) if k)
    assert n_items in (1, WAVES, WAVES + 1) or n_items > BLOCK
    m, _ = parity(ctx, sc)
    items = [it for x in m for it in x["items"]]
    assert len(items) == n_items
    kc = [M.slice_counts(sc["kh"], it, False, True) for it in items]
    rc = [M.slice_counts(sc["rh"], it, True, True) for it in items]
    assert max(k for k, _ in kc) == 200 and max(v for _, v in kc) > 64       # a whole object: four trips, a ragged tail
    if n_items > 1:
        assert max(k for k, _ in rc) == 200 and max(v for _, v in rc) > 64
    if n_items == 300:
        for cnt in (kc, rc):     # narrow intervals too: slices that keep part of an object, and none of it
            assert any(0 < k < 64 for k, _ in cnt) and any(64 < k < 200 for k, _ in cnt) and any(k == 0 for k, _ in cnt)
        assert sum(1 for x in m if len(x["items"]) > 1) > 10


# ---------------------------------------------------------------- 2. both end_inclusive senses

@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("end_inclusive", [True, False])
def test_keys_and_ranges_on_the_bounds(ctx, commit, end_inclusive):
    sc = LC.on_bounds(commit, end_inclusive)
    m, _ = parity(ctx, sc)
    items = [it for x in m for it in x["items"]]
    on = dict(key_start=0, key_end=0, range_end_at_start=0, range_start_at_end=0)
    for d, s, e in items:
        for k, ids in M.relation(sc["kh"], d, False):
            on["key_start"] += bool(ids) and k == s
            on["key_end"] += bool(ids) and k == e
        for (a, b), ids in M.relation(sc["rh"], d, True):
            on["range_end_at_start"] += bool(ids) and b == s
            on["range_start_at_end"] += bool(ids) and a == e
    assert all(v >= 5 for v in on.values()), on
    # the two senses keep different keys from these very inputs
    other = M.latest_deps_merge(sc["groups"], sc["kh"], sc["rh"], not end_inclusive, commit, sc["txn_ids"], sc["execute_ats"])
    assert [x["key"] for x in other] != [x["key"] for x in m] and [x["range"] for x in other] == [x["range"] for x in m]


# ---------------------------------------------------------------- 3. wide values

@pytest.mark.parametrize("commit", [False, True])
def test_wide_values(ctx, commit):
    sc = LC.wide_values(commit)
    ivs = [iv for g in sc["groups"] for r in g for iv in r]
    assert {x for iv in ivs for x in iv[:2]} == set(LC.EDGE_POINTS)
    assert {iv[3] for iv in ivs} == set(LC.EDGE_BALLOTS)
    for objs in (sc["kh"], sc["rh"]):
        assert int(objs["msb"].max()) >= 1 << 63 and int(objs["node"].min()) < 0 < int(objs["node"].max())
        assert np.any(objs["lsb"] & np.uint64(0xFFE1))                        # raw bits outside IDENTITY_LSB
        assert set(LC.EDGE_POINTS) & {int(x) for x in objs["key_a"]}
    m, _ = parity(ctx, sc)
    assert sum(len(x["key"]) for x in m) > 100 and sum(len(x["range"]) for x in m) > 100


# ---------------------------------------------------------------- 4. use_local from real timestamps

def test_use_local_from_real_timestamps(ctx):
    sc = LC.real_timestamps()
    assert sc["equal"][:6] == [True, True, False, False, False, False] and len(sc["groups"]) == 36
    m, _ = parity(ctx, sc)
    assert [x["use_local"] for x in m] == sc["equal"]
    for v in range(6):      # in every variant the flag decides what some group selects
        assert any(M.select(m[g]["map"], True, True) != M.select(m[g]["map"], True, False) for g in range(v, 36, 6)), v


# ---------------------------------------------------------------- 5. missing and empty parts

@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("halves", ["both", "key-null", "range-null"])
def test_missing_and_empty_parts(ctx, commit, halves):
    sc = LC.sparse(commit)
    gs = sc["groups"]
    assert any(not gs[g] and gs[g - 1] and gs[g + 1] for g in range(1, len(gs) - 1))
    assert any(r == [] for g in gs for r in g) and any(any(r == [] for r in g) and any(g) for g in gs)
    kh, rh = (None if halves == "key-null" else sc["kh"]), (None if halves == "range-null" else sc["rh"])
    m, got = parity(ctx, sc, kh=kh, rh=rh)
    assert sum(len(x["items"]) for x in m) > 50
    if kh is None:
        assert not got["key"]["key_off"].any() and any(x["range"] for x in m)
    if rh is None:
        assert not got["range"]["key_off"].any() and any(x["key"] for x in m)


@pytest.mark.parametrize("commit", [False, True])
def test_no_groups(ctx, commit):
    sc = LC.sparse(commit, n_groups=0)
    assert sc["groups"] == []
    _, got = parity(ctx, sc)
    assert got["sufficient"] == [] and [int(x) for x in got["key"]["key_off"]] == [0]


# ---------------------------------------------------------------- 6. the objects in device memory

@pytest.mark.parametrize("name", ["wave", "wide", "key-null"])
def test_objects_in_device_memory(ctx, name):
    import torch
    sc = {"wave": lambda: LC.past_one_wave(300, True), "wide": lambda: LC.wide_values(False),
          "key-null": lambda: LC.sparse(True)}[name]()
    if name == "key-null":
        sc["kh"] = None
    dev = torch.device("cuda", ctx.device)
    up = {h: None if sc[h] is None else {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sc[h].items()}
          for h in ("kh", "rh")}
    torch.cuda.synchronize()
    host = run(ctx, sc)
    got = run(ctx, sc, kh=up["kh"], rh=up["rh"], deps_on_device=True)
    for half in ("key", "range"):
        assert sorted(got[half]) == sorted(host[half])
        for f in host[half]:
            np.testing.assert_array_equal(got[half][f], host[half][f], err_msg=f"{half} {f}")
    assert got["sufficient"] == host["sufficient"]
    assert_parity(got, *expect(sc))
    for h in ("kh", "rh"):      # the call left the caller's arrays as they were
        for k, t in (up[h] or {}).items():
            np.testing.assert_array_equal(t.cpu().numpy(), sc[h][k], err_msg=f"{h} {k}")


# ---------------------------------------------------------------- 7. one Context reused

def test_one_context_reused():
    from accord_amd.deps import Context, IllegalStateException

    def same(a, b):
        for half, rng in (("key", False), ("range", True)):
            for f in FIELDS + (("key_b",) if rng else ()):
                np.testing.assert_array_equal(a[half][f], b[half][f], err_msg=f"{half} {f}")
        assert a["sufficient"] == b["sufficient"]

    big, five = LC.past_one_wave(300, False), LC.five_items()
    bad = dict(five, groups=five["groups"] + [[[(0, 10, M.DEPS_KNOWN, (1, 0, 0), 1, -1)]]])
    assert sum(LC.count_items(r, False, g) for g, r in enumerate(five["groups"])) == WAVES + 1
    with pytest.raises(M.InvalidKnownDeps):
        M.latest_deps_merge(bad["groups"], bad["kh"], bad["rh"])
    with Context(0) as one:
        got = [run(one, big), run(one, five)]
        with pytest.raises(IllegalStateException):
            run(one, bad)
        got.append(run(one, five))
    for sc, g in zip((big, five, five), got):
        with Context(0) as fresh:
            same(g, run(fresh, sc))
        assert_parity(g, *expect(sc))


# ---------------------------------------------------------------- 8. errors

B = (1, 5 << 16, 1)
U, P, CM, E, K, N = range(6)
ND = 8          # deps objects of the error cases: ids 0..7

ARG_CASES = {   # refused as IllegalArgumentException, whatever the mode
    "start == end": [[[(10, 10, U, B, -1, 1)]]],
    "start > end": [[[(10, 5, U, B, -1, 1)]]],
    "start == end at the top": [[[((1 << 64) - 1, (1 << 64) - 1, U, B, -1, 1)]]],
    "unsorted": [[[(20, 30, U, B, -1, 1), (0, 10, U, B, -1, 2)]]],
    "overlapping": [[[(0, 10, U, B, -1, 1), (5, 20, U, B, -1, 2)]]],
    "overlapping in a later group": [[[(0, 10, P, B, 1, -1)]], [[(0, 10, P, B, 2, -1)], [(0, 10, U, B, -1, 1), (9, 20, U, B, -1, 2)]]],
    "ordinal 6": [[[(0, 10, 6, B, 1, 1)]]],
    "ordinal 255": [[[(0, 10, 255, B, 1, 1)]]],
    "coordinatedDeps == n_deps": [[[(0, 10, P, B, ND, -1)]]],
    "localDeps == n_deps": [[[(0, 10, U, B, -1, ND)]]],
    "coordinatedDeps -2": [[[(0, 10, P, B, -2, 1)]]],
    "localDeps -2": [[[(0, 10, U, B, -1, -2)]]],
    "localDeps most negative": [[[(0, 10, U, B, -1, -(1 << 31))]]],
}
STATE_CASES = {   # (commit, txnId equals executeAt, groups): refused as IllegalStateException
    "proposal, null coordinatedDeps": (False, False, [[[(0, 10, P, B, -1, 1)]]]),
    "proposal, null coordinatedDeps after a reduce": (False, False, [[[(0, 10, P, B, -1, 1)], [(0, 10, U, B, 2, 3)]]]),
    "commit Known, null coordinatedDeps": (True, False, [[[(0, 10, K, B, -1, -1)]]]),
    "commit Committed, null coordinatedDeps": (True, False, [[[(0, 10, CM, B, -1, -1)]]]),
    "commit Proposed with local deps, null coordinatedDeps": (True, True, [[[(0, 10, P, B, -1, 1)]]]),
    "proposal Committed": (False, False, [[[(0, 10, CM, B, 1, -1)]]]),
    "proposal Erased": (False, False, [[[(0, 10, E, B, 1, -1)]]]),
    "proposal Known": (False, False, [[[(0, 10, K, B, 1, -1)]]]),
    "proposal NoDeps": (False, False, [[[(0, 10, N, B, 1, -1)]]]),
    "proposal Known over Unknown": (False, False, [[[(0, 10, U, B, -1, 1)], [(5, 10, K, B, 1, -1)]]]),
    "commit Erased": (True, True, [[[(0, 10, E, B, 1, -1)]]]),
    "commit NoDeps": (True, False, [[[(0, 10, N, B, 1, -1)]]]),
    "commit NoDeps over Known": (True, False, [[[(0, 10, K, B, 1, -1)], [(0, 10, N, B, 2, -1)]]]),
    "commit Erased partly under Known": (True, False, [[[(0, 10, E, B, 1, -1)], [(0, 5, K, B, 2, -1)]]]),
    "commit Erased in the second group": (True, False, [[[(0, 10, K, B, 1, -1)]], [[(0, 10, E, B, 1, -1)]]]),
}


@pytest.fixture(scope="module")
def small_objs():
    kh, rh = LC.deps_objects(9, ND)
    assert len(kh["key_off"]) - 1 == ND == len(rh["key_off"]) - 1
    return kh, rh


def call(c, objs, gs, commit=False, equal=False, **kw):
    from accord_amd.deps import latest_deps_merge
    tids = [(1, (g + 1) << 16, 1) for g in range(len(gs))]
    exes = [t if equal else (t[0], t[1] + (1 << 16), t[2]) for t in tids]
    return latest_deps_merge(c, gs, objs[0], objs[1], commit=commit, txn_ids=tids, execute_ats=exes, **kw)


@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("name", sorted(ARG_CASES))
def test_refused_arguments(ctx, small_objs, name, commit):
    from accord_amd.deps import IllegalArgumentException
    with pytest.raises(IllegalArgumentException):
        call(ctx, small_objs, ARG_CASES[name], commit)


@pytest.mark.parametrize("name", sorted(STATE_CASES))
def test_refused_states(ctx, small_objs, name):
    from accord_amd.deps import IllegalStateException
    commit, equal, gs = STATE_CASES[name]
    with pytest.raises(M.InvalidKnownDeps):      # the model refuses the same groups
        for replies in gs:
            M.select(M.fold(replies), commit, equal)
    with pytest.raises(IllegalStateException):
        call(ctx, small_objs, gs, commit, equal)


def test_refused_mode_end_inclusive_and_memory(ctx, small_objs):
    from accord_amd import _lib as L
    from accord_amd.deps import IllegalArgumentException
    gs = [[[(0, 10, P, B, 1, 2)]]]
    call(ctx, small_objs, gs)
    with pytest.raises(IllegalArgumentException):
        call(ctx, small_objs, gs, end_inclusive=2)
    for field, bad in (("mode", 2), ("mode", 0xFFFFFFFF), ("end_inclusive", 2), ("deps_mem", 2)):
        li, v = L.LatestIn(), L.LatestView()      # no groups, no objects: nothing else to refuse
        assert ctx._lib.acc_latest_deps_merge(ctx.handle, C.byref(li), C.byref(v)) == L.ACC_OK
        setattr(li, field, bad)
        with pytest.raises(IllegalArgumentException):
            ctx.check(ctx._lib.acc_latest_deps_merge(ctx.handle, C.byref(li), C.byref(v)))
    kh, rh = small_objs
    with pytest.raises(IllegalArgumentException):      # a range half without its range ends
        call(ctx, (kh, {k: v for k, v in rh.items() if k != "key_b"}), gs)


def test_erased_wholly_under_known_is_no_error(ctx, small_objs):
    """forCommit sees the folded entries, not the replies': Erased wholly under Known is gone, whichever came first and
    however the Erased reply was cut (NoDeps ranks above Known and is never covered: STATE_CASES has it)"""
    for gs in ([[[(0, 10, E, B, 1, -1)], [(0, 10, K, B, 2, -1)]]],
               [[[(0, 10, K, B, 2, -1)], [(3, 7, E, B, 1, -1)]]],
               [[[(0, 5, E, B, 1, -1), (5, 10, E, B, 3, -1)], [(0, 10, K, B, 2, -1)]]]):
        got = call(ctx, small_objs, gs, commit=True)
        m = M.latest_deps_merge(gs, *small_objs, True, True, [(1, 1 << 16, 1)], [(1, 2 << 16, 1)])
        o = latest.latest_deps_merge(gs, *small_objs, commit=True, use_local=[False])
        assert m[0]["items"] == [(2, 0, 10)] and m[0]["sufficient"] == [(0, 10)]
        assert_parity(got, m, o)
