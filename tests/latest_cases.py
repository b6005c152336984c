"""Seeded LatestDeps recovery cases (primitives/LatestDeps.java, coordinate/Recover.java:295-355) — TEST INFRASTRUCTURE.

Deps objects come from rmm_cases (KeyDepsTest / RangeDepsTest shapes over a 0..1000 key space); each recovering txn gets
2-5 replies, each a LatestDeps of 1-4 RoutingKey intervals with gaps, KnownDeps phases, small ballots (ties exercise
the Accept/Commit ballot tie-break), coordinatedDeps / localDeps ids, and neighbours sharing ids (the builder's
tryMergeEqual coalescing).

The families below the first generator are the scenarios of test_latest_scale_gpu.py (GPU parity) and
test_latest_model.py (the same ones on the CPU, model against oracle): objects of exact key counts around one and two
64-lane trips, bounds on the keys themselves, any-u64 values with edge bounds and ballots, commit timestamps that are
and are not Timestamp.equals, groups without replies and replies without intervals."""
from __future__ import annotations

import numpy as np

import rmm_cases as RC


def deps_objects(seed, n_deps):
    _, kh = RC.gen_groups(seed, 1, n_deps, is_range=False, n_keys=25, n_txn=40, p_empty=0.1)
    _, rh = RC.gen_groups(seed + 7, 1, n_deps, is_range=True, n_keys=12, n_txn=40, p_empty=0.1)
    return kh, rh


def groups(seed, n_groups, n_deps, phases, span=1000):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_groups):
        replies = []
        for _ in range(int(rng.integers(1, 6))):
            pts = sorted({int(x) for x in rng.integers(0, span, size=2 * int(rng.integers(1, 5)))})
            if len(pts) < 2:
                pts = [pts[0], pts[0] + 5]
            ivs = []
            # consecutive points make adjacent intervals; skipping one leaves a gap
            i = 0
            prev = None
            while i + 1 < len(pts):
                s, e = pts[i], pts[i + 1]
                known = int(rng.choice(phases))
                ballot = (1 << 15, (int(rng.integers(0, 3)) << 16), int(rng.integers(0, 2)))
                if prev is not None and rng.random() < 0.3 and (known == 0 or prev[4] >= 0):
                    cd, ld = prev[4], prev[5]            # same objects as the neighbour: coalescing candidates
                else:
                    cd = int(rng.integers(0, n_deps)) if (known != 0 or rng.random() < 0.5) else -1
                    ld = int(rng.integers(0, n_deps)) if rng.random() < 0.7 else -1
                iv = (s, e, known, ballot, cd, ld)
                ivs.append(iv)
                prev = iv
                i += 1 if rng.random() < 0.6 else 2
            replies.append(ivs)
        out.append(replies)
    return out


# ---------------------------------------------------------------- families of test_latest_scale_gpu.py / test_latest_model.py

WAVE_COUNTS = (0, 1, 63, 64, 65, 128, 129, 200)     # keys / ranges per object: around one and two 64-lane trips
EDGE_POINTS = (0, 1, (1 << 32) - 1, (1 << 32) + 1, (1 << 63) - 1, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1)
# ballots at the edges of Timestamp.compareTo: msb on both sides of 2^63 (ordered unsigned), node on both sides of 0
# (ordered signed), and raw lsb bits outside IDENTITY_LSB (0xFFFFFFFFFFFF001E), which compare equal
EDGE_BALLOTS = ((1, 5 << 16, 1), ((1 << 63) + 1, 5 << 16, 1), ((1 << 64) - 1, 5 << 16, 1), (1, 5 << 16, -1),
                (1, 5 << 16, -(1 << 31)), (1, (5 << 16) | 0x8001, 1), (1, (5 << 16) | 0x7FE0, 1), (1, (5 << 16) | 0x2, 1),
                (1, (1 << 63) | (5 << 16), 1), (1, 5 << 16, (1 << 31) - 1))


def sized_objects(seed, counts, n_txn, is_range, span=1000, max_w=63, wide=False, p_flip=0.0, dense=100):
    """One deps object per entry of `counts` with exactly that many keys (ranges), keys in [1, span) (wide: any u64),
    each object with n_txn TxnIds of which its first key references `dense` and the others 1-8. An object of no keys
    has no TxnIds either."""
    rng = np.random.default_rng(seed)
    pool = RC.txn_pool(rng, 3 * n_txn, wide=wide, domain=1 if is_range else 0)
    reps = []
    for nk in counts:
        if nk == 0:
            reps.append(([], [], {}))
            continue
        keys = set()
        if wide:     # some keys and range bounds on the edge points themselves
            for _ in range(min(nk, 3)):
                a, b = sorted(int(x) for x in rng.choice(len(EDGE_POINTS), size=2, replace=False))
                keys.add((EDGE_POINTS[a], EDGE_POINTS[b]) if is_range else EDGE_POINTS[a])
        while len(keys) < nk:
            if wide:
                a, b = sorted(int(x) for x in rng.integers(0, (1 << 64) - 1, size=2, dtype=np.uint64, endpoint=True))
                if not is_range:
                    keys.add(a)
                elif a < b:
                    keys.add((a, b))
            else:
                s = int(rng.integers(1, span))
                keys.add((s, s + int(rng.integers(1, max_w + 1))) if is_range else s)
        vals = sorted(rng.choice(len(pool), size=n_txn, replace=False).tolist())
        ent = {i: sorted(rng.choice(n_txn, size=min(n_txn, dense if i == 0 else int(rng.integers(1, 9))),
                                    replace=False).tolist()) for i in range(nk)}
        reps.append((sorted(keys), [RC.flip_bits(rng, pool[v], p_flip) for v in vals], ent))
    return RC.build_half(reps, is_range)


def groups_on(seed, n_groups, n_deps, phases, points, ballots=None, p_full=0.0, p_no_reply=0.0, p_no_interval=0.0):
    """groups() with the interval bounds drawn from the ascending `points` and the ballots from `ballots`; p_full: a
    reply that is one interval from the first point to the last; p_no_reply: a group without replies; p_no_interval:
    a reply without intervals. Every entry above DepsUnknown has a coordinatedDeps, so every group is valid wherever
    its phases are."""
    rng = np.random.default_rng(seed)
    points = sorted(points)
    out = []

    def entry(s, e, prev):
        known = int(rng.choice(phases))
        ballot = tuple(ballots[int(rng.integers(0, len(ballots)))]) if ballots else \
            (1 << 15, (int(rng.integers(0, 3)) << 16), int(rng.integers(0, 2)))
        if prev is not None and rng.random() < 0.3 and (known == 0 or prev[4] >= 0):
            cd, ld = prev[4], prev[5]
        else:
            cd = int(rng.integers(0, n_deps)) if (known != 0 or rng.random() < 0.5) else -1
            ld = int(rng.integers(0, n_deps)) if rng.random() < 0.7 else -1
        return (s, e, known, ballot, cd, ld)

    for _ in range(n_groups):
        replies = []
        if rng.random() < p_no_reply:
            out.append(replies)
            continue
        for _ in range(int(rng.integers(1, 6))):
            u = rng.random()
            if u < p_no_interval:
                replies.append([])
                continue
            if u < p_no_interval + p_full:
                replies.append([entry(points[0], points[-1], None)])
                continue
            idx = sorted({int(x) for x in rng.integers(0, len(points), size=2 * int(rng.integers(1, 5)))})
            if len(idx) < 2:
                idx = [idx[0] - 1, idx[0]] if idx[0] else [0, 1]
            ivs, i, prev = [], 0, None
            while i + 1 < len(idx):
                prev = entry(points[idx[i]], points[idx[i + 1]], prev)
                ivs.append(prev)
                i += 1 if rng.random() < 0.6 else 2
            replies.append(ivs)
        out.append(replies)
    return out


def single_item_group(d, s, e):
    """a group that selects exactly the item (d, s, e) for a proposal and for a commit: one DepsProposed entry would
    need useLocalDeps at commit, so the two modes get one each"""
    return {False: [[(s, e, 1, (1, 0, 0), d, -1)]], True: [[(s, e, 4, (1, 0, 0), d, -1)]]}


def timestamp_variants(g):
    """(txnId, executeAt, txnId.equals(executeAt) by Timestamp.java:244-249) cycling through: the same bits; equal
    except in lsb bits outside IDENTITY_LSB; different only in the hlc, only in the 0x1E flags, only in the node, only
    in the msb"""
    t = ((1 << 63) | (g + 1), ((g + 7) << 16) | 0x4, -3 if g % 4 == 0 else g)
    msb, lsb, node = t
    x, same = [(t, True), ((msb, lsb ^ 0xFFE1, node), True), ((msb, lsb + (1 << 16), node), False),
               ((msb, lsb ^ 0x10, node), False), ((msb, lsb, node + 1), False), ((msb ^ (1 << 63), lsb, node), False)][g % 6]
    return t, x, same


def scenario(groups, kh, rh, commit=False, end_inclusive=True):
    """one call: the groups, the objects' halves, and in commit mode the timestamps of timestamp_variants"""
    tv = [timestamp_variants(g) for g in range(len(groups))] if commit else []
    return dict(groups=groups, kh=kh, rh=rh, commit=commit, end_inclusive=end_inclusive,
                txn_ids=[t for t, _, _ in tv] or None, execute_ats=[x for _, x, _ in tv] or None,
                equal=[q for _, _, q in tv])


PHASES = {False: [0, 1], True: [0, 1, 2, 4]}       # the KnownDeps that forProposal / forCommit accept
WAVE_POINTS = (0, 100, 250, 400, 600, 800, 1100)   # sized_objects' keys lie in [1, 1000), its range ends below 1063


def count_items(replies, commit, g):
    import latest_model as M
    t, x, _ = timestamp_variants(g)
    return len(M.select(M.fold(replies), commit, M.use_local(t, x) if commit else False)[0])


def past_one_wave(n_items, commit):
    """Family 1: objects of WAVE_COUNTS keys (and, in the opposite order, ranges) with 130 TxnIds each; groups that
    select exactly n_items items in all, the first the whole 200-key object (id 7; its ranges: object 0's 200)."""
    kh = sized_objects(11, WAVE_COUNTS, 130, False)
    rh = sized_objects(12, WAVE_COUNTS[::-1], 130, True)
    nd = len(WAVE_COUNTS)
    lo, hi = WAVE_POINTS[0], WAVE_POINTS[-1]
    out = [single_item_group(nd - 1, lo, hi)[commit]]
    total = 1
    if n_items > 1:
        out.append(single_item_group(0, lo, hi)[commit])
        total += 1
    for replies in groups_on(13 + n_items, 3 * n_items, nd, PHASES[commit], WAVE_POINTS, p_full=0.4):
        k = count_items(replies, commit, len(out))
        if total + k <= n_items:
            out.append(replies)
            total += k
    while total < n_items:
        out.append(single_item_group(total % nd, lo, hi)[commit])
        total += 1
    return scenario(out, kh, rh, commit)


def on_bounds(commit, end_inclusive):
    """Family 2: a key space of 70 points, so that keys fall on interval starts and ends and ranges end where an
    interval starts and start where one ends"""
    rng = np.random.default_rng(21)
    counts = [int(x) for x in rng.integers(5, 21, size=20)]
    kh = sized_objects(22, counts, 40, False, span=64, dense=10)
    rh = sized_objects(23, counts[::-1], 40, True, span=64, max_w=8, dense=10)
    return scenario(groups_on(24 + commit, 40, 20, PHASES[commit], range(0, 73)), kh, rh, commit, end_inclusive)


def wide_values(commit):
    """Family 3: any-u64 keys, TxnIds and nodes with raw flag flips, bounds on EDGE_POINTS, ballots of EDGE_BALLOTS"""
    rng = np.random.default_rng(31)
    counts = [int(x) for x in rng.integers(3, 31, size=16)]
    kh = sized_objects(32, counts, 40, False, wide=True, p_flip=0.5, dense=12)
    rh = sized_objects(33, counts[::-1], 40, True, wide=True, p_flip=0.5, dense=12)
    return scenario(groups_on(34 + commit, 40, 16, PHASES[commit], EDGE_POINTS, ballots=EDGE_BALLOTS, p_full=0.2), kh, rh,
                    commit)


def real_timestamps():
    """Family 4: commit mode over the six timestamp_variants, six groups of each"""
    kh, rh = deps_objects(41, 30)
    return scenario(groups(42, 36, 30, [0, 1, 2, 4]), kh, rh, True)


def sparse(commit, n_groups=30):
    """Family 5: groups without replies and replies without intervals among ordinary ones"""
    kh, rh = deps_objects(51, 20)
    gs = groups_on(52 + commit, n_groups, 20, PHASES[commit], range(0, 1001, 40), p_no_reply=0.25, p_no_interval=0.25)
    return scenario(gs, kh, rh, commit)


def five_items(commit=False):
    """five single-item groups over small objects: one more than a block of k_ld_gather holds waves"""
    kh, rh = deps_objects(61, 6)
    return scenario([single_item_group(d, 100 * d, 100 * d + 350)[commit] for d in range(5)], kh, rh, commit)


def canonical_union(objs, items, is_range, end_inclusive=True):
    """{key: set of TxnIds} = union over items of the object's relation restricted to the item's range (KeyDeps.slice:
    keys contained; RangeDeps.slice: ranges intersecting), by compareTo identity."""
    out = {}
    for d, s, e in items:
        k0, k1 = int(objs["key_off"][d]), int(objs["key_off"][d + 1])
        v0 = int(objs["val_off"][d])
        o0 = int(objs["k2v_off"][d])
        nk = k1 - k0
        prev = nk
        for i in range(nk):
            end = int(objs["k2v"][o0 + i])
            if is_range:
                key = (int(objs["key_a"][k0 + i]), int(objs["key_b"][k0 + i]))
                inside = key[0] < e and key[1] > s
            else:
                key = int(objs["key_a"][k0 + i])
                inside = (s < key <= e) if end_inclusive else (s <= key < e)
            if inside:
                ids = {RC.ts_key(objs["msb"][v0 + int(x)], objs["lsb"][v0 + int(x)], objs["node"][v0 + int(x)])
                       for x in objs["k2v"][o0 + prev:o0 + end]}
                if ids:
                    out.setdefault(key, set()).update(ids)
            prev = end
    return out


def result_map(half, g, is_range):
    m = RC.as_groups(half, is_range)[g]
    return {k: set(v) for k, v in m[2].items() if v}
