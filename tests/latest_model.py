"""An independent model of LatestDeps.mergeProposal / mergeCommit — TEST INFRASTRUCTURE ONLY.

Written from primitives/LatestDeps.java, utils/ReducingIntervalMap.java (mergeIntervals :202-273,
AbstractIntervalBuilder :522-577) and primitives/Timestamp.java (compareTo :209-217, equals :244-249), and on purpose
NOT the way oracle/latest.py and csrc/latest.hip state them: no pair of cursors, no builder. It imports nothing from
oracle/.

The fold is stated pointwise. A map is a list of disjoint ascending (start, end, Entry). Folding the accumulated map
with the next reply: cut the key line at every bound of both; on each elementary segment the value is nothing where
neither covers it, the one entry where one does, and reduce(accumulated, new) where both do; then one ascending pass
drops the empty segments and joins a segment to the previously kept one iff they touch and carry the same
coordinatedDeps id and the same merge-id list (MergeBuilder.tryMergeEqual, LatestDeps.java:401-419, returns `a`: the
EARLIER entry survives, with its phase and ballot). Two pass-through rules (mergeIntervals :204-207): folding into an
empty accumulator returns the reply as given, its equal neighbours NOT coalesced; a reply without intervals leaves the
accumulator untouched.

An interval of a reply is (start, end, KnownDeps ordinal, ballot (msb, lsb, node), coordinatedDeps id, localDeps id),
ids -1 = null; bounds and msb / lsb are unsigned 64-bit values, node a signed 32-bit one.
"""
from __future__ import annotations

from collections import namedtuple

DEPS_UNKNOWN, DEPS_PROPOSED, DEPS_COMMITTED, DEPS_ERASED, DEPS_KNOWN, NO_DEPS = range(6)   # local/Status.java KnownDeps
TIE_BREAK_WITH_BALLOT = (DEPS_PROPOSED, DEPS_COMMITTED)      # Phase.Accept, Phase.Commit
IDENTITY_LSB = 0xFFFFFFFFFFFF001E
IDENTITY_FLAGS = 0x001E

Entry = namedtuple("Entry", "known ballot coord merge")      # merge: tuple of deps ids (List<Deps> by identity)


class InvalidKnownDeps(Exception):
    """the AssertionError of forProposal / forCommit, or the NullPointerException of a null coordinatedDeps"""


# ---------------------------------------------------------------- Timestamp

def ts_compare(a, b) -> int:
    """Timestamp.compareTo: msb unsigned, then lsb >>> 16, then lsb & IDENTITY_FLAGS, then the node id signed."""
    ka = (a[0], a[1] >> 16, a[1] & IDENTITY_FLAGS, a[2])
    kb = (b[0], b[1] >> 16, b[1] & IDENTITY_FLAGS, b[2])
    return (ka > kb) - (ka < kb)


def ts_equals(a, b) -> bool:
    """Timestamp.equals: msb, the lsb bits of IDENTITY_LSB, and the node."""
    return a[0] == b[0] and ((a[1] ^ b[1]) & IDENTITY_LSB) == 0 and a[2] == b[2]


def ts_key(t):
    """a hashable stand-in for a TxnId under Timestamp.equals"""
    return (int(t[0]), int(t[1]) & IDENTITY_LSB, int(t[2]))


# ---------------------------------------------------------------- the fold

def reduce(a: Entry, b: Entry) -> Entry:
    """AbstractEntry.reduce (:79-96) under MergeEntry.reduce (:266-270), whose lambda ignores its own parameters and
    builds from the outer a and b."""
    winner = a
    if b.known > a.known:
        winner = b
    elif b.known == a.known and a.known in TIE_BREAK_WITH_BALLOT and ts_compare(b.ballot, a.ballot) > 0:
        winner = b
    if winner.known <= DEPS_PROPOSED:
        return Entry(a.known, a.ballot, a.coord, a.merge + b.merge)
    return winner


def as_map(reply):
    """Merge(LatestDeps): the reply's intervals one for one (localDeps -> a merge list of one, or none)"""
    out = []
    for (s, e, known, ballot, coord, local) in reply:
        if not s < e:
            raise ValueError("interval start must be below its end")
        if out and out[-1][1] > s:
            raise ValueError("intervals of one reply must ascend and not overlap")
        out.append((s, e, Entry(known, tuple(ballot), coord, () if local < 0 else (local,))))
    return out


def _covering(m, lo, hi):
    for s, e, v in m:
        if s <= lo and hi <= e:
            return v
    return None


def fold2(acc, new):
    if not acc:
        return new
    if not new:
        return acc
    cuts = sorted({x for s, e, _ in acc + new for x in (s, e)})
    out = []
    for lo, hi in zip(cuts, cuts[1:]):
        a, b = _covering(acc, lo, hi), _covering(new, lo, hi)
        v = b if a is None else a if b is None else reduce(a, b)
        if v is None:
            continue
        if out and out[-1][1] == lo and out[-1][2].coord == v.coord and out[-1][2].merge == v.merge:
            out[-1] = (out[-1][0], hi, out[-1][2])
        else:
            out.append((lo, hi, v))
    return out


def fold(replies):
    """LatestDeps.merge(list, getter) (:232-243): the replies of one recovering txn, left to right"""
    acc = []
    for r in replies:
        acc = fold2(acc, as_map(r))
    return acc


# ---------------------------------------------------------------- selection

def use_local(txn_id, execute_at) -> bool:
    """mergeCommit :322: useLocalDeps = txnId.equals(executeAt)"""
    return ts_equals(txn_id, execute_at)


def ranges_of(rs):
    """Ranges.of (AbstractRanges.java:688-782, UnionMode.MERGE_OVERLAPPING): sorted, ranges that overlap merged, ranges
    that only touch kept apart"""
    out = []
    for s, e in sorted(rs):
        if out and out[-1][1] > s:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def select(m, commit=False, local=False):
    """(items [(deps id, start, end)] in stream order, sufficientFor) of a folded map: forProposal (:337-347) /
    forCommit (:349-378). mergeCommit runs forCommit once for the KeyDeps and once for the RangeDeps with the same
    `success` list, so every range is added twice before Ranges.of."""
    items, success = [], []

    def need(d):
        if d < 0:
            raise InvalidKnownDeps("null coordinatedDeps")
        return d

    for s, e, v in m:
        if not commit:
            if v.known == DEPS_PROPOSED:
                picked = [need(v.coord)]
            elif v.known == DEPS_UNKNOWN:
                picked = list(v.merge)
            else:
                raise InvalidKnownDeps(f"Invalid KnownDeps for proposal: {v.known}")
        else:
            if v.known in (DEPS_KNOWN, DEPS_COMMITTED):
                picked = [need(v.coord)]
            elif v.known == DEPS_PROPOSED:
                if not local:
                    continue
                picked = [need(v.coord)] + list(v.merge)
            elif v.known == DEPS_UNKNOWN:
                if not local:
                    continue
                picked = list(v.merge)
            else:
                raise InvalidKnownDeps(f"Invalid KnownDeps for commit: {v.known}")
            success.append((s, e))
        items.extend((d, s, e) for d in picked)
    return items, ranges_of(success + success)


# ---------------------------------------------------------------- the deps of the selected items, as sets

def relation(objs, d, is_range):
    """[(key, [TxnId key...])] of deps object d of a half in the Deps.merge layout"""
    k0, k1 = int(objs["key_off"][d]), int(objs["key_off"][d + 1])
    v0, o0 = int(objs["val_off"][d]), int(objs["k2v_off"][d])
    nk, out = k1 - k0, []
    for i in range(nk):
        lo = nk if i == 0 else int(objs["k2v"][o0 + i - 1])
        hi = int(objs["k2v"][o0 + i])
        key = (int(objs["key_a"][k0 + i]), int(objs["key_b"][k0 + i])) if is_range else int(objs["key_a"][k0 + i])
        ids = [int(x) for x in objs["k2v"][o0 + lo:o0 + hi]]
        out.append((key, [ts_key((objs["msb"][v0 + x], objs["lsb"][v0 + x], objs["node"][v0 + x])) for x in ids]))
    return out


def _inside(key, s, e, is_range, end_inclusive):
    if is_range:      # Range.compareIntersecting: the same test for (a, b] against (s, e] and for [a, b) against [s, e)
        return key[0] < e and key[1] > s
    return s < key <= e if end_inclusive else s <= key < e


def slice_of(objs, item, is_range, end_inclusive):
    """KeyDeps.slice / RangeDeps.slice of one item: {key or range: set of TxnIds}, keys without TxnIds left out"""
    d, s, e = item
    return {k: set(ids) for k, ids in relation(objs, d, is_range) if ids and _inside(k, s, e, is_range, end_inclusive)}


def slice_counts(objs, item, is_range, end_inclusive):
    """(keys kept, distinct TxnIds kept) of one item, keys without TxnIds included"""
    d, s, e = item
    kept = [(k, ids) for k, ids in relation(objs, d, is_range) if _inside(k, s, e, is_range, end_inclusive)]
    return len(kept), len({t for _, ids in kept for t in ids})


def expected_half(objs, items, is_range, end_inclusive=True):
    """KeyDeps.merge / RangeDeps.merge of the items' slices as {key or range: set of TxnIds}"""
    out = {}
    if objs is None:
        return out
    for it in items:
        for k, ids in slice_of(objs, it, is_range, end_inclusive).items():
            out.setdefault(k, set()).update(ids)
    return out


def latest_deps_merge(groups, key_objs, range_objs, end_inclusive=True, commit=False, txn_ids=None, execute_ats=None):
    """Per group: dict(map=folded map, use_local, items, sufficient, key={key: TxnIds}, range={range: TxnIds})."""
    out = []
    for g, replies in enumerate(groups):
        local = use_local(txn_ids[g], execute_ats[g]) if commit else False
        m = fold(replies)
        items, suff = select(m, commit, local)
        out.append(dict(map=m, use_local=local, items=items, sufficient=suff,
                        key=expected_half(key_objs, items, False, end_inclusive),
                        range=expected_half(range_objs, items, True, end_inclusive)))
    return out


def decode_half(half, g, is_range):
    """group g of a merged half (host copy of the library's view, or the oracle's) as {key or range: set of TxnIds}"""
    if half is None:
        return {}
    k0, k1 = int(half["key_off"][g]), int(half["key_off"][g + 1])
    v0, o0 = int(half["val_off"][g]), int(half["k2v_off"][g])
    nk, out = k1 - k0, {}
    for i in range(nk):
        lo = nk if i == 0 else int(half["k2v"][o0 + i - 1])
        hi = int(half["k2v"][o0 + i])
        key = (int(half["key_a"][k0 + i]), int(half["key_b"][k0 + i])) if is_range else int(half["key_a"][k0 + i])
        ids = {ts_key((half["msb"][v0 + int(x)], half["lsb"][v0 + int(x)], half["node"][v0 + int(x)]))
               for x in half["k2v"][o0 + lo:o0 + hi]}
        if ids:
            assert key not in out, "a key twice in one merged group"
            out[key] = ids
    return out
