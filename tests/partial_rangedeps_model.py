"""acc_rcmd_partial_rangedeps restated in plain Python — TEST INFRASTRUCTURE.

PreAccept.calculatePartialDeps returns builder.build().with(redundant) (messages/PreAccept.java:245-265): the stab
result united (RangeDeps.with, primitives/RangeDeps.java:567-581: a linearUnion of ranges, TxnIds and pairs) with
RedundantBefore.collectDeps (local/RedundantBefore.java:181-190, 418-421), one (entry.range,
shardAppliedOrInvalidatedBefore) range dep per RedundantBefore entry with a bound above TxnId.NONE that a participant
touches (ReducingRangeMap.foldl, utils/ReducingRangeMap.java:120-196).

The model is pointwise and shares nothing with csrc/: per query it is a set of (range, compare key) pairs,
  the stab half   test_rcmd_gpu.expect_rangedeps, decoded pair by pair;
  the other half  every interval of the map (cfk_redundant_model.BoundMap.intervals(), as ranges of the store's bound
                  type the way RedundantModel.raw_intervals converts them) with a bound above NONE that some key of the
                  query lies in or some range of it intersects, by plain membership / intersection tests;
re-encoded canonically: the union dictionary, the ids with id_row, and the per-query CSR in the Java layout.
"""
import numpy as np

from cfk_redundant_model import NONE, order
from test_rcmd_gpu import RD_FIELDS

NO_ROW = 0xFFFFFFFF


def model_intervals(model):
    """RedundantModel -> [((a, b), compare key, raw bits)]: raw_intervals() with the raw bits of the first update given
    to the map that holds the interval's bound on its first key (a host-only stand-in for what acc_rcmd_redundant_view reports;
    the GPU tests take the bits from the store's view, device_intervals)."""
    out = []
    for (lo, hi, v), (rng, _) in zip(model.map.intervals(), model.raw_intervals()):
        raw = next(t for a, b, t in model.map.updates if a <= lo <= b and order(t) == v)
        out.append((rng, v, raw))
    return out


def device_intervals(store, model):
    """the model's intervals with the raw bits the store's view holds for each (the structure is asserted equal)"""
    g = store.redundant_map()
    iv = model.raw_intervals()
    assert len(g["st"]) == len(iv)
    out = []
    for i, (rng, v) in enumerate(iv):
        raw = (int(g["msb"][i]), int(g["lsb"][i]), int(g["node"][i]))
        assert order(raw) == v, "the store's map is the model's"
        out.append((rng, v, raw))
    return out


def decode(rd, t):
    """the (range, index into the result's id table) pairs of query t of a RangeDeps in the acc_rangedeps_view layout"""
    a = rd["arena"][int(rd["arena_off"][t]):int(rd["arena_off"][t + 1])]
    r = rd["range_id"][int(rd["rd_off"][t]):int(rd["rd_off"][t + 1])]
    d = rd["dep_txn"][int(rd["u_off"][t]):int(rd["u_off"][t + 1])]
    out, start = set(), len(r)
    for i, rid in enumerate(r):
        end = int(a[i])
        rng = (int(rd["rng_start"][rid]), int(rd["rng_end"][rid]))
        for x in a[start:end]:
            out.add((rng, int(d[int(x)])))
        start = end
    return out


def touches(rng, ei, keys, ranges):
    a, b = rng
    if any((a < k <= b) if ei else (a <= k < b) for k in keys):
        return True
    return any(x < b and a < y for x, y in ranges)      # two ranges of one bound type: touching ends do not intersect


def partial_rangedeps(tab, stab, intervals, q, ei):
    """tab: RangeCmdStore.table(); stab: expect_rangedeps(tab, q, ei); intervals: [((a, b), compare key, raw bits)];
    q: the queries dict. Returns dict(RD_FIELDS..., msb, lsb, node, id_row, intervals = sum of |I(q)|, shared = pairs of
    both sides, per_query = [(stab pairs, redundant pairs)] as sets of (range, compare key))."""
    n, nq = len(tab["msb"]), len(q["msb"])
    row_key = [order((tab["msb"][j], tab["lsb"][j], tab["node"][j])) for j in range(n)]
    live = [(rng, v, raw) for rng, v, raw in intervals if v > order(NONE)]
    # ---- the two union tables
    ranges = sorted(set(zip(tab["dict_start"].tolist(), tab["dict_end"].tolist())) | {rng for rng, _, _ in live})
    bits = {}
    for rng, v, raw in live:
        bits.setdefault(v, raw)                          # the lowest interval holding the bound
    for j, k in enumerate(row_key):
        bits[k] = (int(tab["msb"][j]), int(tab["lsb"][j]), int(tab["node"][j]))   # linearUnion keeps the left instance
    ids = sorted(bits)
    row_of = {k: j for j, k in enumerate(row_key)}
    rid_of = {r: i for i, r in enumerate(ranges)}
    id_of = {k: i for i, k in enumerate(ids)}
    # ---- per query
    out = {f: [] for f in ("arena", "range_id", "dep_txn")}
    offs = {f: [0] for f in ("arena_off", "rd_off", "u_off")}
    total = shared = 0
    per_query = []
    for t in range(nq):
        keys = [int(k) for k in q["key_code"][int(q["key_off"][t]):int(q["key_off"][t + 1])]]
        rr = list(zip(q["rng_start"][int(q["rng_off"][t]):int(q["rng_off"][t + 1])].tolist(),
                      q["rng_end"][int(q["rng_off"][t]):int(q["rng_off"][t + 1])].tolist()))
        left = {(rng, row_key[j]) for rng, j in decode(stab, t)}
        right = {(rng, v) for rng, v, _ in live if touches(rng, ei, keys, rr)}
        total += len(right)
        shared += len(left & right)
        per_query.append((left, right))
        pairs = left | right
        rs = sorted({rng for rng, _ in pairs})
        ts_ = sorted({v for _, v in pairs})
        pos = {v: i for i, v in enumerate(ts_)}
        of_range = {}
        for rng, v in pairs:
            of_range.setdefault(rng, []).append(pos[v])
        ends, lists = [], []
        for rng in rs:
            lists += sorted(of_range[rng])
            ends.append(len(rs) + len(lists))
        out["arena"] += ends + lists
        out["range_id"] += [rid_of[r] for r in rs]
        out["dep_txn"] += [id_of[v] for v in ts_]
        offs["arena_off"].append(len(out["arena"]))
        offs["rd_off"].append(len(out["range_id"]))
        offs["u_off"].append(len(out["dep_txn"]))
    res = dict(rng_start=np.array([a for a, _ in ranges], np.uint64), rng_end=np.array([b for _, b in ranges], np.uint64),
               arena=np.array(out["arena"], np.int32), range_id=np.array(out["range_id"], np.uint32),
               dep_txn=np.array(out["dep_txn"], np.uint32))
    for f, v in offs.items():
        res[f] = np.array(v, np.uint64)
    res.update(msb=np.array([bits[k][0] for k in ids], np.uint64), lsb=np.array([bits[k][1] for k in ids], np.uint64),
               node=np.array([bits[k][2] for k in ids], np.int32),
               id_row=np.array([row_of.get(k, NO_ROW) for k in ids], np.uint32),
               intervals=total, shared=shared, per_query=per_query)
    return res


def assert_partial(g, want, msg=""):
    """every array of a RangeCmdStore.partial_rangedeps result against the model's"""
    for f in RD_FIELDS:
        np.testing.assert_array_equal(getattr(g, f), want[f], err_msg=f"{msg}: {f}")
    for f in ("msb", "lsb", "node"):
        np.testing.assert_array_equal(g.ids[f], want[f], err_msg=f"{msg}: ids {f}")
    np.testing.assert_array_equal(g.id_row, want["id_row"], err_msg=f"{msg}: id_row")


def describe(res, t):
    """{(start, end): [(msb, lsb & IDENT, node) ...]} of query t of a model result: what the docstring tables list"""
    ids = [order(x) for x in zip(res["msb"], res["lsb"], res["node"])]
    out = {}
    for rng, i in sorted(decode(res, t)):
        out.setdefault(rng, []).append(ids[i])
    return out
