"""RedundantBefore on the range-command store, restated in plain Python — TEST INFRASTRUCTURE.

An independent model of acc_rcmd_redundant_before: CommandStore.markShardDurable (local/CommandStore.java:520-528) ->
InMemoryCommandStore.markShardDurable (impl/InMemoryCommandStore.java:346-370), one call per distinct bound of the
input, and the registration of InMemorySafeStore.update under a non-empty map (:757-760, through
RedundantBefore.removeShardRedundant, local/RedundantBefore.java:214-223, 431-435), on top of the model of the store
with state (rcmd_state_model.StateModel).

The cut shares nothing with csrc/ranges.hpp or the kernels: per stored range it walks the sorted boundaries of the
applicable input ranges that fall inside it and joins the uncovered elementary segments into maximal pieces
(cut_range). tests/test_rcmd_redundant_model.py pins it against accord_amd.ranges.Ranges.subtract.

seen collects what a stream exercised (TAGS), beside the tags of test_rcmd_gpu.Model."""
import numpy as np

from accord_amd.ranges import Ranges
from cfk_redundant_model import BoundMap, order
from rcmd_state_model import ERASED, StateModel
from test_rcmd_gpu import ident

TAGS = {"cut_head", "cut_tail", "cut_middle_3_pieces", "covered_whole_range", "dropped_first_row", "dropped_last_row",
        "dropped_with_deps", "dropped_already_empty", "equal_bound_stays", "touching_ranges_different_bounds",
        "tombstone_kept", "trim_to_nothing_inserted_empty", "trim_partial", "noop_call", "lower_bound_absorbed",
        "store_emptied"}


def cut_range(a, b, cutters):
    """The maximal sub-intervals of (a, b) that no (s, e) of cutters covers, in order. Both sides are ranges of one bound
    type, so a bound is a bound: (a, b) minus (s, e) leaves (a, s) and (e, b) where they are not empty."""
    inside = [(max(s, a), min(e, b)) for s, e in cutters if s < b and a < e]
    pts = sorted({a, b} | {p for r in inside for p in r})
    out = []
    for lo, hi in zip(pts, pts[1:]):
        if any(s <= lo and hi <= e for s, e in inside):
            continue
        if out and out[-1][1] == lo:
            out[-1] = (out[-1][0], hi)      # the segment continues the piece before it
        else:
            out.append((lo, hi))
    return out


def cut(ranges, cutters):
    """every range of `ranges` cut on its own: nothing is merged across two of them"""
    return [p for a, b in ranges for p in cut_range(a, b, cutters)]


def pairs(r):
    return [] if r is None else [(int(a), int(b)) for a, b in zip(r.start, r.end)]


class RedundantModel(StateModel):
    def __init__(self, end_inclusive):
        super().__init__(end_inclusive)
        self.map = BoundMap(end_inclusive)
        self.rstats = dict(cmds_cut=0, cmds_dropped=0, ranges_before=0, ranges_after=0)
        self.trimmed = 0

    def _ranges(self, prs):
        return Ranges(np.array([a for a, _ in prs], np.uint64), np.array([b for _, b in prs], np.uint64), self.ei)

    def n_ranges(self):
        return sum(len(pairs(c[2])) for c in self.cmd.values())

    # ---- acc_rcmd_redundant_before
    def mark(self, ranges, bounds=None):
        """ranges: the RangeCmdStore.redundant_before dict, or [(start, end)] with bounds = [raw TxnId]"""
        if bounds is not None:
            ranges = dict(rng_start=np.array([a for a, _ in ranges], np.uint64), rng_end=np.array([b for _, b in ranges], np.uint64),
                          msb=np.array([t[0] for t in bounds], np.uint64), lsb=np.array([t[1] for t in bounds], np.uint64),
                          node=np.array([t[2] for t in bounds], np.int32))
        inp = [((int(s), int(e)), order((m, l, n))) for s, e, m, l, n in
               zip(ranges["rng_start"], ranges["rng_end"], ranges["msb"], ranges["lsb"], ranges["node"])]
        before = self.n_ranges()
        self.rstats = dict(cmds_cut=0, cmds_dropped=0, ranges_before=before, ranges_after=before)
        if not inp:
            return
        # the map: pointwise max; a bound at or below what the map holds there is absorbed
        for (s, e), b in inp:
            first_key = s + 1 if self.ei else s
            if b <= order(self.map.get(first_key)) and self.map.updates:
                self.seen.add("lower_bound_absorbed")
        self.map.add(ranges)
        # the prune: by the call's input
        keys = self.keys()
        dropped = []
        for row, k in enumerate(keys):
            raw, erased, rngs = self.cmd[k]
            t = order(raw)
            J = [r for r, b in inp if t < b]
            if erased:
                if J:
                    self.seen.add("tombstone_kept")
                continue
            old = pairs(rngs)
            if any(t == b and any(s < y and x < e for x, y in old) for (s, e), b in inp):
                self.seen.add("equal_bound_stays")
            if not J:
                continue
            for ((s0, e0), b0), ((s1, e1), b1) in zip(inp, inp[1:]):
                if e0 == s1 and (t < b0) != (t < b1) and any(x < e0 < y for x, y in old):
                    self.seen.add("touching_ranges_different_bounds")
            new = []
            for a, b in old:
                p = cut_range(a, b, J)
                new += p
                if not p:
                    self.seen.add("covered_whole_range")
                else:
                    if p[0][0] > a:
                        self.seen.add("cut_head")
                    if p[-1][1] < b:
                        self.seen.add("cut_tail")
                    if len(p) >= 3:
                        self.seen.add("cut_middle_3_pieces")
            if not new:
                dropped.append(k)
                self.rstats["cmds_dropped"] += 1
                if row == 0:
                    self.seen.add("dropped_first_row")
                if row == len(keys) - 1:
                    self.seen.add("dropped_last_row")
                if self.state[k]["deps"]:
                    self.seen.add("dropped_with_deps")
                if not old:
                    self.seen.add("dropped_already_empty")
            elif new != old:
                self.rstats["cmds_cut"] += 1
                self.cmd[k][2] = self._ranges(new)
        for k in dropped:
            del self.cmd[k]
            del self.state[k]
        if not self.rstats["cmds_cut"] and not self.rstats["cmds_dropped"]:
            self.seen.add("noop_call")
        if keys and not self.cmd:
            self.seen.add("store_emptied")
        self.rstats["ranges_after"] = self.n_ranges()

    # ---- registration under the map
    def raw_intervals(self):
        """the map's intervals as ranges of the store's bound type, with their compare keys"""
        return [((lo - 1, hi) if self.ei else (lo, hi + 1), v) for lo, hi, v in self.map.intervals()]

    def trim(self, upd):
        """upd with the ranges of every non-erasing update of a range-domain TxnId t cut by the map's intervals whose
        bound is above t; returns (updates, input ranges changed or removed)"""
        iv = self.raw_intervals()
        n = len(upd["msb"])
        flags = upd["flags"] if upd.get("flags") is not None else np.zeros(n, np.uint8)
        off, rs, re_ = [0], [], []
        changed = 0
        for u in range(n):
            t = (int(upd["msb"][u]), int(upd["lsb"][u]), int(upd["node"][u]))
            a, b = int(upd["rng_off"][u]), int(upd["rng_off"][u + 1])
            old = [(int(x), int(y)) for x, y in zip(upd["rng_start"][a:b], upd["rng_end"][a:b])]
            new = old
            if t[1] & 1 and not int(flags[u]) & ERASED:
                above = [r for r, v in iv if v > order(t)]
                new = []
                for x, y in old:
                    p = cut_range(x, y, above)
                    changed += p != [(x, y)]
                    new += p
                if new and new != old:
                    self.seen.add("trim_partial")
            rs += [x for x, _ in new]
            re_ += [y for _, y in new]
            off.append(len(rs))
        out = dict(upd, rng_off=np.array(off, np.uint32), rng_start=np.array(rs, np.uint64), rng_end=np.array(re_, np.uint64))
        return out, changed

    def apply(self, upd):
        had = set(self.cmd)
        offered = {}
        flags = upd["flags"] if upd.get("flags") is not None else np.zeros(len(upd["msb"]), np.uint8)
        for u in range(len(upd["msb"])):
            if int(upd["lsb"][u]) & 1 and not int(flags[u]) & ERASED:
                k = ident((int(upd["msb"][u]), int(upd["lsb"][u]), int(upd["node"][u])))
                offered[k] = offered.get(k, 0) + int(upd["rng_off"][u + 1]) - int(upd["rng_off"][u])
        trimmed, self.trimmed = self.trim(upd)
        super().apply(trimmed)
        for k, cnt in offered.items():
            if k not in had and cnt and k in self.cmd and not self.cmd[k][1] and not pairs(self.cmd[k][2]):
                self.seen.add("trim_to_nothing_inserted_empty")


def assert_map(store, model, msg=""):
    g = store.redundant_map()
    want = model.map.intervals()
    assert g["end_inclusive"] == model.ei, msg
    np.testing.assert_array_equal(g["st"], np.array([a for a, _, _ in want], np.uint64), err_msg=f"{msg}: map st")
    np.testing.assert_array_equal(g["en"], np.array([b for _, b, _ in want], np.uint64), err_msg=f"{msg}: map en")
    assert [order(t) for t in zip(g["msb"], g["lsb"], g["node"])] == [v for _, _, v in want], f"{msg}: map bounds"
