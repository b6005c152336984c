"""Host side of acc_cfk_keydeps_mixed (no GPU): the ctypes mirror of acc_cfk_mixed_queries against the header's layout
and the helper that turns acc_preaccept_in-layout queries into the CfkStore.keydeps_mixed dict."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from accord_amd import _lib as L
from accord_amd import workload as W
from accord_amd.deps import mixed_queries_from_preaccept

HEADER = (Path(__file__).resolve().parent.parent / "include" / "accord_amd.h").read_text()


def test_cfk_mixed_queries_layout_matches_the_header():
    body = re.search(r"typedef struct acc_cfk_mixed_queries \{(.*?)\} acc_cfk_mixed_queries;", HEADER, re.S).group(1)
    names = []
    for decl in re.findall(r"([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        names += [part.split()[-1].strip("*") for part in decl.split(",")]   # `type a, *b;` -> a, b
    M = L.CfkMixedQueries
    assert names == [f[0] for f in M._fields_]
    assert M.n_pairs.offset == 8 and M.n_ranges.offset == 16 and M.txn_id.offset == 24 and M.execute_at.offset == 48
    assert M.key_off.offset == 72 and M.rng_off.offset == 88 and M.end_inclusive.offset == 112 and M.lane_seg.offset == 116
    assert C.sizeof(M) == 120
    assert "acc_cfk_keydeps_mixed" in L.EXPORTS
    assert re.search(r"#define\s+ACC_CFQ_LANE_NONE\s+0xFFFFFFFFu", HEADER) and L.ACC_CFQ_LANE_NONE == 0xFFFFFFFF
    # the key-only struct stays as it was
    assert C.sizeof(L.CfkQueries) == 80


def test_mixed_queries_from_preaccept_splits_parts_by_domain():
    ts = lambda h, fl: tuple(int(x) for x in W.encode_ts(1, h, fl, 1))  # noqa: E731
    ids = [ts(5, 2), ts(7, 3), ts(9, 0), ts(11, 9), ts(13, 3)]     # key, range, key (no keys), range, range (no ranges)
    q = dict(msb=np.array([t[0] for t in ids], np.uint64), lsb=np.array([t[1] for t in ids], np.uint64),
             node=np.array([t[2] for t in ids], np.int32), is_range=np.array([0, 1, 0, 1, 1], np.uint8),
             part_off=np.array([0, 2, 4, 4, 5, 5], np.uint32), part_start=np.array([100, 120, 90, 150, 10], np.uint64),
             part_end=np.array([0, 0, 110, 200, 20], np.uint64))
    m = mixed_queries_from_preaccept(q)
    np.testing.assert_array_equal(m["key_off"], [0, 2, 2, 2, 2, 2])
    np.testing.assert_array_equal(m["key_code"], [100, 120])
    np.testing.assert_array_equal(m["rng_off"], [0, 0, 2, 2, 3, 3])
    np.testing.assert_array_equal(m["rng_start"], [90, 150, 10])
    np.testing.assert_array_equal(m["rng_end"], [110, 200, 20])
    assert m["key_off"].dtype == np.uint32 and m["rng_off"].dtype == np.uint32
    for k in ("msb", "lsb", "node"):
        np.testing.assert_array_equal(m[k], q[k])
    assert "xmsb" not in m
    x = dict(q, xmsb=q["msb"], xlsb=q["lsb"] + np.uint64(1 << 16), xnode=q["node"])
    mx = mixed_queries_from_preaccept(x)
    np.testing.assert_array_equal(mx["xlsb"], x["xlsb"])
    # no queries at all
    e = mixed_queries_from_preaccept(dict(msb=np.zeros(0, np.uint64), lsb=np.zeros(0, np.uint64), node=np.zeros(0, np.int32),
                                          is_range=np.zeros(0, np.uint8), part_off=np.zeros(1, np.uint32),
                                          part_start=np.zeros(0, np.uint64), part_end=np.zeros(0, np.uint64)))
    np.testing.assert_array_equal(e["key_off"], [0])
    np.testing.assert_array_equal(e["rng_off"], [0])
