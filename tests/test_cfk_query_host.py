"""Host side of acc_cfk_keydeps (no GPU): the ctypes mirror of acc_cfk_queries and of the acc_opts knob against the
header's layout, and the executeAt ReplicaStore.preaccept_batch(scan="new") gives a query that carries none."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np

import cfk_cases as CC
from accord_amd import _lib as L
from accord_amd import workload as W
from accord_amd.deps import Context, _execute_at_after

HEADER = (Path(__file__).resolve().parent.parent / "include" / "accord_amd.h").read_text()


def test_opts_keeps_its_size_and_names_the_knob():
    assert C.sizeof(L.Opts) == 24
    assert [f[0] for f in L.Opts._fields_][-1] == "cfq_wave_cap"
    body = re.search(r"typedef struct acc_opts \{(.*?)\} acc_opts;", HEADER, re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == [f[0] for f in L.Opts._fields_]
    # the slice limit of the wave-per-item launches took the reserved second word: flags stays first, the rest in place
    assert [f[0] for f in L.Opts._fields_][:3] == ["flags", "wave_grid_max", "cfk_hot"]
    assert L.Opts.wave_grid_max.offset == 4 and L.Opts.cfq_wave_cap.offset == 20
    for knob in ("wave_grid_max", "cfq_wave_cap"):
        p = inspect.signature(Context.__init__).parameters[knob]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0


def test_cfk_queries_layout_matches_the_header():
    body = re.search(r"typedef struct acc_cfk_queries \{(.*?)\} acc_cfk_queries;", HEADER, re.S).group(1)
    names = []
    for decl in re.findall(r"([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        names += [part.split()[-1].strip("*") for part in decl.split(",")]   # `type a, b;` -> a, b
    assert names == [f[0] for f in L.CfkQueries._fields_]
    assert L.CfkQueries.n_pairs.offset == 8 and L.CfkQueries.txn_id.offset == 16
    assert L.CfkQueries.execute_at.offset == 40 and L.CfkQueries.key_off.offset == 64
    assert C.sizeof(L.CfkQueries) == 80
    assert "acc_cfk_keydeps" in L.EXPORTS


def test_execute_at_after_follows_the_store_rule():
    """TxnInfo.create (CommandsForKey.java:669-670): the executeAt of the txn's last update in the batch when that status
    carries one, else the TxnId; a TxnId the batch does not hold keeps its own."""
    ts = lambda h, fl=2, nd=1: tuple(int(x) for x in W.encode_ts(1, h, fl, nd))  # noqa: E731
    a, b, c, d = ts(4), ts(8), ts(12), ts(16)
    bump = ts(30, 0, 3)
    rows = [(a, a, CC.ACC), (b, b, CC.PRE), (a, bump, CC.COMMITTED), (c, c, CC.ACC), (c, bump, CC.INVALID), (b, b, 0xFF)]
    part = dict(msb=np.array([r[0][0] for r in rows], np.uint64), lsb=np.array([r[0][1] for r in rows], np.uint64),
                node=np.array([r[0][2] for r in rows], np.int32), xmsb=np.array([r[1][0] for r in rows], np.uint64),
                xlsb=np.array([r[1][1] for r in rows], np.uint64), xnode=np.array([r[1][2] for r in rows], np.int32),
                status=np.array([r[2] for r in rows], np.uint8))
    q = dict(msb=np.array([t[0] for t in (a, b, c, d)], np.uint64), lsb=np.array([t[1] for t in (a, b, c, d)], np.uint64),
             node=np.array([t[2] for t in (a, b, c, d)], np.int32))
    xm, xl, xn = _execute_at_after(part, q)
    got = list(zip((int(x) for x in xm), (int(x) for x in xl), (int(x) for x in xn)))
    assert got == [bump, b, c, d]
    assert q["lsb"][0] == a[1], "the queries' own columns are left as they were"
