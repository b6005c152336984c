"""Host side of the range-command store acc_rcmd_* (no GPU): the ctypes mirrors of acc_rcmd_updates and acc_rcmd_table
against the header's field lists and sizes, the query struct the call shares with acc_cfk_keydeps_mixed, acc_opts left as
it was, and the two Ranges.with orders the store's fold has to keep apart (the host restatement, which the device fold
shares through csrc/ranges_with.hpp)."""
import ctypes as C
import re
from pathlib import Path

from accord_amd import _lib as L
from accord_amd.ranges import Ranges

HEADER = (Path(__file__).resolve().parent.parent / "include" / "accord_amd.h").read_text()


def field_names(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
    names = []
    for decl in re.findall(r"([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        names += [part.split()[-1].strip("*") for part in decl.split(",")]   # `type a, *b;` -> a, b
    return names


def test_rcmd_updates_layout_matches_the_header():
    M = L.RcmdUpdates
    assert field_names("acc_rcmd_updates") == [f[0] for f in M._fields_]
    assert M.n_upd.offset == 0 and M.mem.offset == 4 and M.n_ranges.offset == 8 and M.txn_id.offset == 16
    assert M.flags.offset == 40 and M.rng_off.offset == 48 and M.rng_start.offset == 56 and M.rng_end.offset == 64
    assert C.sizeof(M) == 72


def test_rcmd_table_layout_matches_the_header():
    M = L.RcmdTable
    assert field_names("acc_rcmd_table") == [f[0] for f in M._fields_]
    assert M.n_cmd.offset == 0 and M.end_inclusive.offset == 4 and M.n_ranges.offset == 8 and M.n_dict.offset == 16
    assert M.txn_id.offset == 24 and M.flags.offset == 48 and M.rng_off.offset == 56 and M.rng_start.offset == 64
    assert M.dict_start.offset == 80 and M.dict_end.offset == 88
    assert C.sizeof(M) == 96


def test_rcmd_exports_and_prototypes():
    names = ("acc_rcmd_create", "acc_rcmd_destroy", "acc_rcmd_update", "acc_rcmd_view", "acc_rcmd_rangedeps")
    for n in names:
        assert n in L.EXPORTS
        assert re.search(r"\b%s\(" % n, HEADER)
    # the query call takes the struct of acc_cfk_keydeps_mixed: one query batch serves both halves of PartialDeps
    assert re.search(r"int\s+acc_rcmd_rangedeps\(acc_ctx \*ctx, acc_rcmd \*store, const acc_cfk_mixed_queries \*q,\s*"
                     r"acc_rangedeps_view \*out_view\);", HEADER)
    assert C.sizeof(L.CfkMixedQueries) == 120
    assert re.search(r"#define\s+ACC_RCMD_ERASED\s+1u", HEADER) and L.ACC_RCMD_ERASED == 1


def test_acc_opts_is_untouched():
    assert C.sizeof(L.Opts) == 24
    assert L.Opts._fields_[-1][0] == "cfq_wave_cap"
    assert field_names("acc_opts")[-1] == "cfq_wave_cap"


def test_with_is_order_dependent_as_the_store_replays_it():
    R = lambda *r: Ranges([a for a, _ in r], [b for _, b in r], 0)  # noqa: E731
    pairs = lambda x: list(zip(x.start.tolist(), x.end.tolist()))  # noqa: E731
    assert pairs(R((1, 3)).with_(R((3, 5))).with_(R((2, 4)))) == [(1, 3), (3, 5)]
    assert pairs(R((1, 3)).with_(R((2, 4))).with_(R((3, 5)))) == [(1, 5)]
    # the superset short-cut: the left operand comes back as it is
    assert pairs(R((1, 10), (20, 30)).with_(R((2, 5), (22, 30)))) == [(1, 10), (20, 30)]
