"""Host side of acc_rcmd_redundant_before / acc_rcmd_redundant_view (no GPU): the exports and prototypes, the input and
map structs left exactly as acc_cfk_redundant_before declared them, acc_opts left as it was, the Python entry points'
signatures, and the header's out-of-scope list."""
import ctypes as C
import inspect
import re
from pathlib import Path

from accord_amd import _lib as L
from accord_amd.deps import RangeCmdStore, ReplicaStore
from test_cfk_redundant_host import header_fields

HEADER = (Path(__file__).resolve().parent.parent / "include" / "accord_amd.h").read_text()


def test_exports_and_prototypes():
    assert "acc_rcmd_redundant_before" in L.EXPORTS and "acc_rcmd_redundant_view" in L.EXPORTS
    assert re.search(r"int\s+acc_rcmd_redundant_before\(acc_ctx \*ctx, acc_rcmd \*store, const acc_cfk_redundant_in \*in\);", HEADER)
    assert re.search(r"int\s+acc_rcmd_redundant_view\(acc_ctx \*ctx, acc_rcmd \*store, acc_cfk_redundant_map \*out\);", HEADER)


def test_the_library_exports_them():
    lib = L.load()
    for name in ("acc_rcmd_redundant_before", "acc_rcmd_redundant_view"):
        assert getattr(lib, name).restype is C.c_int
        assert len(getattr(lib, name).argtypes) == 3


def test_structs_are_reused_unchanged():
    assert header_fields("acc_cfk_redundant_in") == ["mem", "n_ranges", "end_inclusive", "rng_start", "rng_end", "bound"]
    assert {n: getattr(L.CfkRedundantIn, n).offset for n, _ in L.CfkRedundantIn._fields_} == dict(
        mem=0, n_ranges=4, end_inclusive=8, rng_start=16, rng_end=24, bound=32)
    assert C.sizeof(L.CfkRedundantIn) == 56
    assert header_fields("acc_cfk_redundant_map") == ["n", "end_inclusive", "st", "en", "bound"]
    assert {n: getattr(L.CfkRedundantMap, n).offset for n, _ in L.CfkRedundantMap._fields_} == dict(
        n=0, end_inclusive=8, st=16, en=24, bound=32)
    assert C.sizeof(L.CfkRedundantMap) == 56
    assert C.sizeof(L.Opts) == 24 and [f[0] for f in L.Opts._fields_][-1] == "cfq_wave_cap"


def test_python_entry_points():
    p = inspect.signature(RangeCmdStore.redundant_before).parameters
    assert list(p) == ["self", "ranges"] and p["ranges"].default is inspect.Parameter.empty
    assert list(inspect.signature(RangeCmdStore.redundant_map).parameters) == ["self"]
    p = inspect.signature(ReplicaStore.mark_shard_durable).parameters
    assert list(p) == ["self", "ranges"] and p["ranges"].default is inspect.Parameter.empty
    assert list(inspect.signature(ReplicaStore.mark_shard_redundant).parameters) == ["self", "ranges"]


def test_header_states_the_scope():
    doc = re.search(r"/\* RedundantBefore on the resident range-command store.*?\*/", HEADER, re.S).group(0)
    for word in ("collectDeps", "locally-redundant", "historicalRangeCommands", "maxRedundant", "tombstones", "NotDefined"):
        assert word in doc, word
    cfk_doc = re.search(r"/\* RedundantBefore on the resident store:.*?\*/", HEADER, re.S).group(0)
    assert "acc_rcmd_redundant_before" in cfk_doc and "ACC_RCMD_ERASED" not in cfk_doc
