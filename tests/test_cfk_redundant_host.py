"""Host side of acc_cfk_redundant_before / acc_cfk_redundant_view (no GPU): the ctypes mirrors against the header's
declarations, the exports and prototypes, acc_opts left as it was, and the Python entry points' signatures."""
import ctypes as C
import inspect
import re
from pathlib import Path

from accord_amd import _lib as L
from accord_amd.deps import CfkStore, ReplicaStore

HEADER = (Path(__file__).resolve().parent.parent / "include" / "accord_amd.h").read_text()


def header_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    names = []
    for decl in re.findall(r"([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        names += [part.split()[-1].strip("*") for part in decl.split(",")]   # `type a, b;` -> a, b
    return names


def test_redundant_in_layout_matches_the_header():
    names = header_fields("acc_cfk_redundant_in")
    assert names == [f[0] for f in L.CfkRedundantIn._fields_]
    # u32 x3, padding to 8 | two pointers | three pointers
    offsets = dict(mem=0, n_ranges=4, end_inclusive=8, rng_start=16, rng_end=24, bound=32)
    assert {n: getattr(L.CfkRedundantIn, n).offset for n in names} == offsets
    assert C.sizeof(L.CfkRedundantIn) == 56
    assert dict(L.CfkRedundantIn._fields_)["bound"] is L.TsCols


def test_redundant_map_layout_matches_the_header():
    names = header_fields("acc_cfk_redundant_map")
    assert names == [f[0] for f in L.CfkRedundantMap._fields_]
    # u64 | u32, padding to 8 | two pointers | three pointers
    offsets = dict(n=0, end_inclusive=8, st=16, en=24, bound=32)
    assert {n: getattr(L.CfkRedundantMap, n).offset for n in names} == offsets
    assert C.sizeof(L.CfkRedundantMap) == 56


def test_exports_and_prototypes():
    assert "acc_cfk_redundant_before" in L.EXPORTS and "acc_cfk_redundant_view" in L.EXPORTS
    assert re.search(r"int\s+acc_cfk_redundant_before\(acc_ctx \*ctx, acc_cfk \*cfk, const acc_cfk_redundant_in \*in\);", HEADER)
    assert re.search(r"int\s+acc_cfk_redundant_view\(acc_ctx \*ctx, acc_cfk \*cfk, acc_cfk_redundant_map \*out\);", HEADER)


def test_opts_keeps_its_size():
    assert C.sizeof(L.Opts) == 24
    assert [f[0] for f in L.Opts._fields_][-1] == "cfq_wave_cap"


def test_python_entry_points():
    p = inspect.signature(CfkStore.redundant_before).parameters
    assert list(p) == ["self", "ranges", "end_inclusive"]
    assert p["ranges"].default is inspect.Parameter.empty and p["end_inclusive"].default == 1
    assert list(inspect.signature(CfkStore.redundant_map).parameters) == ["self"]
    assert list(inspect.signature(ReplicaStore.mark_shard_redundant).parameters) == ["self", "ranges"]
