"""The bound families of rd_cases.py do what the GPU tests rely on, checked without a GPU: each family's masks come to
the plan widths its band needs (so test_bound_families of test_rangedeps_gpu.py and test_rcmd_gpu.py reach the band
they name), the commands' widths reach every width class, and the oracle finds deps in every one."""
import numpy as np
import pytest

import rd_cases
from rd_cases import U64, plan_bits


def test_plan_bits_literals():
    """make_runs (csrc/prims.hpp): the set bits; with more than 12 runs the hull highest - lowest + 1."""
    assert plan_bits(0) == 0 and plan_bits(1) == 1 and plan_bits(U64) == 64 and plan_bits(1 << 63) == 1
    assert plan_bits(0b1011) == 3
    twelve = sum(1 << (2 * i) for i in range(12))
    assert plan_bits(twelve) == 12                       # 12 runs: still the set bits
    assert plan_bits(twelve | 1 << 24) == 25             # 13 runs: bits 0..24
    assert plan_bits(rd_cases.SPARSE) == 61 and bin(rd_cases.SPARSE).count("1") == 21
    assert plan_bits(rd_cases.SPARSE << 3) == 61         # the hull does not start at bit 0


@pytest.mark.parametrize("ei", [1, 0])
@pytest.mark.parametrize("name", list(rd_cases.FAMILIES))
def test_family_shapes(name, ei):
    import oracle
    f = rd_cases.family(name, 0x5EED, ei)
    assert 330 <= len(f["cmds"]) <= 420 and len(f["keyq"]) >= 300 and len(f["rngq"]) == 300
    keys = [k for q in f["keyq"] for k in q]
    los = keys + [s for q in f["rngq"] for s, _ in q]
    ref = keys[0]
    mask = 0
    for x in los:
        mask |= x ^ ref
    assert mask == rd_cases.FAMILIES[name][1], "the XOR mask of the query low bounds is the family's varying bits"
    if name in rd_cases.FAMILY_QUERY_BITS:
        assert plan_bits(mask) == rd_cases.FAMILY_QUERY_BITS[name]
    rs = [s for c in f["cmds"] for s, _ in c]
    re = [e for c in f["cmds"] for _, e in c]
    sb, eb = plan_bits(rd_cases.or_mask(rs)), plan_bits(rd_cases.or_mask(re))       # the store's masks: plain OR
    if name in rd_cases.FAMILY_DICT:
        assert (sb + eb, int(sb + eb > 64)) == rd_cases.FAMILY_DICT[name]
        if name == "e64":
            assert (sb, eb) == (0, 64)
    else:
        assert sb + eb > 64
    cls = set(rd_cases.width_classes(rs, re))
    if name in ("top3", "top2", "top1", "full", "sparse"):
        assert cls == set(range(33))
    # a key on a bound that contains it under this bound type
    bound = {(e if ei else s) for c in f["cmds"] for s, e in c}
    assert any(k in bound for k in keys)
    if name == "full":
        assert 0 in keys and U64 in keys
    rb = rd_cases.family_batch(name, 0x5EED, ei)
    want = rd_cases.batch_plan_bits(rb)
    if name in rd_cases.FAMILY_QUERY_BITS:
        assert want["query_bits"] == rd_cases.FAMILY_QUERY_BITS[name]
    if name in rd_cases.FAMILY_DICT:
        assert (want["dict_bits"], want["dict_split"]) == rd_cases.FAMILY_DICT[name]
    o = oracle.rangedeps_batch(rb)
    nd = np.diff(o.u_off.astype(np.int64))
    n_cmd = len(f["cmds"])
    assert (nd[n_cmd:n_cmd + len(f["keyq"])] > 0).sum() >= 100, "the key queries find deps"
    assert (nd[n_cmd + len(f["keyq"]):] > 0).sum() >= 100, "the range queries find deps"
