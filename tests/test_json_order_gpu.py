"""GPU: Datum.compareTo (mael/Datum.java:171-185: hash, kind, null last, value) where the hash ties, so that the later
words of the device's three-word encoding (k_json_words in csrc/wire.hip) decide the dictionary's order: LONGs with
equal Long.hashCode, DOUBLEs with equal Double.hashCode, "Aa" / "BB" block STRINGs with equal String.hashCode, and
every kind on one hash. Datum.hash is a CRC32 of the 32-bit hashCode, a bijection on ints, so random values never tie.
STRINGs that tie through the 16 ranked bytes must be rejected (k_json_strcheck), never merged into one key."""
import numpy as np
import pytest

import json_cases as JC
from test_json_gpu import dict_datum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def check_order(ctx, raw):
    """the dictionary is the batch's distinct datums in Datum.compareTo order with the reference's hashes, no two
    distinct datums share a rank, and each document comes back as the Builder result"""
    from accord_amd.deps import deps_from_json, deps_to_json
    seen = {JC.datum_order(d): d for ke, re_ in raw for d, _ in ke}
    seen.update({JC.datum_order(x): x for ke, re_ in raw for (a, b), _ in re_ for x in (a, b)})
    want = sorted(seen)
    r = deps_from_json(ctx, [JC.write_deps(*x) for x in raw], with_view=True)
    got = [JC.datum_order(dict_datum(r, i)) for i in range(len(r["dict_kind"]))]
    assert got == want
    assert len(set(got)) == len(got) == len(want)
    assert [int(h) for h in r["dict_hash"]] == [w[0] for w in want]
    out = deps_to_json(ctx, r["view"])
    for i, (ke, re_) in enumerate(raw):
        assert out[i] == JC.write_deps(*JC.build(ke, re_)), i
    return r


def test_collision_groups_alone(ctx):
    """one document per collision group, its members as keys in reverse order and as the ends of one range: within the
    group nothing but kind, null and the value words can order them"""
    raw = []
    for name, ds in JC.collision_groups().items():
        assert len({JC.datum_hash(*d) for d in ds}) == 1, name
        ds = sorted(ds, key=JC.datum_order)
        ke = [(d, (1, (i + 1) << 16, 1)) for i, d in enumerate(reversed(ds))]
        raw.append((ke, [((ds[0], ds[-1]), (1, 2, 1)), ((ds[1], ds[-1]), (1, 2, 1)), ((ds[0], ds[1]), (1, 2, 1))]))
    check_order(ctx, raw)


def test_collisions_among_random_datums(ctx):
    """the collision groups shuffled into 40 unsorted documents with duplicates, as keys and range ends, among ordinary
    random datums of every kind"""
    raw = JC.collision_docs(np.random.default_rng(0xC0), 40)
    special = {JC.datum_order(d) for ds in JC.collision_groups().values() for d in ds}
    used = {JC.datum_order(d) for ke, re_ in raw for d, _ in ke} | \
           {JC.datum_order(x) for ke, re_ in raw for (a, b), _ in re_ for x in (a, b)}
    assert special <= used and len(used) > len(special) + 100
    check_order(ctx, raw)


def key_doc(datums):
    return JC.write_deps([(d, (1, 2, 1)) for d in datums], [])


@pytest.mark.parametrize("a,b", [(JC.block_string(9), JC.block_string(9, (8,))), ("", "\x00"),
                                 ("Aa" * 8 + "Aa" * 3 + "x", "Aa" * 8 + "BB" * 3 + "x")])
def test_string_tie_beyond_16_bytes_rejected(ctx, a, b):
    """two STRINGs with one hash and the same zero-padded first 16 bytes are one key to the ranked words; the batch
    must fail with IllegalArgumentException -- in one document or across two -- and the context stays usable"""
    from accord_amd.deps import IllegalArgumentException, deps_from_json
    assert a != b and JC.string_hash_code(a) == JC.string_hash_code(b)
    assert a.encode()[:16].ljust(16, b"\0") == b.encode()[:16].ljust(16, b"\0")
    da, db = (JC.STRING, False, a), (JC.STRING, False, b)
    for docs in ([key_doc([da, db])], [key_doc([db]), key_doc([(JC.LONG, False, 1)]), key_doc([da])]):
        with pytest.raises(IllegalArgumentException):
            deps_from_json(ctx, docs)
    check_order(ctx, [([(da, (1, 2, 1))], []), ([((JC.STRING, False, b + "z"), (1, 2, 1))], [])])


def test_string_shared_prefix_different_hash_accepted(ctx):
    """STRINGs that share their first 16 bytes (and more) but not their hash are distinct keys, ordered by hash"""
    pre = "Aa" * 8
    ds = [(JC.STRING, False, pre + t) for t in ("", "x", "y", "xy", "yx", "Aa", "BBx", "Aa" * 4)]
    assert len({JC.datum_hash(*d) for d in ds}) == len(ds)
    r = check_order(ctx, [([(d, (1, 2, 1)) for d in ds], [((ds[1], ds[2]) if JC.datum_order(ds[1]) < JC.datum_order(ds[2])
                                                           else (ds[2], ds[1]), (1, 2, 1))])])
    assert len(r["dict_kind"]) == len(ds)
