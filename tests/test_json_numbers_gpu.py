"""GPU: the JSON wire's arbitrary-precision number paths (csrc/wire.hip) at their edges. Double.parseDouble
(decimal_to_double: a 1408-bit long division) and Double.toString (shortest_digits / write_double: Burger-Dybvig digit
generation with the JDK 19 two-digit rule) against Python's correctly rounded float(), fractions.Fraction and the
rational-arithmetic model json_cases.java_double_to_string. Every comparison is bit for bit or byte for byte.

For each literal: (1) the datum it parses to -- kind and dict_value (the long, or doubleToLongBits of float(literal)) --
is located through the document's key codes; (2) the document acc_deps_to_json writes holds the long, or
Double.toString of the double. (3) The expected values are fixed before the device is called; nothing is filtered by
what it returns."""
import numpy as np
import pytest

import json_cases as JC

pytestmark = pytest.mark.gpu

PER_DOC = 32
TXN = (1, 2, 1)


@pytest.fixture(scope="module")
def ctx():
    from accord_amd.deps import Context
    c = Context(0)
    yield c
    c.close()


def doc_of(lits):
    return ('{"keyDeps":[' + ",".join(f'[{x},[1,2,"n1"]]' for x in lits) + '],"rangeDeps":[]}').encode()


def check_numbers(ctx, lits, seed=1):
    """parse every literal as a key of some document (at most PER_DOC per document, one device thread each), write the
    documents back, and compare datum by datum and byte by byte"""
    from accord_amd.deps import deps_from_json, deps_to_json
    lits = list(lits)
    want = [JC.parse_number(x) for x in lits]   # before the device runs
    order = np.random.default_rng(seed).permutation(len(lits))   # spread cheap and expensive literals over the threads
    groups = [[int(i) for i in order[a:a + PER_DOC]] for a in range(0, len(lits), PER_DOC)]
    docs = [doc_of([lits[i] for i in g]) for g in groups]
    r = deps_from_json(ctx, docs, with_view=True)
    out = deps_to_json(ctx, r["view"])
    assert len(out) == len(docs)
    key_off, key_a = r["key"]["key_off"], r["key"]["key_a"]
    for d, g in enumerate(groups):
        # the Builder result: the document's distinct datums in Datum.compareTo order
        exp = sorted({JC.datum_order(want[i]): want[i] for i in g}.items())
        ranks = [int(x) for x in key_a[int(key_off[d]):int(key_off[d + 1])]]
        assert len(ranks) == len(exp), ([lits[i] for i in g], out[d])
        for rank, (_, dat) in zip(ranks, exp):
            got = (int(r["dict_kind"][rank]), int(r["dict_null"][rank]), int(r["dict_value"][rank]))
            assert got == (dat[0], 0, JC.datum_value_bits(dat)), ([lits[i] for i in g if want[i] == dat], dat, got)
        assert out[d] == JC.write_deps([(dat, TXN) for _, dat in exp], []), [lits[i] for i in g]
    return r


def check_rejected(ctx, lit):
    from accord_amd.deps import IllegalArgumentException, deps_from_json
    with pytest.raises(IllegalArgumentException):
        deps_from_json(ctx, [doc_of([lit])])


def test_double_to_string_edges(ctx):
    """Double.toString of every power of two 2^k, k in [-1074, -1] and [63, 1023] (all but 2^-1074 and 2^-1022 below 1
    take the asymmetric interval: the predecessor is half as far as the successor), of successors and predecessors of
    powers of two, subnormals, the JDK 19 two-digit rule where the second digit wins and where it does not, the layout
    boundaries 10^-3 and 10^7, and negative copies. Each value is fed as its own Double.toString text. An integral
    double below 2^63 is read back as LONG (2^63 itself as Long.MAX_VALUE: Java's (long) d == d), so it cannot be
    written as DOUBLE through the parse; the others come back as the same text."""
    xs = JC.tostring_doubles()
    check_numbers(ctx, [JC.java_double_to_string(x) for x in xs])


def test_parse_double_rounding(ctx):
    """Double.parseDouble where the rounding decides: 19-digit literals just below and just above the midpoint of two
    adjacent doubles (500 random pairs over the whole exponent range, subnormals included), exact ties with an even
    and an odd lower neighbour, the zero boundary 2^-1075, the largest finite literal, the subnormal / normal seam, the
    limits of Clinger's fast path, and the literal forms JsonReader.peekNumber takes."""
    check_numbers(ctx, JC.parse_literals())


@pytest.mark.parametrize("lit", JC.INFINITY_LITERALS + JC.NUMBER_REJECTS)
def test_number_rejected(ctx, lit):
    """a literal that rounds to infinity (JsonReader rejects infinities), has 20 nonzero significant digits (the limit
    of the device path), or is no JSON number fails the batch with IllegalArgumentException; the context then still
    parses a good document"""
    check_rejected(ctx, lit)
    check_numbers(ctx, [JC.MAX_DOUBLE_LITERAL, "0.1", "7"])
