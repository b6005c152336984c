"""CPU: the test-side JSON writer reproduces the reference's byte forms (Datum.write, Json.writeTimestamp, toString(Id))
and Datum.hash; no GPU."""
import json

import json_cases as JC


def test_writer_forms():
    doc = JC.write_deps([((JC.LONG, False, -7), (32768, 327682, 1)), ((JC.HASH, False, -3), (1, 2, 0)),
                         ((JC.HASH, True, 0), (1, 2, -4)), ((JC.LONG, True, 0), ((1 << 64) - 1, 2, 3))],
                        [(((JC.LONG, False, 1), (JC.LONG, False, 9)), (1, 2, 5))])
    assert doc == (b'{"keyDeps":[[-7,[32768,327682,"n1"]],[["HASH",true,-3],[1,2,null]],[["HASH",false],[1,2,"c-4"]],'
                   b'[["LONG"],[-1,2,"n3"]]],"rangeDeps":[[1,9,[1,2,"n5"]]]}')
    json.loads(doc)


def test_datum_hash_and_order():
    # hash(null) = Integer.MAX_VALUE sorts null datums last; a Hash datum's hash is itself
    assert JC.datum_hash(JC.LONG, True, 0) == 0x7FFFFFFF
    assert JC.datum_hash(JC.HASH, False, -5) == -5
    assert JC.datum_order((JC.HASH, False, 0x7FFFFFFF)) < JC.datum_order((JC.HASH, True, 0))
    vals = [JC.datum_hash(JC.LONG, False, v) for v in range(1000)]
    assert len(set(vals)) == 1000 and sorted(vals) != vals   # hash order, not value order


def test_java_double_to_string():
    # Double.toString (JDK >= 19: shortest digits that round-trip; sci form outside [1e-3, 1e7))
    cases = [(0.0, "0.0"), (-0.0, "-0.0")] + list({1.0: "1.0", 0.1: "0.1", 1e7: "1.0E7", 9999999.0: "9999999.0", 0.001: "0.001",
             0.0009: "9.0E-4", 5e-324: "4.9E-324", 2e23: "2.0E23", 1e22: "1.0E22", 12345678.9: "1.23456789E7",
             1.7976931348623157e308: "1.7976931348623157E308", 2.2250738585072014e-308: "2.2250738585072014E-308",
             0.30000000000000004: "0.30000000000000004", -2.5e-3: "-0.0025", 100.0: "100.0", 123.456: "123.456"}.items())
    for x, want in cases:
        assert JC.java_double_to_string(x) == want, (x, JC.java_double_to_string(x))
    import numpy as np
    rng = np.random.default_rng(5)
    for _ in range(2000):
        x = JC.random_double(rng)
        s = JC.java_double_to_string(x)
        assert float(s) == x            # round trips
        m = s.lstrip("-").split("E")[0].replace(".", "").strip("0")
        assert len(m) <= 17


def test_gson_string():
    # JsonWriter.string with htmlSafe: <, >, &, =, ' as \u00XX; quote, backslash, control chars escaped
    assert JC.gson_string('a<b"\\\n') == '"a\\u003cb\\"\\\\\\n"'
    assert JC.gson_string("x>y&z='w'") == '"x\\u003ey\\u0026z\\u003d\\u0027w\\u0027"'
    assert JC.gson_string("\t\x01/") == '"\\t\\u0001/"'
    import json
    for t in ["", "abc", "a\"b", "q\\\n\r\b\f", "<>&='"]:
        assert json.loads(JC.gson_string(t)) == t


# ---------------------------------------------------------------- the number / order case generators (no GPU)
# These keep tests/test_json_numbers_gpu.py and tests/test_json_order_gpu.py from passing vacuously and pin the model.

def test_parse_number_rule():
    # JsonReader.nextLong, else nextDouble: the forms test_json_number_forms lists
    for lit, want in [("1.0", (JC.LONG, False, 1)), ("1e2", (JC.LONG, False, 100)), ("-0", (JC.LONG, False, 0)),
                      ("-0.0", (JC.LONG, False, 0)), ("9223372036854775807", (JC.LONG, False, (1 << 63) - 1)),
                      ("9223372036854775808", (JC.LONG, False, (1 << 63) - 1)),
                      ("9.223372036854775807E18", (JC.LONG, False, (1 << 63) - 1)),
                      ("-9223372036854775809", (JC.LONG, False, -(1 << 63))), ("9007199254740993", (JC.LONG, False, 9007199254740993)),
                      ("9007199254740993.0", (JC.LONG, False, 9007199254740992)), ("0.1", (JC.DOUBLE, False, 0.1)),
                      ("1e19", (JC.DOUBLE, False, 1e19)), ("4.9E-324", (JC.DOUBLE, False, 5e-324))]:
        assert JC.parse_number(lit) == want, lit
    import pytest
    for lit in JC.INFINITY_LITERALS:
        with pytest.raises(ValueError):
            JC.parse_number(lit)
    assert JC.significant_digits("-0.001230e5") == 3 and JC.significant_digits("100000000000000000000e-20") == 1


def test_two_digit_rule_below_the_decade():
    # Double.toString javadoc (JDK >= 19): with a minimal length of 1, the nearest of ALL decimals of length 1 or 2 that
    # round to x. 20 * 2^-1074 = 9.88..E-323: both 1E-322 and 9.9E-323 round to it and 9.9E-323 is nearer, one decade
    # below the one-digit decimal (Double.MIN_VALUE * 20 prints "9.9E-323", * 2 prints "9.9E-324").
    import math
    for m, want in [(1, "4.9E-324"), (2, "9.9E-324"), (3, "1.5E-323"), (4, "2.0E-323"), (16, "7.9E-323"), (20, "9.9E-323"),
                    (202, "1.0E-321"), (2024, "1.0E-320")]:
        assert JC.java_double_to_string(math.ldexp(float(m), -1074)) == want, m


def test_tostring_cases_against_repr():
    """every Double.toString case: the model's text parses back to the value and is the decimal Python's repr gives (the
    shortest, then closest), except where a one-digit decimal rounds to the value and the two-digit rule applies"""
    import math
    from decimal import Decimal
    xs = JC.tostring_doubles()
    assert len(xs) == len(set(xs)) and 2800 <= len(xs) <= 3600
    differs = []
    for x in xs:
        s = JC.java_double_to_string(x)
        assert float(s) == x and (s[0] == "-") == (x < 0), (x, s)
        if Decimal(s) != Decimal(repr(x)):
            assert JC.has_one_digit_form(x) and JC.text_digits(s) == 2, (x, s)
            if x > 0:
                differs.append(x)
    p2 = set(JC.pow2_doubles())
    # among the powers of two: 4.9E-324, 9.9E-324 (repr: 1e-323, the one-digit decimal a decade above) and 7.9E-323
    assert sorted(x for x in differs if x in p2) == [math.ldexp(1.0, k) for k in (-1074, -1073, -1070)]
    assert sum(1 for x in xs if x < 0) >= len(xs) // 4 - 1


def test_tostring_case_coverage():
    import math
    p2 = JC.pow2_doubles()
    assert len(p2) == 2035
    as_double = [x for x in p2 if JC.parse_number(JC.java_double_to_string(x))[0] == JC.DOUBLE]
    assert len(as_double) >= 1900
    # negative binary exponent and a normal or subnormal 2^k other than 2^-1022 and 2^-1074 (whose intervals are
    # symmetric): the asymmetric-interval branch of shortest_digits
    asym = [x for x in as_double if x < 1 and x not in (math.ldexp(1.0, -1022), math.ldexp(1.0, -1074))
            and math.frexp(x)[1] - 1 >= -1022]
    assert len(asym) >= 1000
    assert 2.0 ** -44 in asym and JC.java_double_to_string(2.0 ** -44) == "5.684341886080802E-14"
    nb = JC.pow2_neighbours()
    assert len(nb) == 200 and all(math.frexp(x)[0] != 0.5 for x in nb)
    sub = [x for x in JC.subnormal_doubles() if x < math.ldexp(1.0, -1022)]
    assert len(sub) == 105 and math.ldexp(1.0, -1022) in JC.subnormal_doubles()
    assert math.ldexp(float((1 << 52) - 1), -1074) in sub
    wins, stays = JC.two_digit_cases()
    assert len(wins) >= 10 and len(stays) >= 10
    assert 5e-324 in wins and math.ldexp(16.0, -1074) in wins and math.ldexp(20.0, -1074) in wins
    assert 0.5 in stays and 2.0e-3 in stays
    for x in wins:
        assert JC.has_one_digit_form(x) and JC.text_digits(JC.java_double_to_string(x)) == 2
    for x in stays:
        assert JC.has_one_digit_form(x) and JC.text_digits(JC.java_double_to_string(x)) == 1
    by_k10, edges = JC.layout_doubles()
    assert sorted(by_k10) == list(range(-4, 9))
    for k, x in by_k10.items():
        s = JC.java_double_to_string(x)
        assert x != math.floor(x) and math.floor(math.log10(x)) == k and ("E" in s) == (not -3 <= k < 7), (k, s)
    assert [JC.java_double_to_string(x) for x in edges[:8]] == [
        "0.001", "9.999999999999998E-4", "9999999.999999998", "1.0000000000000002E7", "1.0E23", "2.0E23",
        "9.223372036854776E18", "1.0E19"]
    # integral doubles above 2^63 stay DOUBLE; 2^63 itself reads as Long.MAX_VALUE
    assert [JC.parse_number(JC.java_double_to_string(x))[0] for x in edges[4:]] == [JC.DOUBLE, JC.DOUBLE, JC.LONG, JC.DOUBLE, JC.DOUBLE]


def test_parse_cases():
    import math
    from fractions import Fraction

    def value(lit):   # the literal's exact value
        m, _, e = lit.lower().partition("e")
        return Fraction(m) * Fraction(10) ** int(e or 0)

    mids = JC.midpoint_cases()
    assert len(mids) == 500 and sum(1 for x, *_ in mids if x < math.ldexp(1.0, -1022)) >= 50
    assert len({math.frexp(x)[1] // 64 for x, *_ in mids}) >= 30   # the whole exponent range
    pairs, around = JC.seam_cases()
    for x, y, m, lo, hi in mids + pairs:
        assert y == math.nextafter(x, math.inf) and m == (Fraction(x) + Fraction(y)) / 2
        assert value(lo) <= m < value(hi) and value(hi) - value(lo) == Fraction(10) ** int(lo.partition("e")[2])
        assert JC.significant_digits(lo) <= 19 and JC.significant_digits(hi) <= 19
        # float() and the exact comparison with the midpoint agree
        assert float(lo) == JC.rounds_between(value(lo), x, y) and float(hi) == JC.rounds_between(value(hi), x, y) == y
        assert float(lo) == x or value(lo) == m
    big_sub, min_norm = math.ldexp(float((1 << 52) - 1), -1074), math.ldexp(1.0, -1022)
    assert (pairs[0][0], pairs[0][1], pairs[1][0]) == (big_sub, min_norm, min_norm)
    assert float(pairs[0][3]) == big_sub and float(pairs[0][4]) == min_norm   # the carry into the smallest normal
    assert value(around[0]) < Fraction(min_norm) < value(around[1]) and float(around[0]) == float(around[1]) == min_norm
    ties = JC.exact_tie_literals()
    assert len(ties) >= 18 and [t for t, _, _ in ties[:6]] == [
        "9007199254740993.0", "9007199254740995.0", "2251799813685248.25", "2251799813685248.75", "4503599627370496.5",
        "4503599627370497.5"]
    for lit, x, y in ties:
        assert value(lit) == (Fraction(x) + Fraction(y)) / 2 and float(lit) == JC.rounds_between(value(lit), x, y)
        assert JC.significant_digits(lit) <= 19
    assert {JC.double_bits(x) & 1 for _, x, _ in ties} == {0, 1}
    assert {JC.parse_number(t)[0] for t, _, _ in ties} == {JC.LONG, JC.DOUBLE}
    z = JC.ZERO_BOUNDARY
    assert value(z[0]) < Fraction(1, 2 ** 1075) < value(z[1])
    assert [JC.parse_number(t) for t in z] == [(JC.LONG, False, 0), (JC.DOUBLE, False, 5e-324)] + [(JC.LONG, False, 0)] * 4
    top = (Fraction(2) ** 1024 + Fraction(1.7976931348623157e308)) / 2
    assert value(JC.MAX_DOUBLE_LITERAL) < top < value(JC.INFINITY_LITERALS[0])
    assert JC.parse_number(JC.MAX_DOUBLE_LITERAL) == (JC.DOUBLE, False, 1.7976931348623157e308)
    lits = JC.parse_literals()
    assert len(lits) >= 1040 and all(JC.significant_digits(t) <= 19 for t in lits)
    assert set(JC.ZERO_BOUNDARY + JC.CLINGER + JC.LITERAL_FORMS + around) <= set(lits)
    assert JC.significant_digits(JC.NUMBER_REJECTS[0]) == 20 and "0" not in JC.NUMBER_REJECTS[0]
    for t in lits:
        JC.parse_number(t)   # none is an infinity


def test_collision_groups():
    import math
    g = JC.collision_groups()
    assert set(g) == {"long_0", "long_c", "double_c", "string_16", "string_18", "cross_0", "cross_max"}
    for name, ds in g.items():
        assert len({JC.datum_hash(*d) for d in ds}) == 1, name
        assert len({JC.datum_order(d) for d in ds}) == len(ds) >= 5, name
    for name in ("long_0", "long_c"):
        vs = [v for _, _, v in g[name]]
        assert len(vs) >= 6 and min(vs) < 0 < max(vs) and all(-(1 << 63) <= v < 1 << 63 for v in vs)
    assert {0, -1, (1 << 32) | 1, -(1 << 63) + (1 << 31)} <= {v for _, _, v in g["long_0"]}
    ds = [v for _, _, v in g["double_c"]]
    assert all(math.isfinite(x) and x != math.floor(x) for x in ds)
    assert sum(1 for x in ds if x > 0) >= 2 and sum(1 for x in ds if x < 0) >= 2
    for name, n in (("string_16", 16), ("string_18", 18)):
        ss = sorted(s for _, _, s in g[name])
        assert all(len(s) == n for s in ss)
        firsts = {next(i for i in range(n) if a[i] != b[i]) for a in ss for b in ss if a != b}
        assert firsts == {0, 6, 8, 14}   # the first and the second ranked word both decide
    kinds = [(k, nl) for k, nl, _ in g["cross_0"]]
    assert {k for k, _ in kinds} == {JC.STRING, JC.LONG, JC.DOUBLE, JC.HASH} and not any(nl for _, nl in kinds)
    assert all(x != math.floor(x) for k, _, x in g["cross_0"] if k == JC.DOUBLE)
    assert sorted((k, nl) for k, nl, _ in g["cross_max"]) == [(0, True), (1, True), (2, True), (3, False), (3, True)]
    # Datum.compareTo inside one hash: kind, then null last, then the value (signed longs, Double.compare)
    order = sorted(g["cross_max"], key=JC.datum_order)
    assert [(k, nl) for k, nl, _ in order] == [(0, True), (1, True), (2, True), (3, False), (3, True)]
    lo = sorted(g["long_0"], key=JC.datum_order)
    assert [v for _, _, v in lo] == sorted(v for _, _, v in lo)
    do = sorted(g["double_c"], key=JC.datum_order)
    assert [x for _, _, x in do] == sorted(x for _, _, x in do)
