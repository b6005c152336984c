"""Maelstrom Deps JSON (accord-maelstrom Json.DEPS_ADAPTER, mael/Json.java:316-398) — TEST INFRASTRUCTURE: a Python
writer in Gson's compact form and the Builder semantics (sorted unique keys by Datum.compareTo, sorted unique TxnIds by
Timestamp.compareTo) over every datum kind: LONG, HASH, null sentinels, STRING (ASCII; Gson's HTML-safe escaping) and
DOUBLE (Java's Double.toString, restated with exact rational arithmetic: shortest digits that round back, closest on
ties, the JDK 19 two-digit rule, Java's plain / computerized-scientific layout). A datum is (kind, null, value) with
value an int (LONG, HASH), a str (STRING) or a float (DOUBLE)."""
from __future__ import annotations

import math
import struct
import zlib
from fractions import Fraction
from functools import lru_cache

import numpy as np

STRING, LONG, DOUBLE, HASH = range(4)   # Datum.Kind ordinals


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def double_bits(x: float) -> int:
    return struct.unpack(">Q", struct.pack(">d", x))[0]


def string_hash_code(s: str) -> int:
    """String.hashCode over UTF-16 units (ASCII here: one per character)"""
    h = 0
    for ch in s:
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    return _i32(h)


def datum_hash(kind, null, value):
    """Datum.hash (mael/Datum.java:188-200): null -> Integer.MAX_VALUE; Hash -> its hash; else CRC32 over the 4 low
    bytes of value.hashCode() (Long.hashCode = (int)(v ^ (v >>> 32)); Double.hashCode the same over the bits)."""
    if null:
        return 0x7FFFFFFF
    if kind == HASH:
        return _i32(value)
    if kind == STRING:
        i = string_hash_code(value) & 0xFFFFFFFF
    else:
        v = double_bits(value) if kind == DOUBLE else value & 0xFFFFFFFFFFFFFFFF
        i = (v ^ (v >> 32)) & 0xFFFFFFFF
    return _i32(zlib.crc32(bytes([i & 0xFF, (i >> 8) & 0xFF, (i >> 16) & 0xFF, (i >> 24) & 0xFF])))


def _value_order(kind, value):
    if kind == DOUBLE:   # Double.compareTo: bit order with -0.0 < 0.0
        b = double_bits(value)
        return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else b | (1 << 63)
    return value


def datum_order(d):
    """Datum.compareTo (:172-186): hash, kind, null last, value"""
    kind, null, value = d
    return (datum_hash(kind, null, value), kind, 1 if null else 0, 0 if null else _value_order(kind, value))


def _rounds_to(q: Fraction, x: float) -> bool:
    try:
        return float(q) == x
    except OverflowError:
        return False


def java_double_to_string(x: float) -> str:
    """Double.toString (JDK >= 19): among the decimals that round to x, the shortest; of those the closest (ties: even
    last digit); if the shortest has one digit, the closest of those with one or two digits. Then Java's layout:
    plain with at least one fraction digit for 1e-3 <= |x| < 1e7, else d.dddE[-]n."""
    if x == 0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    neg = x < 0
    v = Fraction(abs(x))
    # shortest digit count n with some n-digit decimal rounding to x
    best = None
    for n in range(1, 18):
        e = math.floor(math.log10(abs(x)))
        for ee in (e - 1, e, e + 1):   # the decimal exponent of the first digit
            scale = Fraction(10) ** (ee - n + 1)
            q = v / scale
            lo, hi = math.floor(q), math.ceil(q)
            cands = []
            for c in {lo, hi}:
                if 10 ** (n - 1) <= c < 10 ** n and _rounds_to(Fraction(c) * scale, abs(x)):
                    cands.append((abs(Fraction(c) * scale - v), c % 2, c, ee))
            if cands:
                cands.sort()
                if best is None or cands[0][:2] < best[0][:2]:
                    best = (cands[0][0], cands[0][1]), cands[0][2], cands[0][3], n
        if best is not None:
            if n == 1:
                # JDK 19 javadoc: when the minimal length is 1, the nearest of ALL decimals s * 10^i of length 1 or 2
                # (1 <= s <= 99) that round to x, ties to the even significand. That includes two-digit decimals one
                # decade below the one-digit one (9.9E-323 against 1.0E-322 for 20 * 2^-1074).
                _, c1, ee1, _ = best
                t = []
                for i in range(ee1 - 2, ee1 + 1):
                    scale = Fraction(10) ** i
                    for c in {math.floor(v / scale), math.ceil(v / scale)}:
                        if 1 <= c <= 99 and _rounds_to(Fraction(c) * scale, abs(x)):
                            t.append((abs(Fraction(c) * scale - v), c % 2, c, i))
                _, _, c, i = min(t)
                while c % 10 == 0:
                    c, i = c // 10, i + 1
                best = (None, c, i + len(str(c)) - 1, len(str(c)))
            break
    _, c, ee, n = best
    digits = str(c).rstrip("0") or "0"
    k = ee   # value = 0.d1d2.. * 10^(k+1) = d1.d2.. * 10^k
    if -3 <= k < 7:
        if k < 0:
            s = "0." + "0" * (-k - 1) + digits
        else:
            ip = digits[:k + 1].ljust(k + 1, "0")
            fp = digits[k + 1:] or "0"
            s = ip + "." + fp
    else:
        s = digits[0] + "." + (digits[1:] or "0") + "E" + str(k)
    return ("-" if neg else "") + s


def gson_string(t: str) -> str:
    """JsonWriter.string with Gson's default HTML-safe replacement table"""
    out = ['"']
    for ch in t:
        o = ord(ch)
        if ch == '"':
            out.append('\\"')
        elif ch == "\\":
            out.append("\\\\")
        elif ch in "\t\b\n\r\f":
            out.append({"\t": "\\t", "\b": "\\b", "\n": "\\n", "\r": "\\r", "\f": "\\f"}[ch])
        elif o < 0x20 or ch in "<>&='":
            out.append("\\u%04x" % o)
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def ts_order(t):
    msb, lsb, node = t
    return (msb & 0xFFFFFFFFFFFFFFFF, (lsb & 0xFFFFFFFFFFFFFFFF) >> 16, lsb & 0x1E, node)


def write_datum(d):
    kind, null, value = d
    if null:
        return '["HASH",false]' if kind == HASH else f'["{("STRING", "LONG", "DOUBLE", "HASH")[kind]}"]'
    if kind == HASH:
        return f'["HASH",true,{_i32(value)}]'
    if kind == STRING:
        return gson_string(value)
    if kind == DOUBLE:
        return java_double_to_string(value)
    return str(value)


def write_txn(t):
    msb, lsb, node = t
    s = lambda x: x - (1 << 64) if x >= 1 << 63 else x  # noqa: E731  (Java longs)
    nd = "null" if node == 0 else f'"{"c" if node < 0 else "n"}{node}"'
    return f"[{s(msb)},{s(lsb)},{nd}]"


def write_deps(key_entries, range_entries):
    """entries in the order given: [(datum, txn)], [((start, end), txn)]"""
    k = ",".join(f"[{write_datum(d)},{write_txn(t)}]" for d, t in key_entries)
    r = ",".join(f"[{write_datum(a)},{write_datum(b)},{write_txn(t)}]" for (a, b), t in range_entries)
    return ('{"keyDeps":[' + k + '],"rangeDeps":[' + r + "]}").encode()


def build(key_entries, range_entries):
    """KeyDeps / RangeDeps Builder result in DEPS_ADAPTER write order: keys ascending, then each key's TxnIds ascending"""
    km, rm = {}, {}
    for d, t in key_entries:
        km.setdefault(datum_order(d), (d, {}))[1].setdefault(ts_order(t), t)
    for (a, b), t in range_entries:
        rm.setdefault((datum_order(a), datum_order(b)), ((a, b), {}))[1].setdefault(ts_order(t), t)
    ke = [(d, ts[o]) for _, (d, ts) in sorted(km.items()) for o in sorted(ts)]
    re_ = [(r, ts[o]) for _, (r, ts) in sorted(rm.items()) for o in sorted(ts)]
    return ke, re_


_ALPHABET = "abcXYZ019 <>&='\"\\/\t\n-_.~"


def random_double(rng):
    """a non-integral double (an integral one is read back as LONG): random bits over the whole range, or short decimals"""
    while True:
        if rng.random() < 0.5:
            x = struct.unpack(">d", struct.pack(">Q", int(rng.integers(0, 1 << 63))))[0]
            if rng.random() < 0.5:
                x = -x
        else:
            x = float(f"{int(rng.integers(-10**6, 10**6))}e{int(rng.integers(-12, 12))}")
        if math.isfinite(x) and x != math.floor(x):
            return x


def random_datum(rng, p_hash=0.25, p_null=0.03, span=None, p_string=0.0, p_double=0.0):
    if rng.random() < p_null:
        return (int(rng.choice([LONG, HASH, STRING, DOUBLE] if p_string or p_double else [LONG, HASH])), True, 0)
    if rng.random() < p_hash:
        return (HASH, False, int(rng.integers(-(1 << 31), 1 << 31)))
    if rng.random() < p_string:
        n = int(rng.integers(0, 24))
        return (STRING, False, "".join(_ALPHABET[int(i)] for i in rng.integers(0, len(_ALPHABET), size=n)))
    if rng.random() < p_double:
        return (DOUBLE, False, random_double(rng))
    v = int(rng.integers(-(1 << 62), 1 << 62)) if span is None else int(rng.integers(0, span))
    return (LONG, False, v)


def random_txn(rng):
    epoch, hlc = int(rng.integers(0, 3)), int(rng.integers(0, 500))
    kind = int(rng.choice([0, 1, 3, 4]))
    node = int(rng.choice([0, 1, 2, 3, -2]))
    return ((epoch << 15) | (hlc >> 48), (hlc << 16) | (kind << 1), node)


def random_doc(rng, n_keys=20, n_txn=30, n_entries=60, n_ranges=10, canonical=False, p_string=0.0, p_double=0.0):
    keys = [random_datum(rng, span=None if rng.random() < 0.5 else 200, p_string=p_string, p_double=p_double)
            for _ in range(n_keys)]
    txns = [random_txn(rng) for _ in range(n_txn)]
    ke = [(keys[int(rng.integers(0, n_keys))], txns[int(rng.integers(0, n_txn))]) for _ in range(int(rng.integers(0, n_entries)))]
    re_ = []
    for _ in range(int(rng.integers(0, n_ranges))):
        a, b = keys[int(rng.integers(0, n_keys))], keys[int(rng.integers(0, n_keys))]
        if datum_order(a) == datum_order(b):
            continue
        if datum_order(a) > datum_order(b):
            a, b = b, a
        re_.append(((a, b), txns[int(rng.integers(0, n_txn))]))
    if canonical:
        ke, re_ = build(ke, re_)
    return ke, re_


# ---------------------------------------------------------------- number and Datum-order edge cases
# Generators for tests/test_json_numbers_gpu.py and tests/test_json_order_gpu.py; tests/test_json_cases.py checks them
# on the CPU. Everything is deterministic (fixed seeds) and cached, so the CPU checks and the GPU tests of one run share
# one computation.

def parse_number(lit: str):
    """Datum.read of a JSON number (JsonReader.nextLong, else nextDouble): an integer literal that fits a long is that
    LONG ("-0" is no PEEKED_LONG); every other literal goes through Double.parseDouble and is LONG when
    (long) d == d -- with Java's saturating cast, so 2^63 reads as Long.MAX_VALUE -- else DOUBLE. An infinity is
    rejected by JsonReader (ValueError here)."""
    if all(c.isdigit() or c == "-" for c in lit):
        v = int(lit)
        if -(1 << 63) <= v < (1 << 63) and lit != "-0":
            return (LONG, False, v)
    d = float(lit)
    if math.isinf(d) or math.isnan(d):
        raise ValueError(lit)
    ll = max(-(1 << 63), min((1 << 63) - 1, int(d)))
    if float(ll) == d:
        return (LONG, False, ll)
    return (DOUBLE, False, d)


def datum_value_bits(d) -> int:
    """dict_value of a non-null LONG / DOUBLE datum: the long, or Double.doubleToLongBits, as an unsigned 64-bit word"""
    kind, _, value = d
    return double_bits(value) if kind == DOUBLE else value & 0xFFFFFFFFFFFFFFFF


def significant_digits(lit: str) -> int:
    """decimal digits of a number literal's mantissa once leading and trailing zeros are stripped"""
    m = lit.lstrip("+-")
    for e in "eE":
        m = m.split(e)[0]
    return len(m.replace(".", "").strip("0"))


def text_digits(s: str) -> int:
    """significant digits of a Double.toString result"""
    return max(1, significant_digits(s))


def has_one_digit_form(x: float) -> bool:
    """some decimal d * 10^j with one digit d rounds to x (so Double.toString's two-digit rule applies)"""
    a = abs(x)
    e = math.floor(math.log10(a))
    return any(float(f"{d}e{ee}") == a for ee in (e - 1, e, e + 1) for d in range(1, 10))


@lru_cache(maxsize=None)
def pow2_doubles():
    """2^k for k in [-1074, -1] and [63, 1023]. An integral double below 2^63 is read back as LONG, so it cannot be
    written as a DOUBLE through the parse; 2^63 itself reads as Long.MAX_VALUE (see parse_number)."""
    return tuple(math.ldexp(1.0, k) for k in list(range(-1074, 0)) + list(range(63, 1024)))


@lru_cache(maxsize=None)
def pow2_neighbours():
    """successor and predecessor of 2^k for 100 values of k over the range: the predecessor has the largest mantissa
    and a symmetric rounding interval, the successor the smallest odd mantissa"""
    out = []
    for k in range(-1072, 1024, 21):
        p = math.ldexp(1.0, k)
        out += [math.nextafter(p, math.inf), math.nextafter(p, 0.0)]
    return tuple(out)


@lru_cache(maxsize=None)
def subnormal_doubles():
    """subnormals by mantissa: 1, 2, 3, 2^51, 2^52 - 1 (the largest) and 100 random ones; then the smallest normal"""
    rng = np.random.default_rng(0x5B)
    ms = [1, 2, 3, 1 << 51, (1 << 52) - 1] + [int(rng.integers(1, 1 << 52)) for _ in range(100)]
    return tuple(math.ldexp(float(m), -1074) for m in ms) + (math.ldexp(1.0, -1022),)


@lru_cache(maxsize=None)
def two_digit_cases():
    """(wins, stays): doubles with a one-digit decimal that rounds to them, split by whether Double.toString (JDK >= 19)
    prints a closer two-digit decimal instead (4.9E-324, 7.9E-323, ...) or keeps the single digit (0.5, 2.0E-3, ...).
    Found by scanning the subnormal mantissas below 5000 and values d * 10^j. A one-digit and a nearer two-digit decimal
    both round to x only where decimals are as dense as doubles: exactly the 8 mantissas 1, 2, 10, 12, 14, 16, 18 and 20
    (2 and 20 print 9.9E-324 and 9.9E-323, a decade below their one-digit decimals 1E-323 and 1E-322); their negative
    copies make 16 wins."""
    cand = [0.5, 2.0e-3] + [math.ldexp(float(m), -1074) for m in range(1, 5000)]
    cand += [float(f"{d}e{j}") for j in list(range(-323, -300)) + list(range(-300, 309, 19)) + [-3, -1] for d in (1, 2, 5, 9)]
    wins, stays = [], []
    for x in dict.fromkeys(cand):
        if x == 0 or math.isinf(x) or not has_one_digit_form(x):
            continue
        n = text_digits(java_double_to_string(x))
        if n == 2:
            wins.append(x)
        elif n == 1:
            stays.append(x)
    return tuple(wins + [-x for x in wins]), tuple(stays[:60])


@lru_cache(maxsize=None)
def layout_doubles():
    """Double.toString's layout boundaries: plain notation for 10^-3 <= |x| < 10^7, else computerized scientific. Maps
    the decimal exponent k10 of the first digit to one non-integral double (k10 from -4 to 8); "edges" holds 0.001, its
    predecessor, both non-integral neighbours of 10^7, and integral doubles >= 2^63 that stay DOUBLE."""
    by_k10 = {k: float(f"1.2345678912345e{k}") for k in range(-4, 9)}
    edges = (0.001, math.nextafter(0.001, 0.0), 9999999.999999998, math.nextafter(1e7, math.inf),
             1.0e23, 2.0e23, 9.223372036854776e18, 1.0e19, math.nextafter(9.223372036854776e18, math.inf))
    return by_k10, edges


@lru_cache(maxsize=None)
def tostring_doubles():
    """every value of the Double.toString section, with a negative copy of each third one"""
    wins, stays = two_digit_cases()
    by_k10, edges = layout_doubles()
    pos = list(pow2_doubles()) + list(pow2_neighbours()) + list(subnormal_doubles()) + list(wins) + list(stays) + \
        list(by_k10.values()) + list(edges)
    pos = list(dict.fromkeys(pos))
    return tuple(dict.fromkeys(pos + [-x for x in pos[::3]]))


def trunc19(q: Fraction):
    """(t, e): the 19-significant-digit truncation t * 10^e of a positive rational, 10^18 <= t < 10^19"""
    e = len(str(q.numerator)) - len(str(q.denominator)) - 18
    while True:
        t = math.floor(q / Fraction(10) ** e)
        if t >= 10 ** 19:
            e += 1
        elif t < 10 ** 18:
            e -= 1
        else:
            return t, e


def lit19(t: int, e: int) -> str:
    return f"{t}e{e}"


def rounds_between(q: Fraction, x: float, y: float) -> float:
    """round-half-even of q in [x, y], y the successor of x, by exact comparison with the midpoint"""
    m = (Fraction(x) + Fraction(y)) / 2
    if q != m:
        return x if q < m else y
    return x if double_bits(x) & 1 == 0 else y


def _straddle(x: float):
    """(x, y, M, below, above): 19-digit literals on both sides of the midpoint M of x and its successor y"""
    y = math.nextafter(x, math.inf)
    m = (Fraction(x) + Fraction(y)) / 2
    t, e = trunc19(m)
    return (x, y, m, lit19(t, e), lit19(t + 1, e))


@lru_cache(maxsize=None)
def midpoint_cases():
    """500 random positive doubles from the whole exponent range (60 of them subnormal), each with the 19-digit
    truncation of the midpoint to its successor and that truncation plus one unit in the 19th place"""
    rng = np.random.default_rng(0x3D)
    xs = [struct.unpack(">d", struct.pack(">Q", int(rng.integers(1, 1 << 52))))[0] for _ in range(60)]
    while len(xs) < 500:
        b = (int(rng.integers(1, 0x7FF)) << 52) | int(rng.integers(0, 1 << 52))
        x = struct.unpack(">d", struct.pack(">Q", b))[0]
        if math.isfinite(math.nextafter(x, math.inf)):
            xs.append(x)
    return tuple(_straddle(x) for x in xs)


@lru_cache(maxsize=None)
def seam_cases():
    """the subnormal / normal seam: the midpoint between the largest subnormal and 2^-1022, the midpoint above 2^-1022,
    and 2^-1022 itself approached from below (a literal that rounds up into it) and from above"""
    big_sub, min_norm = math.ldexp(float((1 << 52) - 1), -1074), math.ldexp(1.0, -1022)
    t, e = trunc19(Fraction(min_norm))
    return (_straddle(big_sub), _straddle(min_norm), _straddle(math.nextafter(big_sub, 0.0))), (lit19(t, e), lit19(t + 1, e))


def _dec(q: Fraction) -> str:
    """exact decimal text of a dyadic rational with a fraction part"""
    n, s = q.numerator // q.denominator, ""
    r = q - n
    while r:
        r *= 10
        s += str(r.numerator // r.denominator)
        r -= r.numerator // r.denominator
    return f"{n}.{s or '0'}"


@lru_cache(maxsize=None)
def exact_tie_literals():
    """midpoints between two doubles that fit in 19 digits, both parities of the lower neighbour: (literal, lower,
    upper). The listed ones, then 16 drawn from [2^50, 2^54) (4 per binade, even and odd lower mantissas)."""
    rng = np.random.default_rng(0x71E)
    lows = [9007199254740992.0, 9007199254740994.0, 2251799813685248.0, 2251799813685248.5, 4503599627370496.0,
            4503599627370497.0]
    for k in (50, 51, 52, 53):
        for j in range(4):
            m = (int(rng.integers(0, 1 << 51)) << 1) | (j & 1)
            lows.append(math.ldexp(float((1 << 52) | m), k - 52))
    out = []
    for x in lows:
        y = math.nextafter(x, math.inf)
        out.append((_dec((Fraction(x) + Fraction(y)) / 2), x, y))
    return tuple(out)


ZERO_BOUNDARY = ("2.470328229206232720e-324", "2.470328229206232721e-324", "1e-400", "0e999999999", "1e-999999999",
                 "0." + "0" * 400 + "1")
MAX_DOUBLE_LITERAL = "1.797693134862315807e308"                         # just below the midpoint to 2^1024
INFINITY_LITERALS = ("1.797693134862315808e308", "1e309", "1e999999999")   # each rejected (JsonReader: no infinities)
CLINGER = tuple(f"{m}e{e}" for m in (1 << 53, (1 << 53) + 1) for e in (22, -22, 23, -23)) + \
    tuple(f"1234567890123456789e{e}" for e in (-30, 0, 30))
LITERAL_FORMS = ("1E+2", "1e-0", "1.50", "100000000000000000000e-20", "1.0000000000000000000", "-9223372036854775808",
                 "-9223372036854775809", "10000000000000000000", "0.000000000000000000001")
# rejected: 20 nonzero significant digits (the device path's documented limit), then forms peekNumber does not take
NUMBER_REJECTS = ("1.2345678912345678912", "1.", ".5", "1e", "+1", "-01", "1.5x")


@lru_cache(maxsize=None)
def parse_literals():
    """every accepted literal of the Double.parseDouble section, in a fixed order"""
    out = []
    for _, _, _, lo, hi in midpoint_cases():
        out += [lo, hi]
    out += [t for t, _, _ in exact_tie_literals()]
    out += list(ZERO_BOUNDARY) + [MAX_DOUBLE_LITERAL]
    pairs, around = seam_cases()
    for _, _, _, lo, hi in pairs:
        out += [lo, hi]
    out += list(around) + list(CLINGER) + list(LITERAL_FORMS)
    return tuple(out)


def _i64(v):
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= 1 << 63 else v


def _bits_double(b: int) -> float:
    return struct.unpack(">d", struct.pack(">Q", b))[0]


def block_string(n_blocks: int, flipped=()) -> str:
    """"Aa" blocks with the given ones replaced by "BB": "Aa".hashCode() == "BB".hashCode(), so block strings of one
    length share String.hashCode"""
    return "".join("BB" if i in flipped else "Aa" for i in range(n_blocks))


@lru_cache(maxsize=None)
def collision_groups():
    """name -> datums that share Datum.hash, so that kind, null and the value decide Datum.compareTo"""
    g = {}
    # LONG: Long.hashCode = (int)(v ^ v >>> 32) -> low word = high word ^ c
    for name, c, highs in (("long_0", 0, (0, 0xFFFFFFFF, 1, 0x80000000, 5, 0xFFFFFFFE, 0x7FFFFFFF)),
                           ("long_c", 0x12345678, (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF, 0x40000000))):
        g[name] = tuple((LONG, False, _i64((h << 32) | (h ^ c))) for h in highs)
    # DOUBLE: Double.hashCode folds the bits the same way; two positives, two negatives, and +x / -x pairs
    c = 0x000ABCDE
    g["double_c"] = tuple((DOUBLE, False, _bits_double((h << 32) | (h ^ c)))
                          for h in (0x3FF00000, 0x40590000, 0xBFF00000, 0xC0590000, 0x3FE80000, 0xBFE80000))
    # STRING: equal-length "Aa" / "BB" block strings, first differing at byte 0, 6, 8 and 14
    for n in (8, 9):
        g[f"string_{2 * n}"] = tuple((STRING, False, block_string(n, f)) for f in ((), (0,), (3,), (4,), (7,), (3, 7), (4, 7)))
    # every kind on the hash of hashCode 0, and on Integer.MAX_VALUE (the null sentinels' hash)
    crc0 = datum_hash(LONG, False, 0)
    g["cross_0"] = ((STRING, False, ""), (LONG, False, 0), (LONG, False, -1), (DOUBLE, False, _bits_double(0x3FF000003FF00000)),
                    (DOUBLE, False, _bits_double(0xBFF00000BFF00000)), (HASH, False, crc0))
    g["cross_max"] = ((HASH, False, 0x7FFFFFFF), (STRING, True, 0), (LONG, True, 0), (DOUBLE, True, 0), (HASH, True, 0))
    return g


def collision_docs(rng, n_docs=40):
    """documents whose keys and range ends mix the collision groups' datums with ordinary random ones, unsorted and
    with duplicates: [(key_entries, range_entries)]"""
    special = [d for ds in collision_groups().values() for d in ds]
    docs = []
    for _ in range(n_docs):
        pool = [special[int(i)] for i in rng.integers(0, len(special), size=14)] + \
               [random_datum(rng, p_string=0.3, p_double=0.3, span=None if rng.random() < 0.5 else 200) for _ in range(6)]
        txns = [random_txn(rng) for _ in range(8)]
        ke = [(pool[int(rng.integers(0, len(pool)))], txns[int(rng.integers(0, 8))]) for _ in range(int(rng.integers(8, 32)))]
        re_ = []
        for _ in range(int(rng.integers(2, 12))):
            a, b = pool[int(rng.integers(0, len(pool)))], pool[int(rng.integers(0, len(pool)))]
            if datum_order(a) == datum_order(b):
                continue
            if datum_order(a) > datum_order(b):
                a, b = b, a
            re_.append(((a, b), txns[int(rng.integers(0, 8))]))
        docs.append((ke, re_))
    return docs
