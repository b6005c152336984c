"""Shared RangeDeps test batches (CPU oracle tests and GPU parity tests)."""
import numpy as np

from accord_amd import workload as W


def build(txns, end_inclusive=1):
    """txns: list of dicts {kind, status, keys | ranges, bump (executeAt hlc offset, 0 = executeAt == txnId)}
    in TxnId order (hlc = index + 1). Returns a RangeBatch."""
    n = len(txns)
    i = np.arange(n, dtype=np.int64)
    isr = np.array([1 if "ranges" in t else 0 for t in txns], np.int64)
    kind = np.array([t.get("kind", W.WRITE) for t in txns], np.int64)
    t_msb, t_lsb, t_node = W.encode_ts(np.ones(n), i + 1, (kind << 1) | isr, 1 + (i % 8))
    bump = np.array([t.get("bump", 0) for t in txns], np.int64)
    e_msb, e_lsb, e_node = W.encode_ts(np.ones(n), i + 1 + bump, np.zeros(n), 1000 + (i % 1024))
    exe_msb = np.where(bump > 0, e_msb, t_msb).astype(np.uint64)
    exe_lsb = np.where(bump > 0, e_lsb, t_lsb).astype(np.uint64)
    exe_node = np.where(bump > 0, e_node, t_node).astype(np.int32)
    status = np.array([t.get("status", W.PREACCEPTED) for t in txns], np.uint8)
    keys = [np.array(sorted(t.get("keys", [])), np.uint64) for t in txns]
    ranges = [t.get("ranges", []) for t in txns]
    key_off = np.zeros(n + 1, np.uint32)
    np.cumsum([len(k) for k in keys], out=key_off[1:])
    rng_off = np.zeros(n + 1, np.uint32)
    np.cumsum([len(r) for r in ranges], out=rng_off[1:])
    kc = np.concatenate(keys) if n else np.zeros(0, np.uint64)
    rs = np.array([s for r in ranges for s, _ in r], np.uint64)
    re = np.array([e for r in ranges for _, e in r], np.uint64)
    kb = W.Batch(t_msb, t_lsb, t_node, exe_msb, exe_lsb, exe_node, status, key_off, kc.astype(np.uint64))
    return W.RangeBatch(kb, rng_off, rs, re, end_inclusive)


def handmade(end_inclusive=1):
    """Boundary keys, duplicate stored ranges, a range covering two keys of one txn, Accept-style range txn (p1),
    an erased range command, kind filters, multi-range txns."""
    R, K = W.READ, W.WRITE
    return build([
        dict(kind=K, ranges=[(10, 20)]),                                  # 0
        dict(kind=K, ranges=[(10, 20), (30, 40)]),                        # 1 same (10,20) as 0: one stored range
        dict(kind=R, ranges=[(15, 35)]),                                  # 2 a read: only writes witness it
        dict(kind=K, ranges=[(0, 100)], status=W.INVALID_OR_TRUNCATED),   # 3 erased range command
        dict(kind=K, keys=[10, 11, 20, 21, 30, 40]),                      # 4 boundary keys of 0/1/2
        dict(kind=R, keys=[12, 18]),                                      # 5 both keys in (10,20]: one entry per cmd
        dict(kind=K, ranges=[(5, 12)], bump=3),                           # 6 Accept-style: executeAt past txn 8
        dict(kind=K, ranges=[(11, 13)]),                                  # 7
        dict(kind=W.SYNC_POINT, ranges=[(0, 50)]),                        # 8
        dict(kind=W.EXCLUSIVE_SYNC_POINT, keys=[12]),                     # 9 ESP witnesses SyncPoints
        dict(kind=R, ranges=[(19, 31)], status=W.APPLIED),                # 10 range query over ranges
        dict(kind=K, keys=[15], status=W.INVALID_OR_TRUNCATED),           # 11 invalid key txn still queries
    ], end_inclusive)


def dense(seed, n=3000, end_inclusive=1, ranges_per_txn=2, key_bits=12, max_width_log2=8, p_range=0.5):
    return W.rangedeps_batch(n, seed, p_range=p_range, keys_per_txn=4, ranges_per_txn=ranges_per_txn, key_bits=key_bits,
                             max_width_log2=max_width_log2, window=n // 3, p_syncpoint=0.05,
                             end_inclusive=end_inclusive)


def global_tier(n_cmds=9000):
    """One key txn after n_cmds range commands that all cover it: a txn beyond the LDS tiers."""
    txns = [dict(kind=W.WRITE, ranges=[(i % 7, 1000 + (i % 13))]) for i in range(n_cmds)]
    txns += [dict(kind=W.WRITE, keys=[500, 501])]
    txns += [dict(kind=W.WRITE, ranges=[(400, 600)])]
    return build(txns)


# ---------------------------------------------------------------- bound families for the bit-compaction plans

U64 = 2**64 - 1
SPARSE = sum(1 << b for b in range(0, 61, 3))        # bits 0, 3, .., 60: 21 runs of one bit
# name -> (fixed prefix, mask of the bits that vary in a query low bound)
FAMILIES = {
    "top3": (0b010 << 61, (1 << 61) - 1),             # top 3 bits constant: 61 query bits
    "top2": (0b01 << 62, (1 << 62) - 1),              # 62: the range bit only
    "top1": (0, (1 << 63) - 1),                       # 63
    "full": (0, U64),                                 # 64: keys and ranges mixed
    "sparse": (0b010 << 61, SPARSE),                  # more than Runs::MAX_RUNS runs: the hull
    "d32": (0, (1 << 32) - 1),                        # every bound below 2^32: a 64-bit dictionary key, not split
    "d33": (0, (1 << 32) - 1),                        # the same and one end at 2^32: 65 bits, split
    "e64": (0, U64),                                  # every start 0, ends over 64 bits: a shift by the full width
}
# what the plans must come to, where the family fixes it (else the tests compute it from the bounds alone)
FAMILY_QUERY_BITS = {"top3": 61, "top2": 62, "top1": 63, "full": 64, "sparse": 61, "e64": 64}
FAMILY_DICT = {"d32": (64, 0), "d33": (65, 1), "e64": (64, 0)}


def plan_bits(mask):
    """Bits of the compaction plan of an OR-mask (make_runs, csrc/prims.hpp): its set bits, or beyond 12 runs of set
    bits the hull from the lowest to the highest."""
    mask = int(mask)
    if mask == 0:
        return 0
    runs = bin(mask & ~(mask << 1) & U64).count("1")      # set bits with a clear bit (or nothing) below them
    if runs > 12:
        return mask.bit_length() - ((mask & -mask).bit_length() - 1)
    return bin(mask).count("1")


def or_mask(values, ref=0):
    """OR over values ^ ref (numpy u64)."""
    v = np.asarray(values, np.uint64)
    return int(np.bitwise_or.reduce(v ^ np.uint64(ref))) if len(v) else 0


def family(name, seed, end_inclusive):
    """Range commands and queries whose query low bounds (keys and range starts) are `prefix | (random & vary)`.
    -> dict(cmds=[[(s, e)..]] (about 400 commands), keyq=[[key..]] (about 300), rngq=[[(s, e)..]] (about 300)).
    The first key and the second are complements in the varying bits, so the XOR mask against the first low bound has
    every varying bit. Command widths reach every width class (4^c for c = 0..31, 2^62 + 1 for class 32) where the
    family leaves room; other commands run between two family values, so their ends are family values too and a key
    can equal an end (contained under end_inclusive = 1) or a start (contained under 0)."""
    prefix, vary = FAMILIES[name]
    rng = np.random.RandomState(seed)

    def val():
        return prefix | (int(rng.randint(0, 2**32, dtype=np.int64)) << 32 | int(rng.randint(0, 2**32, dtype=np.int64))) & vary

    singles, between = [], 0
    if name == "e64":
        x = val() | 1
        ends = [x, U64 ^ x | 2, U64, 1] + [val() | 1 for _ in range(396)]
        singles = [(0, e) for e in ends]
    else:
        top = (1 << 32) if name in ("d32", "d33") else U64 + 1
        for c in range(33):
            w = 4**c if c < 32 else 2**62 + 1
            for _ in range(6):
                s = val()
                if s + w < top:
                    singles.append((s, s + w))
        between = len(singles)                            # from here: ranges between two family values
        while len(singles) < 400:
            a, b = val(), val()
            if a != b:
                singles.append((min(a, b), max(a, b)))
        if name == "d33":
            singles.append((2**32 - 5, 2**32))
        if name == "full":
            singles += [(0, 1), (U64 - 1, U64), (2**63 - 1, 2**63), (2**63, 2**63 + 1)]
    cmds = []
    i = 0
    while i < len(singles):                               # every fifth command takes two ranges when they do not overlap
        if i % 5 == 0 and i + 1 < len(singles) and name != "e64":
            a, b = sorted(singles[i:i + 2])
            if a[1] <= b[0]:
                cmds.append([a, b]); i += 2
                continue
        cmds.append([singles[i]]); i += 1
    x = val()
    keyq = [[x], [prefix | (x ^ vary) & vary]]
    if name == "full":
        keyq += [[0], [U64], [0, U64], [2**63 - 1, 2**63]]
    fits = lambda k: 0 <= k <= U64 and (k & ~vary & U64) == prefix  # noqa: E731
    for s, e in singles[::3]:                             # keys on and next to the bounds of stored ranges
        ks = sorted({k for k in (s, s + 1, e - 1, e, e + 1 if e < U64 else e, (s + e) // 2) if fits(k)})
        if ks:
            keyq.append(ks[:3] if len(keyq) % 2 else ks[-3:])
    hit = singles[between][1 if end_inclusive else 0]     # a key equal to a range's end (ei = 1) / start (ei = 0)
    assert fits(hit)
    keyq.append([hit])
    while len(keyq) < 300:
        keyq.append(sorted({val() for _ in range(int(rng.randint(1, 4)))}))
    rngq = []
    while len(rngq) < 300:
        if name == "e64":
            rngq.append([(0, val() | 1)])
            continue
        s = val()
        w = 1 << int(rng.randint(0, 62)) if len(rngq) % 2 else 1 + int(rng.randint(0, 1 << (4 * (len(rngq) // 2 % 4) + 2)))
        e = min(s + w, (1 << 32) - 1 if name in ("d32", "d33") else U64)
        if s >= e:
            continue
        r = [(s, e)]
        s2 = val()
        if len(rngq) % 7 == 0 and s2 >= e and s2 < U64 and name not in ("d32", "d33"):
            r.append((s2, s2 + 1))
        rngq.append(r)
    return dict(cmds=cmds, keyq=keyq, rngq=rngq)


def family_batch(name, seed, end_inclusive):
    """The family as one acc_rangedeps_batch: its commands (reads and writes, a few erased), then its key queries, then
    its range queries, every seventh txn with a bumped executeAt."""
    f = family(name, seed, end_inclusive)
    txns = [dict(kind=W.WRITE if i % 3 else W.READ, ranges=r,
                 status=W.INVALID_OR_TRUNCATED if i % 41 == 40 else W.PREACCEPTED) for i, r in enumerate(f["cmds"])]
    txns += [dict(kind=W.WRITE if i % 2 else W.READ, keys=k) for i, k in enumerate(f["keyq"])]
    txns += [dict(kind=W.WRITE if i % 4 else W.EXCLUSIVE_SYNC_POINT, ranges=r) for i, r in enumerate(f["rngq"])]
    for i in range(0, len(txns), 7):
        txns[i]["bump"] = 5 + i % 11
    return build(txns, end_inclusive)


def batch_plan_bits(rb):
    """The plans acc_rangedeps_batch takes for a batch, from its bounds: every mask is the OR of a column XOR its first
    element (the query low bounds = the keys and every range start, against the first key)."""
    kc, rs, re = rb.keys.key_code, rb.rng_start, rb.rng_end
    ref_lo = int(kc[0]) if len(kc) else int(rs[0])
    q = plan_bits(or_mask(kc, ref_lo) | or_mask(rs, ref_lo))
    d = plan_bits(or_mask(rs, int(rs[0]))) + plan_bits(or_mask(re, int(re[0])))
    return dict(query_bits=q, dict_bits=d, dict_split=int(d > 64))


def width_classes(rs, re):
    """The width class of each range: the smallest c with end - start <= 4^c."""
    return [((int(e) - int(s) - 1).bit_length() + 1) >> 1 for s, e in zip(rs, re)]


def wide_codes(seed, n=2000):
    """u64 codes spanning the full range (split dictionary and class sorts), widths up to 2^62."""
    rng = np.random.RandomState(seed)
    txns = []
    for t in range(n):
        if rng.rand() < 0.5:
            s = int(rng.randint(0, 2**62, dtype=np.int64)) * 3
            w = 1 << int(rng.randint(0, 62))
            txns.append(dict(kind=int(rng.randint(0, 2)), ranges=[(s, min(s + w, 2**64 - 1))]))
        else:
            ks = sorted({int(rng.randint(0, 2**62, dtype=np.int64)) * 3 + int(rng.randint(0, 3)) for _ in range(3)})
            txns.append(dict(kind=int(rng.randint(0, 2)), keys=ks))
    return build(txns)
