"""A plain numpy decoder of one KeyDeps fragment message, written from the format description at the top of
csrc/fragwire.hip (not from its kernels): the reference the wire codec's tests decode captured messages with.

A message is a 64-byte header (16 little-endian u32 words: magic, flags, nfrag, G, kbase as two words, five u64 section
sizes) and five sections, each padded to 8 bytes: slots (a bitmap of G bits, or a u32 list), counts ((nk, nv, TxnId
bytes) per fragment as u16 or u32), keys (u32 offsets from kbase, or u64 codes), TxnIds (LEB128 varints per fragment:
the first is the zigzag of its difference from the fragment's txn t, the others are the gap to the previous TxnId minus
one) and key bits (per fragment with two or more keys an nk x nv bit matrix, bit k * nv + e set when key k lists TxnId
e; a single key lists every TxnId and sends no bits). The txn of the fragment in slot g sent to home rank `dest` of
`world` ranks is t = dest + g * world.
"""
from dataclasses import dataclass

import numpy as np

MAGIC = 0x4B464341
F_SLOT_LIST, F_WIDE_CNT, F_WIDE_KEY = 1, 2, 4
HEADER_BYTES = 64
SECTIONS = ("slots", "counts", "keys", "txn_ids", "key_bits")


@dataclass
class Header:
    magic: int
    flags: int
    nfrag: int
    G: int
    kbase: int
    sizes: tuple        # the five section byte sizes, in SECTIONS order

    @property
    def form(self):
        """(slot list, wide counts, wide keys)"""
        return bool(self.flags & F_SLOT_LIST), bool(self.flags & F_WIDE_CNT), bool(self.flags & F_WIDE_KEY)


@dataclass
class Fragments:
    """One message's fragments as acc_shard_pack lays them out, plus what the tests ask about the varints."""
    header: Header
    hdr: np.ndarray          # u32 [4 * nfrag]: (t, nk, nv, no) per fragment
    keys: np.ndarray         # u64
    vals: np.ndarray         # u32, global txn indices
    k2v: np.ndarray          # i32, keysToTxnIds per fragment
    varint_len: np.ndarray   # bytes of each TxnId's varint, in stream order
    first_delta: np.ndarray  # per fragment: its first TxnId minus t (the zigzag value's sign)


def parse_header(msg) -> Header:
    raw = np.frombuffer(bytes(msg[:HEADER_BYTES]), dtype="<u4")
    if len(raw) != 16:
        raise ValueError("message shorter than its header")
    w = [int(x) for x in raw]
    return Header(w[0], w[1], w[2], w[3], w[4] | (w[5] << 32), tuple(w[6 + 2 * q] | (w[7 + 2 * q] << 32) for q in range(5)))


def _varints(raw: np.ndarray):
    """Every LEB128 varint of a byte string: (values u64, lengths). A byte below 0x80 ends a varint."""
    if len(raw) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    last = raw < 0x80
    if not last[-1]:
        raise ValueError("TxnId bytes end inside a varint")
    first = np.concatenate([[True], last[:-1]])
    which = np.cumsum(first) - 1                              # the varint each byte belongs to
    place = np.arange(len(raw)) - np.nonzero(first)[0][which]   # the byte's position inside it
    if place.max() > 9:
        raise ValueError("varint longer than ten bytes")
    out = np.zeros(int(which[-1]) + 1, np.uint64)
    np.add.at(out, which, (raw & 0x7F).astype(np.uint64) << (7 * place).astype(np.uint64))
    return out, np.bincount(which)


def _ramp(counts):
    """0 .. c-1 for every c of counts, concatenated"""
    start = np.concatenate([[0], np.cumsum(counts)])
    return np.arange(int(start[-1]), dtype=np.int64) - np.repeat(start[:-1], counts)


def decode(msg, world: int, dest: int) -> Fragments:
    msg = np.frombuffer(bytes(msg), dtype=np.uint8)
    h = parse_header(msg)
    if h.magic != MAGIC:
        raise ValueError("not a fragment message")
    if h.flags & ~(F_SLOT_LIST | F_WIDE_CNT | F_WIDE_KEY):
        raise ValueError("unknown flags")
    if any(s % 8 for s in h.sizes) or HEADER_BYTES + sum(h.sizes) != len(msg):
        raise ValueError("section sizes do not add up to the message")
    sec, pos = {}, HEADER_BYTES
    for name, size in zip(SECTIONS, h.sizes):
        sec[name] = msg[pos:pos + size]
        pos += size
    lst, wide_cnt, wide_key = h.form
    n = h.nfrag

    def take(name, nbytes):
        """The section's content: nbytes, then only zero padding up to the next multiple of 8."""
        s = sec[name]
        if len(s) != (nbytes + 7) // 8 * 8 or s[nbytes:].any():
            raise ValueError(f"{name}: {len(s)} bytes for {nbytes} of content")
        return s[:nbytes].tobytes()

    # slots -> txns
    if n == 0:
        slots = np.zeros(0, np.int64)
        take("slots", 0)
    elif lst:
        slots = np.frombuffer(take("slots", 4 * n), "<u4").astype(np.int64)
        if (np.diff(slots) <= 0).any():
            raise ValueError("slot list not ascending")
    else:
        words = (h.G + 31) // 32
        bits = np.unpackbits(np.frombuffer(take("slots", 4 * words), np.uint8), bitorder="little")
        slots = np.nonzero(bits)[0].astype(np.int64)
        if len(slots) != n:
            raise ValueError("bitmap population differs from nfrag")
    if n and slots[-1] >= h.G:
        raise ValueError("slot past G")
    t = dest + slots * world
    # counts
    cnt = np.frombuffer(take("counts", n * (12 if wide_cnt else 6)), "<u4" if wide_cnt else "<u2").astype(np.int64)
    cnt = cnt.reshape(n, 3)
    nk, nv, vb = cnt[:, 0], cnt[:, 1], cnt[:, 2]
    if n and (nk.min() < 1 or nv.min() < 1):
        raise ValueError("a fragment without keys or TxnIds")
    # keys
    NK = int(nk.sum())
    if wide_key:
        keys = np.frombuffer(take("keys", 8 * NK), "<u8").astype(np.uint64)
    else:
        keys = np.frombuffer(take("keys", 4 * NK), "<u4").astype(np.uint64) + np.uint64(h.kbase)
    # TxnIds
    codes, lens = _varints(np.frombuffer(take("txn_ids", int(vb.sum())), np.uint8))
    NV = int(nv.sum())
    if len(codes) != NV:
        raise ValueError("TxnId count differs from the fragments' nv")
    v0 = np.concatenate([[0], np.cumsum(nv)])
    if not np.array_equal(np.add.reduceat(lens, v0[:-1]) if n else np.zeros(0, np.int64), vb):
        raise ValueError("a fragment's TxnId bytes differ from its count entry")
    first = v0[:-1]
    z = codes[first].astype(np.int64) if n else np.zeros(0, np.int64)   # (a zigzag of a u32 difference: below 2^33)
    first_delta = (z >> 1) ^ -(z & 1)
    step = codes.astype(np.int64) + 1
    step[first] = t + first_delta
    run = np.cumsum(step)
    vals = run - np.repeat(run[first] - step[first], nv) if n else np.zeros(0, np.int64)
    if NV and (vals.min() < 0 or vals.max() > 0xFFFFFFFF):
        raise ValueError("TxnId outside u32")
    # key bits -> keysToTxnIds: the end of every key's list (counted from nk), then the lists
    kb = np.where(nk >= 2, (nk * nv + 7) // 8, 0)
    allbits = np.frombuffer(take("key_bits", int(kb.sum())), np.uint8)
    b0 = np.concatenate([[0], np.cumsum(kb)])
    lists = {}
    no = nk + nv                                  # one key: it lists every TxnId
    for f in np.nonzero(nk >= 2)[0].tolist():
        k, v = int(nk[f]), int(nv[f])
        bits = np.unpackbits(allbits[b0[f]:b0[f + 1]], bitorder="little")
        if bits[k * v:].any():
            raise ValueError("key bits set past nk * nv")
        rows = bits[:k * v].reshape(k, v).astype(bool)
        lists[f] = np.concatenate([k + np.cumsum(rows.sum(axis=1)), np.nonzero(rows)[1]])
        no[f] = len(lists[f])
    o0 = np.concatenate([[0], np.cumsum(no)])
    k2v = np.zeros(int(o0[-1]), np.int64)
    one = np.nonzero(nk == 1)[0]
    k2v[o0[one]] = 1 + nv[one]
    k2v[np.repeat(o0[one] + 1, nv[one]) + _ramp(nv[one])] = _ramp(nv[one])
    for f, a in lists.items():
        k2v[o0[f]:o0[f + 1]] = a
    hdr = np.stack([t, nk, nv, no], axis=1).astype(np.uint32).reshape(-1) if n else np.zeros(0, np.uint32)
    return Fragments(h, hdr, keys, vals.astype(np.uint32),
                     k2v.astype(np.int32), lens, first_delta)
