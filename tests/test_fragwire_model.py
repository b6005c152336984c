"""The independent wire-format model (tests/fragwire_model.py) against two messages assembled by hand from the format
description in csrc/fragwire.hip: one in the bitmap / u16-count / u32-key form, one in the list / u32-count / u64-key
form, each with a one-key and a three-key fragment. They pin the model without any GPU run; test_fragwire_gpu.py then
holds the kernels to the model."""
import numpy as np
import pytest

import fragwire_model as M


def _hex(*parts):
    return bytes.fromhex("".join(parts))


# world 2, home rank 1, n_global 80 -> G = 40 (a bitmap of two words; two fragments are denser than 1 in 32)
#   slot 3  (t = 7):  key 1000; TxnIds 2, 5 (first 5 below t: zigzag 9; gap 3 - 1 = 2)
#   slot 39 (t = 79): keys 1000, 1003, 1300; TxnIds 143, 271, 400 (first 64 above t: zigzag 128 = 80 01; gaps 128 and
#                     129 minus one: 7F, 80 01); key 0 lists TxnIds {0, 2}, key 1 {1}, key 2 {0, 1, 2}: bits 0, 2, 4, 6,
#                     7, 8 of the 3 x 3 matrix = D5 01
BITMAP_MSG = _hex(
    "4143464b", "00000000", "02000000", "28000000",    # magic "ACFK", flags, nfrag, G
    "e8030000", "00000000",                            # kbase 1000
    "0800000000000000", "1000000000000000", "1000000000000000", "0800000000000000", "0800000000000000",
    "08000000", "80000000",                            # bitmap: bit 3 of word 0, bit 7 of word 1
    "0100", "0200", "0200", "0300", "0300", "0500", "00000000",   # (nk, nv, bytes) x 2 as u16, padded
    "00000000", "00000000", "03000000", "2c010000",    # key offsets from kbase
    "0902", "80017f8001", "00",                        # TxnId varints, padded
    "d501", "000000000000")                            # key bits of the second fragment, padded

# world 3, home rank 2, n_global 3000 -> G = 1000 (a bitmap would be 32 words: two fragments go as a list)
#   slot 100 (t = 302):  key 2^63 - 1; TxnIds 238, 16622, 33007 (first 64 below t: zigzag 127 = 7F; gaps minus one 16383
#                        = FF 7F and 16384 = 80 80 01)
#   slot 999 (t = 2999): keys 7, 2^32 + 7, 2^63 + 1; TxnIds 0, 1 (first 2999 below t: zigzag 5997 = ED 2E; gap minus one
#                        0); key 0 lists {1}, key 1 {0}, key 2 {0, 1}: bits 1, 2, 4, 5 of the 3 x 2 matrix = 36
LIST_MSG = _hex(
    "4143464b", "07000000", "02000000", "e8030000",
    "07000000", "00000000",                            # kbase 7, the smallest key
    "0800000000000000", "1800000000000000", "2000000000000000", "1000000000000000", "0800000000000000",
    "64000000", "e7030000",                            # slots 100, 999
    "01000000", "03000000", "06000000", "03000000", "02000000", "03000000",
    "ffffffffffffff7f", "0700000000000000", "0700000001000000", "0100000000000080",
    "7fff7f808001", "ed2e00", "00000000000000",
    "36", "00000000000000")


def test_bitmap_u16_u32key_message():
    assert len(BITMAP_MSG) == 120
    m = M.decode(BITMAP_MSG, world=2, dest=1)
    assert m.header == M.Header(M.MAGIC, 0, 2, 40, 1000, (8, 16, 16, 8, 8))
    assert m.header.form == (False, False, False)
    np.testing.assert_array_equal(m.hdr, [7, 1, 2, 3, 79, 3, 3, 9])
    np.testing.assert_array_equal(m.keys, [1000, 1000, 1003, 1300])
    np.testing.assert_array_equal(m.vals, [2, 5, 143, 271, 400])
    np.testing.assert_array_equal(m.k2v, [3, 0, 1, 5, 6, 9, 0, 2, 1, 0, 1, 2])
    np.testing.assert_array_equal(m.varint_len, [1, 1, 2, 1, 2])
    np.testing.assert_array_equal(m.first_delta, [-5, 64])
    assert (m.hdr.dtype, m.keys.dtype, m.vals.dtype, m.k2v.dtype) == (np.uint32, np.uint64, np.uint32, np.int32)


def test_list_u32_u64key_message():
    assert len(LIST_MSG) == 152
    m = M.decode(LIST_MSG, world=3, dest=2)
    assert m.header == M.Header(M.MAGIC, 7, 2, 1000, 7, (8, 24, 32, 16, 8))
    assert m.header.form == (True, True, True)
    np.testing.assert_array_equal(m.hdr, [302, 1, 3, 4, 2999, 3, 2, 7])
    np.testing.assert_array_equal(m.keys, np.array([(1 << 63) - 1, 7, (1 << 32) + 7, (1 << 63) + 1], np.uint64))
    np.testing.assert_array_equal(m.vals, [238, 16622, 33007, 0, 1])
    np.testing.assert_array_equal(m.k2v, [4, 0, 1, 2, 4, 5, 7, 1, 0, 0, 1])
    np.testing.assert_array_equal(m.varint_len, [1, 2, 3, 2, 1])
    np.testing.assert_array_equal(m.first_delta, [-64, -2999])


def test_empty_message():
    msg = _hex("4143464b", "00000000", "00000000", "28000000") + bytes(48)
    m = M.decode(msg, world=2, dest=0)
    assert m.header.nfrag == 0 and m.header.sizes == (0, 0, 0, 0, 0)
    assert len(m.hdr) == len(m.keys) == len(m.vals) == len(m.k2v) == len(m.varint_len) == 0


@pytest.mark.parametrize("at,byte,what", [(0, 0x40, "not a fragment message"), (4, 0x08, "unknown flags"),
                                          (24, 0x10, "section sizes"), (64, 0x0C, "population"),
                                          (110, 0x81, "varint")])
def test_model_rejects(at, byte, what):
    """The model refuses a message it cannot account for byte by byte, so a test that decodes a captured message
    with it also checks the padding, the bitmap population and the varint framing."""
    bad = bytearray(BITMAP_MSG)
    bad[at] = byte
    with pytest.raises(ValueError, match=what):
        M.decode(bytes(bad), world=2, dest=1)


def test_shard_batch_keeps_txns_without_keys():
    """sharded.shard_batch on a batch with keyless txns, trailing ones included (it indexed past the key array)"""
    from accord_amd import sharded as S
    from accord_amd import workload as W
    n = 6
    ts = W.encode_ts(np.ones(n), np.arange(n) + 1, np.full(n, W.WRITE << 1), np.ones(n))
    off = np.array([0, 1, 3, 3, 4, 4, 4], np.uint32)
    b = W.Batch(*ts, *ts, np.full(n, W.PREACCEPTED, np.uint8), off, np.array([5, 9, 20, 7], np.uint64))
    lo, hi = (S.shard_batch(b, np.array([0, 8, 30], np.uint64), r) for r in range(2))
    np.testing.assert_array_equal(lo.key_off, [0, 1, 1, 1, 2, 2, 2])
    np.testing.assert_array_equal(lo.key_code, [5, 7])
    np.testing.assert_array_equal(hi.key_off, [0, 0, 2, 2, 2, 2, 2])
    np.testing.assert_array_equal(hi.key_code, [9, 20])
    sub, g = S.store_batch(b, np.array([0, 8, 30], np.uint64), 0)
    np.testing.assert_array_equal(g, [0, 3])
    np.testing.assert_array_equal(sub.key_off, [0, 1, 2])


def test_harness_reference_helpers():
    """The harness's own references on the CPU: the placement-aware expected view equals sharded.home_result_from_full
    for the identity placement, and the varint lengths follow LEB128's 7-bit groups."""
    import oracle
    import fragwire_harness as H
    from accord_amd import sharded as S
    from accord_amd import workload as W
    b = W.keydeps_batch(500, 3, 60, 0xF4A8, "zipf", 0.99, status_model="model", window=200)
    full = oracle.keydeps_batch(b)
    for world in (1, 3):
        for r in range(world):
            want, got = S.home_result_from_full(full, b, r, world), H.expected_home(full, b, None, b.n_txn, r, world)
            for f in H.MERGE_FIELDS:
                np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    # a placement: every txn three global txns apart, after two empty ones
    g = (3 * np.arange(b.n_txn) + 2).astype(np.uint32)
    got, want = H.expected_home(full, b, g, int(g[-1]) + 1, 0, 1), S.home_result_from_full(full, b, 0, 1)
    np.testing.assert_array_equal(np.diff(got["key_off"].astype(np.int64))[2::3], np.diff(want["key_off"].astype(np.int64)))
    np.testing.assert_array_equal(got["key_code"], want["key_code"])
    np.testing.assert_array_equal(got["txn_rank"], g[want["txn_rank"].astype(np.int64)])
    np.testing.assert_array_equal(H.varint_bytes([0, 127, 128, 16383, 16384, 2097151, 2097152, (1 << 28) - 1, 1 << 28]),
                                  [1, 1, 2, 2, 3, 3, 4, 4, 5])
