"""W ranks of acc_shard_reduce / acc_partial_deps_reduce in one process over the host transport, with every message
captured: the library hands the encoded bytes to the transport callback (Comm.host_fn), so a loopback (world 1) or an
in-memory all-to-all between one thread per rank (worlds 2 and 3) moves them and keeps a copy. Also the four comparisons
every case of test_fragwire_gpu.py makes (check_case):

  1. each captured message, decoded by the independent model (fragwire_model.py), equals the destination's slice of
     acc_shard_pack's streams for the sending store (the encoder alone);
  2. each rank's merged view equals the single-store KeyDeps of its home txns (decoder + merge);
  3. the form each header announces (slot list / bitmap / empty, u16 / u32 counts, u32 / u64 keys) equals the form the
     reference streams call for, so a case that misses the branch it was built for fails;
  4. the byte statistics equal the captured sizes and the reference streams' sizes.
"""
import threading

import numpy as np

import fragwire_model as M

MERGE_FIELDS = ("key_off", "key_code", "val_off", "txn_rank", "k2v_off", "k2v")
BARRIER_TIMEOUT = 60    # a safety cap: a rank that fails breaks the barrier at once, nobody waits this long
JOIN_TIMEOUT = 150


class Store:
    """One rank's input: its batch, the global index of each of its txns (None: the batch index)."""

    def __init__(self, batch, gidx=None):
        self.batch, self.gidx = batch, None if gidx is None else np.ascontiguousarray(gidx, dtype=np.uint32)


class Rank:
    """One rank: a Context, a host Comm whose exchange is `transport(send, send_bytes, recv_bytes) -> bytes | None`,
    and the record of every exchange it made: calls[i] = (send bytes, send_bytes, recv_bytes, received bytes | None)."""

    def __init__(self, world, rank, transport):
        import torch
        from accord_amd import sharded as S
        from accord_amd.deps import Context
        self.world, self.rank = world, rank
        self.dev = torch.device("cuda", 0)
        self.calls = []

        def fn(send, sb, rb):
            out = transport(send, sb, rb)
            self.calls.append((send.tobytes(), list(sb), list(rb), None if out is None else bytes(out)))
            return out

        self.ctx = Context(0)
        self.comm = S.Comm.host_fn(self.ctx, world, rank, fn)
        self._keep = None

    def close(self):
        self.comm.close()
        self.ctx.close()

    def load(self, store):
        """acc_keydeps_batch of the store's batch, then the explicit acc_shard_pack of it: per destination d the four
        reference streams (hdr u32, keys u64, vals u32, k2v i32)."""
        import torch
        from accord_amd import sharded as S
        bi, cols = S.batch_in_device(store.batch, self.dev)
        gdev = torch.from_numpy(store.gidx.astype(np.int32)).to(self.dev) if store.gidx is not None else None
        self._keep = (bi, cols, gdev)
        self.ctx.keydeps_batch_raw(bi)
        bufs, counts = S.shard_pack(self.ctx, bi, self.world, self.dev, gdev)
        host = dict(hdr=bufs["hdr"].cpu().numpy().view(np.uint32), keys=bufs["keys"].cpu().numpy().view(np.uint64),
                    vals=bufs["vals"].cpu().numpy().view(np.uint32), k2v=bufs["k2v"].cpu().numpy())
        ref = []
        for d in range(self.world):
            one = {}
            for q, (name, mult, _) in enumerate(S.STREAMS):
                off = np.concatenate([[0], np.cumsum(counts[q])]) * mult
                one[name] = host[name][int(off[d]):int(off[d + 1])].copy()
            ref.append(one)
        return ref

    def reduce(self, n_global):
        """acc_shard_reduce of the loaded batch; the merged view on the host. Forgets earlier exchanges."""
        from accord_amd import sharded as S
        bi, _, gdev = self._keep
        self.calls.clear()
        view = S.shard_reduce(self.ctx, self.comm, bi, n_global, gdev)
        return S.merged_to_host(self.ctx, view)

    def messages(self):
        """{dest: message bytes} of the last reduce: the first stream of each peer's block of the data exchange, its
        size taken from what this rank announced in the size exchange (one u64 per stream and peer)."""
        assert len(self.calls) == 2, f"a reduce makes a size and a data exchange, saw {len(self.calls)} calls"
        (sizes, sb0, _, _), (data, sb1, _, _) = self.calls
        ns = sb0[0] // 8
        announced = np.frombuffer(sizes, "<u8").reshape(self.world, ns)
        off = np.concatenate([[0], np.cumsum(sb1)])
        return {d: data[int(off[d]):int(off[d]) + int(announced[d, 0])] for d in range(self.world)}


def loopback(tamper=None):
    """World 1's transport: what is sent is what is received; tamper(call index, bytes) -> bytes | None may change it."""
    count = [0]

    def transport(send, sb, rb):
        i = count[0]
        count[0] += 1
        out = send.tobytes()
        return tamper(i, out) if tamper else out
    return transport


class Mailbox:
    """The in-memory all-to-all of W threads: deposit the per-destination slices, wait, take the per-source slices,
    wait again (so nobody deposits the next exchange over slices still being read)."""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=BARRIER_TIMEOUT)
        self.slots = {}

    def transport(self, rank):
        def fn(send, sb, rb):
            try:
                off = np.concatenate([[0], np.cumsum(sb)]).astype(np.int64)
                for d in range(self.world):
                    self.slots[(rank, d)] = send[off[d]:off[d + 1]].tobytes()
                self.barrier.wait()
                parts = [self.slots[(s, rank)] for s in range(self.world)]
                self.barrier.wait()
                if [len(p) for p in parts] != list(rb):
                    raise RuntimeError("received sizes differ from the announced ones")
                return b"".join(parts)
            except Exception:
                self.barrier.abort()    # every other rank's wait fails now: all end with ACC_E_STATE
                return None
        return fn


class Result:
    def __init__(self, world, n_global):
        self.world, self.n_global = world, n_global
        self.ref = [None] * world       # [store][dest] -> the four reference streams
        self.merged = [None] * world    # [rank] -> merged view on the host
        self.stats = [None] * world
        self.msg = {}                   # (source, dest) -> message bytes


def run_world(stores, n_global, reduce=None):
    """acc_shard_reduce over len(stores) ranks in this process. reduce(rank object, store) -> merged replaces the plain
    load + reduce (acc_partial_deps_reduce's case)."""
    world = len(stores)
    res = Result(world, n_global)

    def one(r, transport):
        rk = Rank(world, r, transport)
        try:
            if reduce is not None:
                res.ref[r], res.merged[r] = reduce(rk, stores[r])
            else:
                res.ref[r] = rk.load(stores[r])
                res.merged[r] = rk.reduce(n_global)
            res.stats[r] = rk.ctx.stats()
            for d, m in rk.messages().items():
                res.msg[(r, d)] = m
        finally:
            rk.close()

    if world == 1:
        one(0, loopback())
        return res
    box = Mailbox(world)
    errs = []

    def worker(r):
        try:
            one(r, box.transport(r))
        except BaseException as e:  # noqa: BLE001 - reported by the test thread
            box.barrier.abort()
            errs.append(f"rank {r}: {e!r}")

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=JOIN_TIMEOUT)
    assert not any(t.is_alive() for t in threads), "a rank thread did not finish"
    assert not errs, errs
    return res


# ---------------------------------------------------------------- references

def _gather(off, sel):
    """Indices of the CSR rows `sel`, concatenated; and the rows' lengths."""
    off = off.astype(np.int64)
    cnt = (off[1:] - off[:-1])[sel]
    start = np.concatenate([[0], np.cumsum(cnt)])
    idx = np.repeat(off[:-1][sel] - start[:-1], cnt) + np.arange(int(start[-1]), dtype=np.int64)
    return idx, cnt


def expected_home(full, b, gidx, n_global, rank, world):
    """sharded.home_result_from_full for a batch placed at global indices gidx among n_global txns (the other global
    txns have no keys, hence empty groups): the single-store KeyDeps `full` of every home txn of `rank`, TxnIds as
    global indices. With the identity placement and n_global = b.n_txn it is home_result_from_full itself (asserted by
    the dense case)."""
    g = np.arange(b.n_txn, dtype=np.int64) if gidx is None else gidx.astype(np.int64)
    sel = np.nonzero(g % world == rank)[0]
    slot = g[sel] // world
    ng = len(range(rank, n_global, world))
    out = {}
    ki, kc = _gather(full.kd_off, sel)
    vi, vc = _gather(full.u_off, sel)
    ai, ac = _gather(full.arena_off, sel)
    for name, cnt in (("key_off", kc), ("val_off", vc), ("k2v_off", ac)):
        per = np.zeros(ng, np.int64)
        per[slot] = cnt
        out[name] = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    owner = np.repeat(sel, kc)
    out["key_code"] = b.key_code[b.key_off.astype(np.int64)[owner] + full.key_idx[ki].astype(np.int64)].astype(np.uint64)
    out["txn_rank"] = g[full.dep_txn[vi].astype(np.int64)].astype(np.uint32)
    out["k2v"] = full.arena[ai].astype(np.int32)
    return out


def varint_bytes(x):
    """LEB128 length of each value: one byte per started group of 7 bits"""
    x = np.asarray(x, dtype=np.uint64)
    n = np.ones(len(x), np.int64)
    for k in range(1, 10):
        n += (x >> np.uint64(7 * k)) > 0
    return n


def ref_varint_lens(ref):
    """Per TxnId of one reference slice: the length of its varint (first: zigzag of the difference from t; others: the
    gap minus one), from the explicit streams alone."""
    hdr = ref["hdr"].reshape(-1, 4).astype(np.int64)
    v = ref["vals"].astype(np.int64)
    if len(v) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(hdr[:, 2])])[:-1]
    code = np.empty(len(v), np.int64)
    code[1:] = v[1:] - v[:-1] - 1
    delta = v[first] - hdr[:, 0]
    code[first] = np.where(delta < 0, -2 * delta - 1, 2 * delta)
    return varint_bytes(code), delta


def intended_form(ref, n_global, world):
    """The form fragwire.hip's rules give one (source, dest) slice of the reference streams: (slots, wide counts, wide
    keys) with slots in "bitmap" / "list" / "empty" (an empty message has no counts or keys: its flags say nothing)."""
    hdr = ref["hdr"].reshape(-1, 4).astype(np.int64)
    F = len(hdr)
    if F == 0:
        return ("empty", False, False)
    G = (max(n_global, 1) + world - 1) // world
    lens, _ = ref_varint_lens(ref)
    vb = np.add.reduceat(lens, np.concatenate([[0], np.cumsum(hdr[:, 2])])[:-1])
    wide_cnt = max(int(hdr[:, 1].max()), int(hdr[:, 2].max()), int(vb.max())) > 0xFFFF
    wide_key = int(ref["keys"].max()) - int(ref["keys"].min()) > 0xFFFFFFFF
    return ("list" if 4 * F < 4 * ((G + 31) // 32) else "bitmap", wide_cnt, wide_key)


def header_form(msg):
    h = M.parse_header(msg)
    if h.nfrag == 0:
        return ("empty", False, False)
    lst, wc, wk = h.form
    return ("list" if lst else "bitmap", wc, wk)


def check_case(res, expect, label=""):
    """The four comparisons. expect[rank] = the merged view that rank must hold. Returns what the case reached:
    {(source, dest): form}, the set of varint lengths, and the set of first-value signs."""
    world = res.world
    forms, lens, signs = {}, set(), set()
    for s in range(world):
        wire = raw = 0
        for d in range(world):
            msg, ref = res.msg[(s, d)], res.ref[s][d]
            # 1. model decode of the captured message == the explicit pack's slice
            got = M.decode(msg, world, d)
            for name in ("hdr", "keys", "vals", "k2v"):
                np.testing.assert_array_equal(getattr(got, name), ref[name], err_msg=f"{label} msg {s}->{d} {name}")
            rl, rd = ref_varint_lens(ref)
            np.testing.assert_array_equal(got.varint_len, rl, err_msg=f"{label} msg {s}->{d} varint lengths")
            np.testing.assert_array_equal(got.first_delta, rd, err_msg=f"{label} msg {s}->{d} first values")
            lens |= set(got.varint_len.tolist())
            signs |= set(np.sign(got.first_delta).tolist())
            # 3. the announced form == the intended one
            forms[(s, d)] = header_form(msg)
            assert forms[(s, d)] == intended_form(ref, res.n_global, world), (label, s, d, forms[(s, d)])
            # 4. the header's sections fill the message
            assert sum(got.header.sizes) == len(msg) - M.HEADER_BYTES, (label, s, d)
            assert got.header.G == (max(res.n_global, 1) + world - 1) // world, (label, s, d)
            wire += len(msg)
            raw += 4 * len(ref["hdr"]) + 8 * len(ref["keys"]) + 4 * len(ref["vals"]) + 4 * len(ref["k2v"])
        assert res.stats[s]["exchange.frag_wire_bytes"] == wire, (label, s)
        assert res.stats[s]["exchange.frag_raw_bytes"] == raw, (label, s)
    # 2. wire route == single-store KeyDeps of the home txns
    for r in range(world):
        for f in MERGE_FIELDS:
            np.testing.assert_array_equal(res.merged[r][f], expect[r][f], err_msg=f"{label} rank {r} {f}")
    return forms, lens, signs
