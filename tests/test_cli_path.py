"""hiprun.Session: the torch-free host path `sam2consensus.py -i ... -o ...` runs for a whole file
on one GPU.  It shares the kernels with engine.Workspace, and through devargs.py the run's layout:
the uploaded arrays, their 256-byte slots and 16-byte zero pads, the workspace's buffers, sizes and
zeroed set, the output capacity, the dense layers' rule, the argument blocks, the per-reference sum
of the statistics and the body slots' starts.  Its own are the buffers (one device allocation for
the batch, one for the workspace, a reused pinned buffer), the order of its copies, memsets, launch
and gather, and the result's view of the pinned buffer.  The shared functions are also pinned
directly (the tile ranges only the engine passes them included).

Without a GPU: Session against a recording stub of the HIP runtime.  Its allocations are host
memory filled with 0xA5, every call is logged with its thread, and an access to a freed block
fails; libs2c.so is the real one except s2c_run_lean, which checks what the kernels are handed
and writes results of its own choosing, and s2c_gather_bodies_dev, which copies as s2c.h says.
So the device each thread works on, the bytes and pads of every uploaded array, the workspace's
ranges and zeroed buffers, the fetch arithmetic, the buffers' lifetimes and their reuse are
checked exactly, on batches with insertion columns, a last tile ending mid-word and no tile at
all, under fills of length 1, 0, 2 and 65.

On the GPU: Session.run in place of Workspace.run + fetch on the cases the engine path is held
to, on one shared session, so each case also runs on buffers a differently shaped case left:
every golden case, the 300-threshold and long-skip goldens, test_gpu's pipeline parameter sets,
a deep-tile batch three times, test_dense_walk's and test_dense_ext's cases and the dense and
single stacks of test_counter_edges.  Every comparison is exact."""
import builtins
import ctypes as C
import hashlib
import os
import random
import tempfile
import threading

import numpy as np
import pytest

import batch_model as bm
import s2c_oracle as o
import test_counter_edges as tce
import test_dense_ext as tde
import test_dense_walk as tdw
import test_gpu as tg

from sam2consensus_amd import _lib as L
from sam2consensus_amd import batch, cli, configs, devargs, hiprun
from sam2consensus_amd.records import build_records, fasta_files

H2D, D2H = 1, 2   # hipMemcpyHostToDevice, hipMemcpyDeviceToHost
POISON = 0xA5


# ------------------------------------------------------------------ the stub runtime
class _Block:
    """One allocation of the stub: real host memory on a 256-byte boundary, poisoned; kept after
    its free, so no later allocation takes its addresses and a late access is recognised."""

    def __init__(self, kind, n, dev):
        self.raw = (C.c_uint8 * (n + 256))()
        C.memset(self.raw, POISON, n + 256)
        self.addr = (C.addressof(self.raw) + 255) // 256 * 256
        self.size, self.kind, self.dev, self.alive = n, kind, dev, True


class _World:
    """What the stub runtime and the library proxy share: the allocations, each thread's current
    device, the call log [(thread id, name, arguments)], and the run the test expects."""

    def __init__(self):
        self.blocks, self.log, self.current = [], [], {}
        self.expect = self.result = None

    def note(self, name, *args):
        self.log.append((threading.get_ident(), name, args))

    def device(self):
        return self.current.get(threading.get_ident(), 0)   # (HIP: device 0 until the thread sets one)

    def alloc(self, kind, n):
        b = _Block(kind, max(int(n), 1), self.device())
        self.blocks.append(b)
        return b

    def owner(self, addr):
        return next((b for b in self.blocks if b.addr <= addr < b.addr + b.size), None)

    def span(self, addr, n, kind):
        """The live block of ``kind`` that holds [addr, addr + n)."""
        addr, n = int(addr), int(n)
        b = self.owner(addr)
        assert b is not None, "address %#x lies in no allocation" % addr
        assert b.alive, "access to freed %s memory (%d bytes at +%d of a block of %d)" % (b.kind, n, addr - b.addr, b.size)
        assert b.kind == kind, "%s memory where %s memory belongs" % (b.kind, kind)
        assert addr + n <= b.addr + b.size, "%d bytes at +%d reach past a block of %d" % (n, addr - b.addr, b.size)
        return b

    def host(self, addr, n):
        """A host pointer of a copy: pinned memory of the stub (then live and in range) or the caller's own."""
        if self.owner(int(addr)) is not None:
            self.span(addr, n, "host")

    def view(self, addr, n, kind="dev"):
        if n == 0:
            return np.zeros(0, dtype=np.uint8)
        self.span(addr, n, kind)
        return np.ctypeslib.as_array((C.c_uint8 * int(n)).from_address(int(addr)))

    def release(self, addr, kind):
        b = self.owner(int(addr))
        assert b is not None and b.addr == addr and b.kind == kind and b.alive, "free of %#x: not a live %s allocation" % (addr, kind)
        b.alive = False

    def first(self, name, thread, start=0, args=None):
        """Index of ``thread``'s first call of ``name`` (with ``args``) at or after ``start``, or None."""
        return next((k for k in range(start, len(self.log)) if self.log[k][0] == thread and self.log[k][1] == name
                     and (args is None or self.log[k][2] == args)), None)

    # ---- the intercepted launch: what the kernels are handed, then results of our own
    def launch(self, d, x, y):
        e = self.expect
        sess, hb, thr, md, fill = e["sess"], e["hb"], e["thr"], e["md"], e["fill"]
        i, T = hb.info, len(thr)
        nb = int(i.n_tiles)
        batch_blk = self.span(sess.dbuf, 1, "dev")
        assert batch_blk.addr == sess.dbuf and batch_blk.size >= sess.dcap
        ptrs = {n: getattr(d, n) for n in devargs.ARRAYS}
        ptrs.update({n: getattr(x, n) for n in devargs.EXT_ARRAYS})
        ptrs.update(rop=y.rop, roff=y.roff, drow=y.row)
        assert ptrs["dpc"] is None                       # (read by no kernel: not uploaded)
        ranges = []
        for name in devargs.UPLOAD:
            a = np.ascontiguousarray(np.asarray(hb.device_view(name)).reshape(-1)).view(np.uint8)
            p = ptrs[name]
            if p is None:
                assert a.nbytes == 0, name
                continue
            assert p % 16 == 0, name
            padded = (a.nbytes + 15) // 16 * 16
            if padded == 0:
                continue
            assert self.span(p, padded, "dev") is batch_blk, name
            got = self.view(p, padded)
            assert (got[:a.nbytes] == a).all(), "%s: not the batch's bytes" % name
            assert not got[a.nbytes:].any(), "%s: its pad to 16 bytes is not zero" % name
            ranges.append((p, p + padded, name))
        assert (x.n_drun, x.n_dnev, x.n_dxs, x.n_drare, x.n_dext) == tuple(len(getattr(hb, n)) for n in devargs.EXT_ARRAYS)
        assert (y.n_rop, y.n_roff, y.n_row) == (len(hb.rop), len(hb.roff), len(hb.drow))
        # the workspace: every buffer with the size s2c_workspace_sizes gives, in one live allocation
        sz = L.WsSizes()
        L.check(L.lib.s2c_workspace_sizes(C.byref(i), T, C.byref(sz)))
        cap = int(sz.out_per_fill) * max(1, len(fill)) + int(sz.out_fixed)
        assert d.out_cap == cap
        size = {n: int(getattr(sz, n)) for n in devargs.BUFFERS if n != "out"}
        size.update(out=cap, thresholds=8 * T, fill=max(len(fill), 1))
        ws_blk = None
        for name, n in size.items():
            p = getattr(d, name)
            assert p is not None, name
            b = self.span(p, n, "dev")
            ws_blk = b if ws_blk is None else ws_blk
            assert b is ws_blk and b is not batch_blk, name
            ranges.append((p, p + n, name))
        ranges.sort()
        for (a0, a1, na), (b0, b1, nb_) in zip(ranges, ranges[1:]):
            assert a1 <= b0, "%s and %s overlap" % (na, nb_)
        assert self.view(d.thresholds, 8 * T).tobytes() == np.array([float(v) for v in thr], dtype=np.float64).tobytes()
        assert self.view(d.fill, len(fill)).tobytes() == fill
        for name in ("ibkt", "ilong_n", "counts"):       # (s2c_dev: zero before the first run)
            assert not self.view(getattr(d, name), size[name]).any(), "%s is not zero over its %d bytes" % (name, size[name])
        assert d.layers_built == 1 and d.layers_dense == i.layers_dense
        assert d.layers_dense == e.get("layers_dense", int(len(fill) != 1))
        assert (d.n_thr, d.min_depth, d.fill_len, d.n_tiles, d.n_cols, d.padded_len) == (T, md, len(fill), nb, i.n_cols, i.padded_len)
        # results: body lengths, statistics and bodies keyed by (threshold, tile), each body at the
        # slot s2c.h documents for s2c_dev.out: t·(F·padded_len + n_cols) + F·a + cb0
        F = max(1, len(fill))
        tiles = hb.tiles.astype(np.int64)
        stride = F * int(i.padded_len) + int(i.n_cols)
        base = F * tiles[:, 0] + tiles[:, 8]
        room = np.diff(np.append(base, stride))          # (up to the next tile's slot)
        assert (room >= 0).all() and T * stride <= cap
        tt, kk = np.meshgrid(np.arange(T, dtype=np.int64), np.arange(nb, dtype=np.int64), indexing="ij")
        lens = {"pattern": ((5 * tt + 3 * kk + 1) * 37) % (room[None, :] + 1), "full": room[None, :] + 0 * tt,
                "empty": 0 * tt}[e["mode"]]
        stats = (((tt * nb + kk)[:, :, None] * 4 + np.arange(4)) * 1000003 + 1 + (np.arange(4) << 33)).astype(np.uint64)
        self.view(d.blk_len, 8 * T * nb).view(np.int64)[:] = lens.reshape(-1)
        self.view(d.tile_stats, 32 * T * nb).view(np.uint64)[:] = stats.reshape(-1)
        out = self.view(d.out, cap)
        bodies = []
        for t in range(T):
            for k in range(nb):
                n = int(lens[t, k])
                bodies.append(((np.arange(n) * 7 + t * 131 + k * 17 + 1) % 251).astype(np.uint8))
                out[t * stride + base[k]:t * stride + base[k] + n] = bodies[-1]
        self.result = dict(lens=lens, stats=stats, body=b"".join(b.tobytes() for b in bodies), out=d.out, cap=cap,
                           blocks=(batch_blk, ws_blk), devices={self.device(), batch_blk.dev, ws_blk.dev}, at=len(self.log))
        return L.S2C_OK

    def gather(self, out, out_len, starts, offs, n, dst):
        """s2c_gather_bodies_dev as s2c.h declares it: dst[offs[i], offs[i+1]) = out[starts[i], + len)."""
        r = self.result
        assert (out, out_len) == (r["out"], r["cap"]) and n == r["lens"].size
        g = self.span(starts, 8 * n, "dev")
        assert g not in r["blocks"] and self.span(offs, 8 * (n + 1), "dev") is g
        s = self.view(starts, 8 * n).view(np.int64)
        f = self.view(offs, 8 * (n + 1)).view(np.int64)
        assert f[0] == 0 and (np.diff(f) >= 0).all()
        total = int(f[-1])
        if total:
            assert self.span(dst, total, "dev") is g
        src, to = self.view(out, out_len), self.view(dst, total)
        for k in range(n):
            ln = int(f[k + 1] - f[k])
            if 0 <= s[k] and s[k] + ln <= out_len:       # (a block reaching past out_len is skipped)
                to[f[k]:f[k + 1]] = src[s[k]:s[k] + ln]
        r["devices"] |= {self.device(), g.dev}
        return L.S2C_OK


class _StubHip:
    """hiprun.Hip's methods over the stub's memory."""

    def __init__(self, world):
        self.w = world

    def check(self, rc, what):
        assert rc == 0, what

    def set_device(self, dev):
        self.w.note("hipSetDevice", int(dev))
        self.w.current[threading.get_ident()] = int(dev)

    def cus(self, dev):
        return 256   # (s2c_plan_set_cus' default: the plans of this process stay as they are)

    def malloc(self, n):
        b = self.w.alloc("dev", n)
        self.w.note("hipMalloc", b.addr, int(n))
        return b.addr

    def host_malloc(self, n):
        b = self.w.alloc("host", n)
        self.w.note("hipHostMalloc", b.addr, int(n))
        return b.addr

    def memcpy(self, dst, src, n, kind):
        if not n:
            return
        self.w.note("hipMemcpy", dst, src, int(n), kind)
        assert kind in (H2D, D2H)
        self.w.span(dst if kind == H2D else src, n, "dev")
        self.w.host(src if kind == H2D else dst, n)
        C.memmove(dst, src, int(n))

    def memset(self, p, n):
        if not n:
            return
        self.w.note("hipMemset", p, int(n))
        self.w.span(p, n, "dev")
        C.memset(p, 0, int(n))

    def sync(self):
        self.w.note("hipDeviceSynchronize")

    def free(self, p):
        if p:
            self.w.note("hipFree", p)
            self.w.release(p, "dev")

    def host_free(self, p):
        if p:
            self.w.note("hipHostFree", p)
            self.w.release(p, "host")


class _Lib:
    """libs2c.so itself (s2c_workspace_sizes, s2c_plan_set_cus, ...: it loads without a GPU) but
    for the launch and the gather, and s2c_copy_bytes with its destination checked first."""

    def __init__(self, world):
        self._w = world

    def __getattr__(self, name):
        return getattr(L.lib, name)

    def s2c_copy_bytes(self, dst, src, n):
        self._w.span(dst, n, "host")
        return L.lib.s2c_copy_bytes(dst, src, n)

    def s2c_run_lean(self, d, x, y, stream):
        self._w.note("s2c_run_lean")
        assert stream.value is None                      # (the null stream)
        return self._w.launch(d._obj, x._obj, y._obj)

    def s2c_gather_bodies_dev(self, out, out_len, starts, offs, n, dst, stream):
        self._w.note("s2c_gather_bodies_dev", int(n))
        assert stream.value is None
        return self._w.gather(out.value, int(out_len), starts.value, offs.value, int(n), dst.value)


@pytest.fixture
def world(monkeypatch):
    w = _World()
    monkeypatch.setattr(hiprun, "Hip", lambda: _StubHip(w))
    monkeypatch.setattr(hiprun, "lib", _Lib(w))
    return w


# ------------------------------------------------------------------ the CPU tier's batches and options
THR3 = [0.25, 0.5, 0.75]
FILLS = [b"-", b"", b"XY", b"y" * 65]
FILL_IDS = ["dash", "empty", "XY", "y65"]


def _multi_sam():
    """Three references (one without a read), insertions on two of them: n_cols > 0, tiles whose
    first position and column slot base are not 0."""
    return ("@HD\tVN:1.0\n@SQ\tSN:g1\tLN:100\n@SQ\tSN:g2\tLN:70\n@SQ\tSN:g3\tLN:90\n"
            "r1\t0\tg1\t5\t60\t3M2I3M\t*\t0\t0\tAAACCGGG\t*\n"
            "r2\t0\tg1\t6\t60\t4M\t*\t0\t0\tAATG\t*\n"
            "r3\t0\tg3\t1\t60\t4M3I4M\t*\t0\t0\tAAAACGTCCCC\t*\n"
            "r4\t0\tg3\t1\t60\t2M2D4M\t*\t0\t0\tAACCCC\t*\n"
            "r5\t0\tg3\t40\t60\t8M\t*\t0\t0\tAAAACCCC\t*\n")


def _few_sam():
    return "@SQ\tSN:g\tLN:3000\n" + "".join("r%d\t0\tg\t%d\t60\t8M\t*\t0\t0\tACGTACGT\t*\n" % (k, p) for k, p in enumerate((1, 1500, 2990)))


SAMS = {
    "multi": _multi_sam,
    "midword": lambda: tdw.CASES["midword"][0](random.Random("midword")),   # (test_dense_walk._case's text)
    "nomap": lambda: "@HD\tVN:1.0\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n",
    "few": _few_sam,
}


def _batch(name):
    """A fresh batch (no layers built yet) of one of SAMS."""
    hb = batch.parse_text(SAMS[name](), True, 150)
    i = hb.info
    if name == "multi":
        assert i.n_cols > 0 and i.n_refs == 3 and i.n_tiles == 3 and (hb.tiles[1:, 0] > 0).all() and hb.tiles[:, 8].any()
    if name == "midword":
        assert i.n_dense > 0 and i.n_tiles > 1
    if name == "nomap":
        assert i.n_tiles == 0
    return hb


def _session(device=0, reserve=0):
    """A session brought up as the CLI does: reserve on cli._warm_session's side thread, joined."""
    sess = hiprun.Session(device)
    cli._join_session(sess, cli._warm_session(sess, reserve, {}))
    return sess


def _go(world, sess, hb, thr, md, fill, mode="pattern", **expect):
    world.expect = dict(sess=sess, hb=hb, thr=thr, md=md, fill=fill, mode=mode, **expect)
    world.result = None
    st, offs, body = sess.run(hb, thr, md, fill)
    return st, offs, bytes(body)


def _verify(world, sess, hb, thr, got):
    """Session.run's result == the per-reference sums, running offsets and concatenated bodies of
    what the intercepted run wrote; only the batch and staging buffers outlive the run."""
    st, offs, body = got
    r = world.result
    assert r is not None, "s2c_run_lean was not called"
    assert r["devices"] == {sess.device}, "devices of the launch's thread and buffers: %s, the session's: %d" % (sorted(r["devices"]), sess.device)
    T, nb, R = len(thr), int(hb.info.n_tiles), int(hb.info.n_refs)
    ref = hb.tiles[:, 2].astype(np.int64)
    want = np.zeros((R, T, 4), dtype=np.uint64)
    for k in range(R):
        want[k] = r["stats"][:, ref == k].sum(axis=1, dtype=np.uint64)
    assert st.dtype == np.uint64 and st.shape == want.shape and (st == want).all()
    want_offs = np.concatenate([[0], np.cumsum(r["lens"].reshape(-1))]).astype(np.uint64)
    assert offs.dtype == np.uint64 and offs.shape == want_offs.shape and (offs == want_offs).all()
    assert body == r["body"], tg._first_diff(body, r["body"])
    assert (world.first("s2c_gather_bodies_dev", threading.get_ident(), r["at"]) is not None) == (T * nb > 0)
    assert sorted(b.addr for b in world.blocks if b.alive) == sorted({sess.dbuf, sess.hbuf})


def _run(world, sess, hb, thr, md, fill, mode="pattern", **expect):
    got = _go(world, sess, hb, thr, md, fill, mode, **expect)
    _verify(world, sess, hb, thr, got)
    return got


# ------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("reserve", [0, 2 << 20], ids=["no_reservation", "reservation"])
def test_run_sets_the_device_on_the_calling_thread(world, reserve):
    """HIP's current device belongs to the thread: with the reservation made on the warm-up thread
    (device 2 set there, before its allocations), run() on the main thread sets device 2 before
    its first allocation, copy, memset and launch — with a reservation the batch buffer lives on
    device 2, and kernels launched on device 0 would read it from there."""
    sess = _session(2, reserve)
    main = threading.get_ident()
    assert world.first("hipSetDevice", main) is None
    warm = world.log[0][0]
    assert world.log[0][1:] == ("hipSetDevice", (2,)) and warm != main
    assert (world.first("hipMalloc", warm) is not None) == (reserve > 0)
    n0 = len(world.log)
    hb = _batch("multi")
    got = _go(world, sess, hb, THR3, 1, b"-")
    own = world.first("hipSetDevice", main, n0, (2,))
    for name in ("hipMalloc", "hipHostMalloc", "hipMemcpy", "hipMemset", "s2c_run_lean", "s2c_gather_bodies_dev"):
        k = world.first(name, main, n0)
        assert k is not None or (reserve and name == "hipHostMalloc"), name
        assert k is None or (own is not None and own < k), "the main thread's first %s comes before its hipSetDevice(2)" % name
    _verify(world, sess, hb, THR3, got)
    sess.close()


def test_fetch_sets_the_device_on_its_thread(world, monkeypatch):
    """_fetch on a thread of its own (where HIP starts at device 0): it sets the session's device
    before its first copy, allocation and the gather."""
    fetch, ids = hiprun.Session._fetch, []

    def on_a_thread(self, *args):
        box = {}

        def work():
            ids.append(threading.get_ident())
            try:
                box["res"] = fetch(self, *args)
            except BaseException as e:  # noqa: BLE001 - re-raised on the caller's thread
                box["err"] = e
        th = threading.Thread(target=work)
        th.start()
        th.join()
        if "err" in box:
            raise box["err"]
        return box["res"]
    monkeypatch.setattr(hiprun.Session, "_fetch", on_a_thread)
    sess = _session(2, 2 << 20)
    hb = _batch("multi")
    got = _go(world, sess, hb, THR3, 1, b"-")
    at = world.result["at"]
    own = world.first("hipSetDevice", ids[0], at, (2,))
    for name in ("hipMemcpy", "hipMalloc", "s2c_gather_bodies_dev"):
        k = world.first(name, ids[0], at)
        assert k is not None, name
        assert own is not None and own < k, "_fetch's first %s comes before its thread's hipSetDevice(2)" % name
    assert world.result["devices"] == {2}
    assert got[2] == world.result["body"]
    sess.close()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("name", ["multi", "midword", "nomap"])
def test_kernels_are_handed_the_packed_batch_and_a_zeroed_workspace(world, name, fill):
    """Inside the intercepted s2c_run_lean (_World.launch): every uploaded array 16-byte aligned
    inside the live batch allocation with the batch's bytes and a zero pad (the staging buffer was
    0xA5), dpc NULL, every workspace buffer with its s2c_workspace_sizes size inside one live
    allocation, out_cap = out_per_fill · max(1, len(fill)) + out_fixed, all ranges disjoint (the
    thresholds and the fill among them, one byte for the empty fill), ibkt, ilong_n and counts
    zero, the dense layers built exactly for a fill of length != 1."""
    sess = _session()
    hb = _batch(name)
    _run(world, sess, hb, THR3, 3, fill)
    assert hb.info.layers_dense == int(len(fill) != 1)
    sess.close()
    assert not [b for b in world.blocks if b.alive]


@pytest.mark.parametrize("mode", ["pattern", "full", "empty"])
def test_fetch_returns_reference_sums_running_offsets_and_slot_bytes(world, mode):
    """A fill of width 2 over insertion columns and three thresholds: the statistics summed per
    reference, the offsets, and each body read from t·(2·padded_len + n_cols) + 2·a + cb0 — also
    when every slot is full and when every body is empty; the body stays valid until close()."""
    sess = _session()
    hb = _batch("multi")
    st, offs, body = _run(world, sess, hb, THR3, 1, b"XY", mode)
    lens = world.result["lens"]
    assert lens.shape == (3, 3) and bool(lens.any()) == (mode != "empty")
    if mode == "empty":
        assert st.any() and not offs.any() and body == b""
    else:
        assert (lens[:, 1:] > 0).any() and len(body) == int(offs[-1]) > 0   # (bodies of tiles with a > 0)
    assert world.span(sess.hbuf, max(len(body), 1), "host").alive
    sess.close()
    assert not [b for b in world.blocks if b.alive]


def test_no_tile_gives_the_empty_result(world):
    sess = _session()
    hb = _batch("nomap")
    st, offs, body = _run(world, sess, hb, THR3, 1, b"XY")
    assert st.shape == (0, 3, 4) and offs.tolist() == [0] and body == b""
    sess.close()


def test_one_session_runs_a_large_a_small_and_the_large_batch_again(world):
    """The second and third runs pass every check of the launch and the fetch with the earlier
    run's bytes lying in the batch and staging buffers; the buffers only grow."""
    sess = _session()
    big, small = _batch("midword"), _batch("multi")
    assert sum(np.asarray(big.device_view(n)).nbytes for n in ("pc", "ops", "bq")) > \
        4 * sum(np.asarray(small.device_view(n)).nbytes for n in ("pc", "ops", "bq"))
    seen = []
    for hb, fill, mode in ((big, b"-", "full"), (small, b"XY", "pattern"), (big, b"-", "pattern")):
        _run(world, sess, hb, THR3, 1, fill, mode)
        seen.append((sess.dbuf, sess.dcap, sess.hbuf, sess.hcap))
    assert seen[0] == seen[1] == seen[2]                  # (the first run's buffers serve the later ones)
    few = _batch("few")
    _run(world, sess, few, [(k + 1) / 301.0 for k in range(300)], 1, b"-", "full")
    assert sess.dcap >= seen[0][1] and sess.hcap > seen[0][3]
    _run(world, sess, big, THR3, 1, b"-", "pattern")     # (and once more on the grown staging buffer)
    sess.close()


def test_fetch_grows_the_pinned_buffer_only(world):
    """300 thresholds over three reads: the bodies exceed the packed batch.  Between the launch and
    run()'s return the device batch buffer is neither freed nor re-allocated: only the pinned
    buffer grows."""
    sess = _session()
    hb = _batch("few")
    thr = [(k + 1) / 301.0 for k in range(300)]
    main = threading.get_ident()
    got = _go(world, sess, hb, thr, 1, b"-", "full")
    r = world.result
    dbuf, dcap = r["blocks"][0].addr, r["blocks"][0].size   # (the batch buffer the kernels were handed)
    assert len(got[2]) > dcap and len(got[2]) == 300 * int(hb.info.padded_len)
    after = world.log[r["at"]:]
    assert not [c for c in after if c[1] == "hipFree" and c[2][0] == dbuf], "the fetch freed the device batch buffer"
    assert (sess.dbuf, sess.dcap) == (dbuf, dcap), "the fetch re-allocated the device batch buffer"
    assert [c[1] for c in after if c[1] in ("hipMalloc", "hipFree")] == ["hipMalloc", "hipFree", "hipFree"]   # gather, gather, workspace
    assert world.first("hipHostMalloc", main, r["at"]) is not None and sess.hcap >= len(got[2])
    _verify(world, sess, hb, thr, got)
    sess.close()


# ------------------------------------------------------------------ the shared layout (devargs.py), directly
def test_body_starts_over_tile_ranges():
    """Three thresholds and a fill of width 2 on the batch with insertion columns: the whole range
    is t·(2·padded_len + n_cols) + 2·a + cb0 in [t][tile] order, a tile range its [t][tile] slice."""
    hb = _batch("multi")
    Lp, nc = int(hb.info.padded_len), int(hb.info.n_cols)
    a, cb0 = hb.tiles[:, 0].astype(np.int64), hb.tiles[:, 8].astype(np.int64)
    whole = devargs.body_starts(hb.tiles, 3, 2, 2 * Lp + nc, 0, 3)
    assert whole.dtype == np.int64 and whole.shape == (9,)
    assert whole.tolist() == [t * (2 * Lp + nc) + 2 * int(a[k]) + int(cb0[k]) for t in range(3) for k in range(3)]
    part = devargs.body_starts(hb.tiles, 3, 2, 2 * Lp + nc, 1, 3)
    assert part.dtype == np.int64 and part.tolist() == whole.reshape(3, 3)[:, 1:3].reshape(-1).tolist()
    none = devargs.body_starts(hb.tiles, 3, 2, 2 * Lp + nc, 1, 1)
    assert none.dtype == np.int64 and none.shape == (0,)


def test_ref_stats_over_tile_ranges():
    """Random u64 statistics: each range's sums equal a plain double loop over its tiles (modulo
    2^64), a reference without a tile in the range stays zero, and two ranges add up to their union."""
    hb = _batch("multi")
    R, nb, T = int(hb.info.n_refs), int(hb.info.n_tiles), 3
    ts = np.random.default_rng(5).integers(0, 2 ** 64, size=(T, nb, 4), dtype=np.uint64)
    got = {}
    for t0, t1 in ((0, 1), (1, 3), (0, 3)):
        st = got[t0, t1] = devargs.ref_stats(ts, hb.tiles, R, t0, t1)
        assert st.dtype == np.uint64 and st.shape == (R, T, 4)
        want = [[[0] * 4 for _ in range(T)] for _ in range(R)]
        for t in range(T):
            for k in range(t0, t1):
                for j in range(4):
                    r = int(hb.tiles[k, 2])
                    want[r][t][j] = (want[r][t][j] + int(ts[t, k, j])) % 2 ** 64
        assert st.tolist() == want
        for r in set(range(R)) - {int(v) for v in hb.tiles[t0:t1, 2]}:
            assert not st[r].any()
    assert ((got[0, 1] + got[1, 3]) == got[0, 3]).all() and got[0, 3].any()


def test_layout_slots_and_pads():
    """256-byte slots that hold each buffer up to its 16-byte pad end (at least 16 bytes), disjoint."""
    sizes = [0, 1, 16, 17, 255, 256, 257]
    offs, total = devargs.layout(sizes)
    assert len(offs) == len(sizes) and devargs.ALIGN == 256
    ends = [devargs.padded_end(o, n) for o, n in zip(offs, sizes)]
    for o, n, e, nxt in zip(offs, sizes, ends, offs[1:] + [total]):
        assert o % 256 == 0 and e - o == (max(n, 16) + 15) // 16 * 16 and e <= nxt
    assert devargs.layout([]) == ([], 256)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_workspace_plan_sizes(fill):
    """Every buffer's size is its s2c_workspace_sizes field, but out = out_per_fill · max(1, len(fill))
    + out_fixed; the thresholds take 8 bytes each, the fill at least one byte."""
    hb = _batch("multi")
    i, T, F = hb.info, 3, max(1, len(fill))
    sz = L.WsSizes()
    L.check(L.lib.s2c_workspace_sizes(C.byref(i), T, C.byref(sz)))
    plan = devargs.workspace_plan(i, T, fill)
    cap = int(sz.out_per_fill) * F + int(sz.out_fixed)
    want = {n: int(getattr(sz, n)) for n in devargs.BUFFERS if n != "out"}
    want.update(out=cap, thresholds=8 * T, fill=max(len(fill), 1))
    assert plan.sizes == want
    assert (plan.fill_w, plan.out_cap, plan.out_stride) == (F, cap, F * int(i.padded_len) + int(i.n_cols))
    assert set(devargs.ZEROED) == {"ibkt", "ilong_n", "counts"} and set(devargs.ZEROED) < set(devargs.BUFFERS)


def test_device_index_forms(monkeypatch):
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    assert devargs.device_index(None) == 0
    monkeypatch.setenv("LOCAL_RANK", "3")
    assert devargs.device_index(None) == 3
    assert [devargs.device_index(d) for d in (2, "cuda", "cuda:5")] == [2, 0, 5]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        devargs.device_index("cpu")
    assert hiprun.device_index is devargs.device_index


# ------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def sess():
    """One session for every GPU test below: each case runs on the buffers the earlier ones left."""
    s = hiprun.Session(0).reserve()
    yield s
    s.close()


def _same(got, want):
    st, offs, out = got
    assert st.shape == want[0].shape and (st == want[0]).all()
    assert offs.shape == want[1].shape and (offs == want[1]).all()
    assert out == want[2], tg._first_diff(out, want[2])


def _srun(sess, hb, thr, md, fill):
    st, offs, out = sess.run(hb, thr, md, fill)
    return st, offs, bytes(out)   # (the view is the session's staging buffer: the next run overwrites it)


_PARSER = cli.build_parser()


def _session_text(sess, sam, argv):
    """cli.run_text with Session.run in place of consensus_batch: (status, {file name: text})."""
    args = _PARSER.parse_args(["-i", "in.sam"] + list(argv))
    try:
        thr = [float(v) for v in args.thresholds.split(",")]
        hb = batch.parse_text(sam, not isinstance(args.maxdel, str), 150)
        try:
            st, offs, out = sess.run(hb, thr, args.min_depth, os.fsencode(args.fill))
            files = fasta_files(hb, thr, os.fsencode(args.prefix or "in"), args.n, st, offs, out)
        finally:
            hb.free()
    except cli.REF_ERRORS as e:
        return type(e).__name__, {}
    return "ok", {k.decode("latin-1"): v.decode("latin-1") for k, v in files.items()}


# measured on an MI355X: all 1,532 cases take 0.8 s on the shared session (0.16-0.31 s per slice), so
# the slices are for naming where a failure lies, not for time
GOLDEN_SLICES = 4
_BOUNDS = [len(tg.CASES) * k // GOLDEN_SLICES for k in range(GOLDEN_SLICES + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(GOLDEN_SLICES))
def test_session_matches_reference_on_every_golden_case(sess, k):
    """All KAT and fuzz cases (the reference's own status and files), in contiguous slices."""
    assert _BOUNDS[0] == 0 and _BOUNDS[-1] == len(tg.CASES) == 1532
    for case in tg.CASES[_BOUNDS[k]:_BOUNDS[k + 1]]:
        status, files = _session_text(sess, case["sam"], case["args"])
        assert status == case["status"], case["name"]
        assert files == case["files"], (case["name"], sorted(files))


@pytest.mark.gpu
@pytest.mark.parametrize("gold,idx", [("limits", 0), ("limits", 1), ("longskip", 0), ("longskip", 1)])
def test_session_matches_reference_on_many_thresholds_and_long_skips(sess, gold, idx):
    """300 thresholds (bodies larger than the batch: the fetch grows the pinned buffer) and a
    16.7 Mb skip: sha256 per file against the golden."""
    import golden_io
    c = golden_io.load(gold)[idx]
    status, files = _session_text(sess, c["sam"], c["args"])
    assert status == c["status"]
    got = {k: hashlib.sha256(v.encode("latin-1")).hexdigest() for k, v in files.items()}
    assert got == {k: v["sha256"] for k, v in c["files"].items()}


def _check_records(hb, thr, got, ref):
    """The files of a result == the oracle's, or its exception class."""
    if ref["status"] != "ok":
        with pytest.raises(getattr(builtins, ref["status"])):
            build_records(hb, thr, "case", *got)
        return
    from sam2consensus_amd.records import render
    recs = build_records(hb, thr, "case", *got)
    assert {n + "__case.fasta": render(r, 0).decode("latin-1") for n, r in recs.items()} == ref["files"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,over,thr,md,fill", tg.PIPELINE_CASES)
def test_session_pipeline_equals_batch_model(sess, name, over, thr, md, fill):
    """test_gpu.test_device_pipeline_equals_batch_model's parameter sets and path assertions."""
    hb = configs.synth_batch(name, **over)
    if over.get("ins_max") == 60:
        assert (hb.tiles[:, 3] & 2 == 2).any(), "case must exercise general (k_consensus) tiles"
        assert int(hb.tiles[:, 9].max()) > 1024, "case must exercise long motifs and many columns"
    if over.get("depth") == 9000.0:
        assert hb.info.n_deep > 0 and hb.info.n_ins > 0
    want = bm.model_pipeline(hb, thr, md, fill)
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "case.sam")
        configs.synth_write(name, p, **over)
        text = open(p, "rb").read().decode("latin-1")
    args = ["--consensus-thresholds=" + ",".join(repr(t) for t in thr), "-m", str(md), "--fill=" + fill.decode("latin-1")]
    ref = o.run_case(text, args, name="case.sam")
    for _ in range(2):
        got = _srun(sess, hb, thr, md, fill)
        _same(got, want)
    _check_records(hb, thr, got, ref)
    hb.free()


@pytest.mark.gpu
def test_session_zeroes_the_deep_tiles_counts_on_every_run(sess, monkeypatch):
    """Deep tiles add into the HBM counts, which Session zeroes itself in each run's fresh
    workspace: three runs on the shared session == the batch model.  A fresh device allocation is
    often zero already, and a reused one holds the counts the last run left zero, so here every
    allocation of the runs is filled with 0xA5 before Session gets it: what it must zero (ibkt,
    ilong_n, counts) it has to zero itself, as in the stub's memory without a GPU."""
    real = sess.hip.malloc

    def poisoned(n):
        p = real(n)
        junk = np.full(int(n), POISON, dtype=np.uint8)   # (n: at most the allocation's size)
        sess.hip.memcpy(p, junk.ctypes.data, junk.nbytes, H2D)
        return p
    monkeypatch.setattr(sess.hip, "malloc", poisoned)
    hb = configs.synth_batch("c4", ref_len=2000, depth=12000.0)
    assert hb.info.n_deep > 0, "the deep-tile path must run"
    want = bm.model_pipeline(hb, THR3, 1, b"-")
    for _ in range(3):
        _same(_srun(sess, hb, THR3, 1, b"-"), want)
    hb.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tde.CASES))
def test_session_dense_walk_equals_batch_model_and_oracle(sess, name):
    """test_dense_walk.CASES and test_dense_ext's n_events."""
    _, opt, hb, want, ref = tde._case(name)
    got = _srun(sess, hb, opt.thresholds, opt.min_depth, opt.fill.encode())
    _same(got, want)
    assert tdw._files(hb, opt, *got) == ref["files"]


EDGE_RUNS = [(n, list(tce.CASES[n][1])) for n in ("dense255", "dense255_lookback", "dense255_long", "dense_twodec", "single_twodec")] + \
    [(n, ["m1", "m256", "m255empty"]) for n in ("single256", "single255_ins")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,arg_sets", EDGE_RUNS, ids=[n for n, _ in EDGE_RUNS])
def test_session_counter_edges_equal_model_and_oracle(sess, name, arg_sets):
    """The last dense depth and the first past it under every argument set (empty fills, -f N,
    thresholds outside (0, 1]): the fills of length 0 and 1 alternate on one batch."""
    s, sam, hb = tce._built(name)
    tce._check_path(s, hb)
    for args_name in arg_sets:
        opt, want, ref = tce._expect(name, args_name)
        got = _srun(sess, hb, opt.thresholds, opt.min_depth, opt.fill.encode())
        _same(got, want)
        tce._check_files(hb, opt, *got, ref)
