"""Device side: packed batch → HBM, workspace, the HIP stages, results → host.

PyTorch is used only as the device allocator / stream provider; all compute is
libs2c.so's hand-written HIP kernels (csrc/s2c_*.hip).  There is no CPU
fallback: without a visible GPU ``DeviceBatch`` raises.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch

from . import _lib as L
from ._lib import lib
from .devargs import (BUFFERS, UPLOAD, ZEROED, body_starts, device_index, empty_result, layout, needs_dense_layers,
                      padded_end, ref_stats, run_args, upload_arrays, workspace_plan)
from .table import DEL_KEY, TABLES


def _dev(device):
    """``device`` (devargs.device_index's forms, or a torch.device) as a torch.device."""
    if not torch.cuda.is_available():
        raise RuntimeError("sam2consensus_amd needs a ROCm GPU (torch.cuda unavailable); no CPU fallback")
    return torch.device("cuda", device_index(device))


def _up(arr, device):
    """numpy array → device tensor (bit-preserving, ≥ 16 bytes)."""
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.size == 0:
        a = np.zeros(max(4, 16 // a.itemsize), dtype=a.dtype)
    return torch.from_numpy(a).to(device, non_blocking=False)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()


class Uploader:
    """H2D of packed batches through pinned host staging: a ring of ``nbuf`` pinned buffers of
    ``chunk`` bytes and a copy stream.  ``upload(arrays)`` lays the arrays out in ONE device
    allocation and streams them through the ring: each chunk is packed into the next pinned
    buffer (after that buffer's previous copy has completed) and copied on the copy stream, so
    packing chunk k + 1 overlaps the DMA of chunk k; the compute stream waits on the last
    copy's event, and the host goes on (parsing the next batch) while the copies and the
    kernels run.  Pageable H2D of a GB-sized batch runs at ~2 GB/s on the box; this at the
    memcpy rate."""

    def __init__(self, device=None, nbuf=4, chunk=32 << 20):
        self.device = _dev(device)
        self.copy_stream = torch.cuda.Stream(self.device)
        self.chunk = int(chunk)
        self.slots = [None] * nbuf      # pinned uint8 tensors of `chunk` bytes
        self.events = [None] * nbuf     # the copy out of each slot
        self.k = 0
        self.timing = {"alloc": 0.0, "wait": 0.0, "pack": 0.0, "issue": 0.0}   # host seconds, cumulative

    def _slot(self):
        i = self.k % len(self.slots)
        self.k += 1
        t0 = time.perf_counter()
        if self.events[i] is not None:
            self.events[i].synchronize()          # this slot's previous copy has left it
        t1 = time.perf_counter()
        if self.slots[i] is None:
            self.slots[i] = torch.empty(self.chunk, dtype=torch.uint8, pin_memory=True)
        self.timing["wait"] += t1 - t0
        self.timing["alloc"] += time.perf_counter() - t1
        return i

    def prime(self):
        """Allocate the whole pinned ring now (the CLI does it on its warm-up thread while the
        host parses: 4 × 32 MB of page-locked memory is milliseconds of host time each)."""
        for i, s in enumerate(self.slots):
            if s is None:
                self.slots[i] = torch.empty(self.chunk, dtype=torch.uint8, pin_memory=True)
        return self

    def upload(self, arrays):
        """Flat uint8 arrays (devargs.upload_arrays) → device uint8 views (devargs.layout: each
        256-byte aligned, ≥ 16 bytes, zero-padded to its 16-byte end), in HBM once the compute
        stream reaches this point."""
        offs, total = layout([a.nbytes for a in arrays])
        compute = torch.cuda.current_stream(self.device)
        t0 = time.perf_counter()
        # the allocation on the copy stream (free there in its order: no wait for the compute
        # stream's queued kernels); the compute stream's use is recorded below
        with torch.cuda.stream(self.copy_stream):
            dev = torch.empty(total, dtype=torch.uint8, device=self.device)
        self.timing["alloc"] += time.perf_counter() - t0
        ends = [padded_end(o, a.nbytes) for a, o in zip(arrays, offs)]   # (zero pad to 16 bytes)
        ai = 0
        ev = None
        for w0 in range(0, max(ends) if ends else 0, self.chunk):
            w1 = min(w0 + self.chunk, total)
            i = self._slot()
            host = self.slots[i].numpy()
            t0 = time.perf_counter()
            while ai < len(arrays) and ends[ai] <= w0:
                ai += 1
            j = ai
            while j < len(arrays) and offs[j] < w1:   # the arrays (and their pads) in [w0, w1)
                a, o = arrays[j], offs[j]
                lo, hi = max(o, w0), min(ends[j], w1)
                n_data = max(0, min(o + a.nbytes, hi) - lo)
                if n_data >= (1 << 20):   # (large pieces on the host threads)
                    L.check(lib.s2c_copy_bytes(host.ctypes.data + (lo - w0), a.ctypes.data + (lo - o), n_data))
                elif n_data:
                    host[lo - w0:lo - w0 + n_data] = a[lo - o:lo - o + n_data]
                if lo + n_data < hi:
                    host[lo - w0 + n_data:hi - w0] = 0
                j += 1
            t1 = time.perf_counter()
            with torch.cuda.stream(self.copy_stream):
                dev[w0:w1].copy_(self.slots[i][:w1 - w0], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
            self.events[i] = ev
            self.timing["pack"] += t1 - t0
            self.timing["issue"] += time.perf_counter() - t1
        dev.record_stream(compute)   # (the kernels read it: not reused before they are done)
        if ev is not None:
            compute.wait_event(ev)
        return [dev[o:o + max(a.nbytes, 16)] for a, o in zip(arrays, offs)], dev


_UPLOADERS = {}
_SIDE = {}


def to_host(t):
    """A device uint8 tensor → the host, as a read-only memoryview of a pinned buffer (one DMA
    at the link's rate; no further copy: a 65 MB bytes object built from it would cost more
    than the transfer, its fresh pages faulted in by one thread).  The buffer comes from
    torch's caching host allocator and lives as long as the view; bytes-like everywhere
    (slicing, ``bytes +``, ``b"".join``, ``==``)."""
    n = int(t.numel())
    if n == 0:
        return memoryview(b"")
    if t.device.type != "cuda":
        return memoryview(t.contiguous().numpy()).toreadonly()
    buf = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    buf.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return memoryview(buf.numpy()).toreadonly()


def _side_stream(device):
    """A stream for result copies beside the compute stream (one per device)."""
    if device not in _SIDE:
        _SIDE[device] = torch.cuda.Stream(device)
    return _SIDE[device]


def default_uploader(device=None):
    """The process's Uploader for a device (its pinned ring allocated once)."""
    d = _dev(device)
    if d not in _UPLOADERS:
        _UPLOADERS[d] = Uploader(d)
    return _UPLOADERS[d]


class DeviceBatch:
    """The packed batch resident in HBM (inputs of every launch).  With an ``Uploader`` (by
    default for batches of 64 MB or more) the arrays go through its pinned staging ring and
    copy stream (asynchronous); otherwise each array is copied synchronously."""

    ARRAYS = UPLOAD   # (devargs: s2c_dev's pointer fields less dpc, and the dense windows' extension, in upload order)

    def __init__(self, hb, device=None, uploader=None, dense_layers=False):
        self.device = _dev(device) if uploader is None else uploader.device
        # dense_layers: the dense tiles' layered windows too (Workspace's counts-only modes run
        # them through k_tile); the pileup reads them in place, so by default they are not built
        self.hb = hb.ensure_layers(dense_layers)
        self.info = type(hb.info).from_buffer_copy(hb.info)   # (the arrays as uploaded)
        arrays = upload_arrays(hb)
        if uploader is None and sum(a.nbytes for a in arrays) >= (64 << 20):
            uploader = default_uploader(self.device)   # (large batches: pinned chunks, not pageable copies)
        if uploader is not None:
            views, self._storage = uploader.upload(arrays)
            for name, v in zip(self.ARRAYS, views):
                setattr(self, name, v)
            return
        for name, a in zip(self.ARRAYS, arrays):
            setattr(self, name, _up(a, self.device))

    def nbytes(self):
        return sum(getattr(self, n).numel() * getattr(self, n).element_size() for n in self.ARRAYS)


class Workspace:
    """All scratch + output buffers for one (batch, thresholds, fill, maxdel) configuration."""

    def __init__(self, db: DeviceBatch, thresholds, min_depth=1, fill=b"-", keep_counts=False,
                 maxdel_active=None, maxdel=None, counts=None, tile_range=None):
        dev = db.device
        i = db.info
        self.db = db
        # tile_range (t0, t1): launch only those tiles (their work items, dense and deep lists
        # filtered) and fetch only their results — a streamed batch's final tiles without
        # cutting a sub-batch
        self.tile_range = tile_range
        if needs_dense_layers(fill, keep_counts or counts is not None) and i.n_dense > 0 and not i.layers_dense:
            raise ValueError("counts-only modes and a fill of length != 1 run the dense tiles through k_tile: "
                             "DeviceBatch(..., dense_layers=True)")
        self.T = len(thresholds)
        fill = bytes(fill)
        self.fill_bytes = fill
        plan = workspace_plan(i, self.T, fill)
        self.sizes, self.fill_w, self.out_stride = plan.ws, plan.fill_w, plan.out_stride
        self.thr = torch.tensor([float(t) for t in thresholds], dtype=torch.float64, device=dev)
        self.fill = torch.tensor(list(fill) or [0], dtype=torch.uint8, device=dev)
        self.keep_counts = keep_counts
        self._counts_filled = False   # s2c_pileup_counts leaves counts filled: zeroed before a run
        self._tables_held = False     # the batch's insertion tables are in ibkt / ilong (accumulate(keep_tables=True))
        if counts is not None and counts.numel() * counts.element_size() < 6 * i.padded_len * 4:
            raise ValueError("counts buffer smaller than 6 x padded_len u32")
        for n in BUFFERS:   # one tensor per buffer, devargs.ZEROED zero before the first run
            size = plan.sizes[n]
            if n == "counts":
                # counts live in HBM only for deep / general tiles, unless a test asks for all of
                # them or streamed batches share their running totals (u8 view, 6·L u32)
                if counts is not None:
                    self.counts = counts
                    continue
                if keep_counts:
                    size = 6 * i.padded_len * 4
            setattr(self, n, (torch.zeros if n in ZEROED else torch.empty)(max(size, 16), dtype=torch.uint8, device=dev))
        bufs = {n: getattr(self, n).data_ptr() for n in BUFFERS}
        bufs.update(thresholds=self.thr.data_ptr(), fill=self.fill.data_ptr())
        self.dev, self.ext, self.lean = run_args(db.hb, i, {n: getattr(db, n).data_ptr() for n in UPLOAD}, bufs, self.T,
                                                 min_depth, fill, plan.out_cap, maxdel_active, maxdel)
        if tile_range is not None:   # the work lists and the dense windows' rows of [t0, t1) in place of the batch's
            t0, t1 = tile_range
            hb = db.hb
            keep = lambda a: a[(a[:, 0] >= t0) & (a[:, 0] < t1)] if len(a) else a  # noqa: E731
            win = (hb.dwin[:, 0] >= t0) & (hb.dwin[:, 0] < t1) if len(hb.dwin) else np.zeros(0, dtype=bool)
            sel = {"items": keep(hb.items), "dense": keep(hb.dense), "dwin": keep(hb.dwin),
                   "deep": hb.deep[(hb.deep >= t0) & (hb.deep < t1)], "dext": hb.dext[win], "drow": hb.drow[win]}
            self._sel = {name: _up(np.ascontiguousarray(a).reshape(-1), dev) for name, a in sel.items()}
            d = self.dev
            d.items, d.dense, d.dwin, d.deep = (_ptr(self._sel[n]) for n in ("items", "dense", "dwin", "deep"))
            d.n_items, d.n_dense, d.n_deep = len(sel["items"]), len(sel["dense"]), len(sel["deep"])
            self.ext.dext, self.lean.row = _ptr(self._sel["dext"]), _ptr(self._sel["drow"])
            self.ext.n_dext = self.lean.n_row = int(win.sum())

    def stream_handle(self):
        return C.c_void_p(torch.cuda.current_stream(self.db.device).cuda_stream)

    # ---- the stages in run order (each one C-ABI call; asynchronous on the current stream)
    def reads(self):
        """parsecigar + maxdel per piece → run records; insertion events → hash tables."""
        L.check(lib.s2c_reads(C.byref(self.dev), self.stream_handle()))

    def _counts_ready(self):
        if self._counts_filled:   # (after the counts-only diagnostic)
            self.counts.zero_()
            self._counts_filled = False

    def pileup(self):
        self._counts_ready()
        L.check(lib.s2c_pileup_lean(C.byref(self.dev), C.byref(self.ext), C.byref(self.lean), self.stream_handle()))

    def consensus(self):
        self._tables_held = False   # (k_consensus clears the deep tiles' insertion tables)
        L.check(lib.s2c_consensus(C.byref(self.dev), self.stream_handle()))

    def run(self):
        """reads → pileup (+ insertion columns, vote, FASTA bodies) → deep tiles (no host sync)."""
        self._counts_ready()
        self._tables_held = False
        L.check(lib.s2c_run_lean(C.byref(self.dev), C.byref(self.ext), C.byref(self.lean), self.stream_handle()))

    def record_done(self):
        """An event after this workspace's launches so far on the compute stream: ``fetch(done)``
        then waits for these kernels only, not for later batches queued behind them."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.db.device))
        return ev

    # ---- HIP graph of one run (the stage launches replayed without host launch overhead)
    def capture(self):
        """Capture one ``run()`` into a HIP graph (torch.cuda.CUDAGraph is hipGraph on ROCm);
        the kernel arguments (this workspace's buffers) are baked in."""
        dev = self.db.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.run()                      # warm-up launch outside the capture
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.run()
        self.graph = g
        return g

    def replay(self):
        self.graph.replay()

    # ---- results
    def accumulate(self, keep_tables=False):
        """Streamed batch of unsorted input: this batch's counts added to ``counts``."""
        self._tables_held = False
        L.check(lib.s2c_accumulate(C.byref(self.dev), 1 if keep_tables else 0, self.stream_handle()))
        self._tables_held = bool(keep_tables)

    def vote_all(self):
        """Last streamed batch of unsorted input: k_consensus votes every tile from ``counts``
        (after ``accumulate(keep_tables=True)``)."""
        nt = int(self.db.info.n_tiles)
        self._tables_held = False   # (k_consensus consumes and clears the insertion tables)
        if nt == 0:
            return
        self._all_tiles = torch.arange(nt, dtype=torch.int32, device=self.db.device)
        d = L.Dev.from_buffer_copy(self.dev)
        d.deep, d.n_deep = _ptr(self._all_tiles), nt
        L.check(lib.s2c_consensus(C.byref(d), self.stream_handle()))

    def _table_blocks(self):
        """Device int64 [n_tiles][3] {a, b, p0}: one block of the count table per tile (tiles
        never straddle a reference), p0 = a - ref_off[ref] + 1 the 1-based position of its
        first row; the tiles of a reference without coverage are empty blocks (no table is
        written for it, :334-341)."""
        if getattr(self, "_tblocks", None) is None:
            hb = self.db.hb
            tl = hb.tiles[:, :3].astype(np.int64)
            blocks = np.empty((len(tl), 3), dtype=np.int64)
            blocks[:, 0] = tl[:, 0]
            blocks[:, 1] = np.where(hb.ref_reads[tl[:, 2]] > 0, tl[:, 1], tl[:, 0])
            blocks[:, 2] = tl[:, 0] - hb.ref_off[tl[:, 2]] + 1
            self._tblocks = _up(blocks.reshape(-1), self.db.device)
        return self._tblocks

    def _two_pass(self, name, len_call, write_call, own_checks=None, filled_by="accumulate / pileup_counts"):
        """What the text tables share, for the method ``name``: its preconditions —
        keep_counts=True over the whole batch (every tile's counts in HBM) and counts a
        counts-only stage has filled —, then the method's ``own_checks()``, then on the current
        stream ``len_call(nt, blocks, lens, st)``, the launches that leave tile k's bytes in
        ``lens[k]`` (it allocates what the method needs besides; ``False`` from it: it launched
        nothing and every length is zero), the prefix sum, the one host
        read of the offsets, and ``write_call(nt, blocks, offs, text, total, st)``, the launch
        that formats tile k into text[offs[k], offs[k+1]) (``blocks``: ``_table_blocks``; all
        buffers as pointers).  Returns (offs[n_tiles + 1] int64 numpy, device uint8 tensor of
        exactly offs[-1] bytes); a batch without tiles gives the empty pair: no allocation, no
        launch."""
        if not self.keep_counts or self.tile_range is not None:
            raise ValueError(name + " needs Workspace(keep_counts=True) over the whole batch")
        if not self._counts_filled:
            raise ValueError(name + " needs filled counts (" + filled_by + "; s2c_consensus zeroes them)")
        if own_checks is not None:
            own_checks()
        dev = self.db.device
        nt = int(self.db.info.n_tiles)
        if nt == 0:
            return np.zeros(1, dtype=np.int64), torch.empty(0, dtype=torch.uint8, device=dev)
        st = self.stream_handle()
        blocks = _ptr(self._table_blocks())
        offs_d = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
        lens = torch.empty(nt, dtype=torch.int64, device=dev)
        if len_call(nt, blocks, _ptr(lens), st) is False:   # (it found nothing to format and left lens as it was)
            lens.zero_()
        torch.cumsum(lens, 0, out=offs_d[1:])
        offs = offs_d.cpu().numpy()
        total = int(offs[-1])
        text = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        write_call(nt, blocks, _ptr(offs_d), _ptr(text), total, st)
        return offs, text[:total]

    def _mask_words(self):
        """A bit per position of ``counts`` for a mark kernel (device int64, ≥ 1 word)."""
        return torch.empty(max((int(self.db.info.padded_len) + 63) // 64, 1), dtype=torch.int64, device=self.db.device)

    def counts_table(self):
        """The filled ``counts`` as the text of the count tables (table.py; s2c_table_len, the
        prefix sum, s2c_table_write on the current stream): (offs[n_tiles + 1] int64 numpy,
        device uint8 tensor of exactly offs[-1] bytes) — tile k's rows at [offs[k], offs[k+1]),
        a reference's table its tiles' rows in order.  Needs keep_counts=True (every tile's
        counts in HBM) and counts a counts-only stage has filled."""
        Lp = self.db.info.padded_len

        def len_call(nt, blocks, lens, st):
            L.check(lib.s2c_table_len(_ptr(self.counts), Lp, blocks, nt, lens, st))

        def write_call(nt, blocks, offs, text, total, st):
            L.check(lib.s2c_table_write(_ptr(self.counts), Lp, blocks, offs, nt, text, total, st))
        return self._two_pass("counts_table", len_call, write_call)

    def sites_table(self, min_cov=1, min_alt=2, min_frac=0.05):
        """The filled ``counts`` as the text of the tables of mixed sites (table.py;
        s2c_sites_mark into a bit per position, then s2c_sites_len, the prefix sum and
        s2c_sites_write over the set bits, on the current stream): the return shape and the
        preconditions of ``counts_table`` — tile k's site lines at [offs[k], offs[k+1])."""
        Lp, buf = self.db.info.padded_len, {}

        def len_call(nt, blocks, lens, st):
            buf["mask"] = self._site_mask(min_cov, min_alt, min_frac, st)
            L.check(lib.s2c_sites_len(_ptr(self.counts), Lp, _ptr(buf["mask"]), blocks, nt, lens, st))

        def write_call(nt, blocks, offs, text, total, st):
            L.check(lib.s2c_sites_write(_ptr(self.counts), Lp, _ptr(buf["mask"]), blocks, offs, nt, text, total, st))
        return self._two_pass("sites_table", len_call, write_call)

    def _site_mask(self, min_cov, min_alt, min_frac, st):
        """The mask s2c_sites_mark leaves for a rule.  Inside ``run_with_tables`` a rule is marked
        once: the site tables and the link tables of one rule share the mask."""
        rule = (int(min_cov), int(min_alt), float(min_frac))
        held = getattr(self, "_site_masks", None)
        if held is not None and rule in held:
            return held[rule]
        mask = self._mask_words()
        L.check(lib.s2c_sites_mark(_ptr(self.counts), self.db.info.padded_len, rule[0], rule[1], rule[2], _ptr(mask), st))
        if held is not None:
            held[rule] = mask
        return mask

    def links_table(self, min_cov=1, min_alt=2, min_frac=0.05, min_reads=1):
        """The allele pairs that fragments carry across neighbouring mixed sites as the text of
        the link tables (table.py; the sites of ``sites_table``'s rule, s2c_links_pop and the
        prefix sum for their ranks, s2c_links_count over every piece of the batch into ``pairs``
        — n_sites · 144 bytes, allocated and zeroed here on every call —, then s2c_links_len, the
        prefix sum and s2c_links_write, on the current stream): the return shape and the
        preconditions of ``counts_table`` — the lines of the pairs whose first site lies in tile
        k at [offs[k], offs[k+1]).  ``min_reads`` >= 1: the least reads of a listed pair.  One
        host read more than the other tables make: n_sites, four bytes, sizes ``pairs``."""
        db, i, buf = self.db, self.db.info, {}
        Lp = i.padded_len

        def own_checks():
            if not 1 <= int(min_reads) < 2 ** 32:
                raise ValueError("links_table: 1 <= min_reads < 2^32")

        def len_call(nt, blocks, lens, st):
            mask = buf["mask"] = self._site_mask(min_cov, min_alt, min_frac, st)
            nw = (int(Lp) + 63) // 64
            pop = torch.empty(max(nw, 1), dtype=torch.int32, device=db.device)
            rank = buf["rank"] = torch.zeros(nw + 1, dtype=torch.int32, device=db.device)
            L.check(lib.s2c_links_pop(_ptr(mask), Lp, _ptr(pop), st))
            torch.cumsum(pop[:nw], 0, dtype=torch.int32, out=rank[1:])
            ns = buf["n_sites"] = int(rank[-1].item()) & 0xFFFFFFFF
            pairs = buf["pairs"] = torch.zeros(max(144 * ns, 16), dtype=torch.uint8, device=db.device)
            d = self.dev
            L.check(lib.s2c_links_count(_ptr(db.pc), _ptr(db.ops), _ptr(db.bq), _ptr(db.bx), int(i.n_pieces), int(i.n_qwords),
                                        int(d.maxdel_active), int(d.maxdel), _ptr(mask), _ptr(rank), Lp, ns, _ptr(pairs), st))
            L.check(lib.s2c_links_len(_ptr(mask), _ptr(rank), Lp, _ptr(pairs), ns, blocks, _ptr(self._table_refs()), nt,
                                      int(min_reads), lens, st))

        def write_call(nt, blocks, offs, text, total, st):
            L.check(lib.s2c_links_write(_ptr(buf["mask"]), _ptr(buf["rank"]), Lp, _ptr(buf["pairs"]), buf["n_sites"], blocks,
                                        _ptr(self._table_refs()), offs, nt, int(min_reads), text, total, st))
        return self._two_pass("links_table", len_call, write_call, own_checks)

    def _table_refs(self):
        """Device int64 [n_tiles][2] {s, e}: the global range of the reference each tile lies in
        (``_table_blocks``' companion for the run tables)."""
        if getattr(self, "_trefs", None) is None:
            hb = self.db.hb
            ref = hb.tiles[:, 2].astype(np.int64)
            refs = np.empty((len(ref), 2), dtype=np.int64)
            refs[:, 0] = np.asarray(hb.ref_off, dtype=np.int64)[ref]
            refs[:, 1] = refs[:, 0] + np.asarray(hb.ref_len, dtype=np.int64)[ref]
            self._trefs = _up(refs.reshape(-1), self.db.device)
        return self._trefs

    def depth_table(self, cut=0, min_cov=1):
        """The filled ``counts`` as the text of the runs of equal coverage (table.py;
        s2c_runs_mark into a bit per run start, then s2c_runs_len, the prefix sum and
        s2c_runs_write, on the current stream).  ``cut`` = 0: the depth lines of every run;
        ``cut`` >= 1: the lines of the runs of coverage < cut (the low-coverage mask).  Returns
        (offs, device text, stats): the first two as ``counts_table``'s, with its preconditions
        — the lines of the runs that start in tile k at [offs[k], offs[k+1]); ``stats`` int64
        numpy [n_tiles][6] {runs, covered, passed, sumcov, mincov, maxcov} of those runs
        (``passed``: coverage >= min_cov), or None when cut >= 1."""
        Lp, buf = self.db.info.padded_len, {}

        def own_checks():
            if int(cut) < 0 or int(min_cov) < 0:
                raise ValueError("depth_table: cut >= 0 and min_cov >= 0")

        def len_call(nt, blocks, lens, st):
            c, refs, mask = _ptr(self.counts), _ptr(self._table_refs()), _ptr(buf.setdefault("mask", self._mask_words()))
            if not int(cut):
                buf["stats"] = torch.empty(nt * 6, dtype=torch.int64, device=self.db.device)
            L.check(lib.s2c_runs_mark(c, Lp, int(cut), mask, st))
            L.check(lib.s2c_runs_len(c, Lp, mask, blocks, refs, nt, int(cut), int(min_cov), lens, _ptr(buf.get("stats")), st))

        def write_call(nt, blocks, offs, text, total, st):
            L.check(lib.s2c_runs_write(_ptr(self.counts), Lp, _ptr(buf["mask"]), blocks, _ptr(self._table_refs()), offs, nt,
                                       int(cut), text, total, st))
        offs, text = self._two_pass("depth_table", len_call, write_call, own_checks)
        if int(cut):
            return offs, text, None
        stats = buf["stats"].cpu().numpy() if "stats" in buf else np.zeros(0, dtype=np.int64)
        return offs, text, stats.reshape(-1, 6)

    def insertions_table(self, min_reads=1):
        """The insertion events the batch keeps as the text of the insertion tables (table.py;
        s2c_ins_len, the prefix sum, s2c_ins_write on the current stream): the return shape of
        ``counts_table`` — tile k's lines at [offs[k], offs[k+1]).  Needs its preconditions and
        the insertion tables still held: between ``accumulate(keep_tables=True)`` and
        ``vote_all()``, which consumes them.  ``min_reads`` >= 1: the least reads of a listed
        motif, applied after equal long motifs are counted together."""
        db, i, buf = self.db, self.db.info, {}
        Lp, nq, n_bkt, n_lng = i.padded_len, int(i.n_qwords), int(i.n_bkt), int(i.n_lng)

        def own_checks():
            if not self._tables_held:
                raise ValueError("insertions_table needs the insertion tables: after accumulate(keep_tables=True), "
                                 "before vote_all()")
            if not 1 <= int(min_reads) < 2 ** 32:
                raise ValueError("insertions_table: 1 <= min_reads < 2^32")

        def len_call(nt, blocks, lens, st):
            buf["scratch"] = torch.empty(max(32 * (n_bkt + n_lng), 16), dtype=torch.uint8, device=db.device)   # (s2c.h: the size rule)
            L.check(lib.s2c_ins_len(_ptr(db.tiles), nt, _ptr(self.ibkt), n_bkt, _ptr(self.ilong), n_lng, _ptr(self.ilong_n),
                                    _ptr(db.bq), _ptr(db.bx), nq, _ptr(self.counts), Lp, blocks, int(min_reads),
                                    _ptr(buf["scratch"]), lens, st))

        def write_call(nt, blocks, offs, text, total, st):
            L.check(lib.s2c_ins_write(_ptr(db.tiles), nt, n_bkt, n_lng, _ptr(db.bq), _ptr(db.bx), nq, _ptr(self.counts), Lp,
                                      blocks, _ptr(buf["scratch"]), offs, text, total, st))
        return self._two_pass("insertions_table", len_call, write_call, own_checks, filled_by="accumulate")

    def _ref_names(self):
        """(device uint8 blob of the references' names, device int64 [n_refs][2] {offset, length},
        the blob's bytes): uploaded once per workspace for ``deletions_table``'s lines."""
        if getattr(self, "_names", None) is None:
            raw = [n.encode("latin-1") for n in self.db.hb.names]
            tab = np.zeros((max(len(raw), 1), 2), dtype=np.int64)
            tab[:len(raw), 1] = [len(n) for n in raw]
            tab[:len(raw), 0] = np.cumsum(tab[:len(raw), 1]) - tab[:len(raw), 1]
            blob = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
            self._names = (_up(blob, self.db.device), _up(tab.reshape(-1), self.db.device), int(blob.size))
        return self._names

    def deletions_table(self, min_reads=1):
        """The gap events the batch's pieces carry as the text of the deletion table (table.py;
        s2c_dels_count over every piece, the one 8-byte host read of the events' number E,
        s2c_dels_collect into a table of 2^k >= 2 E slots, s2c_dels_tiles, the prefix sum and
        s2c_dels_scatter into the tiles' parts of E entries, then s2c_dels_len, the prefix sum and
        s2c_dels_write, on the current stream; the table, two arrays of E entries and three words
        per tile are allocated here on every call, 64 to 96 bytes per event in all): the return shape
        and the preconditions of ``counts_table`` — the lines of the events that start in tile k
        at [offs[k], offs[k+1]), each with its reference's name, so the text is in file order.
        ``min_reads`` >= 1: the least fragments of a listed event.  Without an event nothing
        beyond the count is launched."""
        db, i, buf = self.db, self.db.info, {}
        Lp = i.padded_len

        def own_checks():
            if not 1 <= int(min_reads) < 2 ** 32:
                raise ValueError("deletions_table: 1 <= min_reads < 2^32")
            if int(i.word_lo) != 0:
                raise ValueError("deletions_table needs the whole batch's per-word arrays")

        def len_call(nt, blocks, lens, st):
            dev, d = db.device, self.dev
            i32 = lambda n: torch.zeros(max(int(n), 4), dtype=torch.int32, device=dev)  # noqa: E731
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            L.check(lib.s2c_dels_count(_ptr(db.pc), _ptr(db.ops), int(i.n_pieces), int(i.n_ops), Lp, _ptr(total), st))
            E = buf["E"] = int(total.item())
            if E == 0:
                return False
            if E >= 2 ** 32:
                raise L.S2CError(L.S2C_ERR_LIMIT, "more than 2^32 gap events")
            ns = 1 << max((2 * E - 1).bit_length(), 1)
            slots = torch.zeros(16 * ns, dtype=torch.uint8, device=dev)
            over = buf["over"] = i32(1)
            L.check(lib.s2c_dels_collect(_ptr(db.pc), _ptr(db.ops), _ptr(db.bq), _ptr(db.bx), int(i.n_pieces), int(i.n_ops),
                                         int(i.n_qwords), int(d.maxdel_active), int(d.maxdel), Lp, _ptr(slots), ns, _ptr(over), st))
            nw = int(i.word_hi)
            tcount, cursor, tn = i32(nt), i32(nt), i32(nt)
            tstart = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
            L.check(lib.s2c_dels_tiles(_ptr(slots), ns, _ptr(db.wtile), nw, nt, _ptr(tcount), st))
            torch.cumsum(tcount[:nt], 0, dtype=torch.int64, out=tstart[1:])
            ent = torch.empty(16 * E, dtype=torch.uint8, device=dev)
            tmp = torch.empty(16 * E, dtype=torch.uint8, device=dev)
            L.check(lib.s2c_dels_scatter(_ptr(slots), ns, _ptr(db.wtile), nw, nt, _ptr(tstart), _ptr(cursor), _ptr(ent), E, st))
            names, tab, nbytes = self._ref_names()
            buf["args"] = (_ptr(ent), E, _ptr(tstart), _ptr(tn), _ptr(db.tiles), nt, blocks, _ptr(names), nbytes, _ptr(tab),
                           int(i.n_refs), _ptr(self.counts), Lp)
            buf["keep"] = (ent, tmp, tstart, tn, slots)
            L.check(lib.s2c_dels_len(_ptr(ent), _ptr(tmp), E, _ptr(tstart), _ptr(db.tiles), nt, blocks, _ptr(names), nbytes, _ptr(tab),
                                     int(i.n_refs), _ptr(self.counts), Lp, int(min_reads), _ptr(tn), lens, st))

        def write_call(nt, blocks, offs, text, total, st):
            if not buf["E"]:
                return
            if int(buf["over"][0].item()):   # (only a table of too few slots fills)
                raise L.S2CError(L.S2C_ERR_LIMIT, "deletions_table: the event table overflowed")
            L.check(lib.s2c_dels_write(*buf["args"], offs, text, total, st))
        return self._two_pass("deletions_table", len_call, write_call, own_checks)

    def run_with_tables(self, request, deletions=None):
        """``run()`` through the counts route, with the tables of ``request`` (``table.request``'s
        mapping, a table's parameters those of its method): ``counts: ()``, ``variants: (min_cov,
        min_alt, min_frac)``, ``depth: (min_cov,)`` (``passed`` counted at min_cov), ``lowcov:
        (cut,)`` (the runs of coverage < cut), ``insertions: (min_reads,)``, ``links: (min_cov,
        min_alt, min_frac, min_reads)``.  Every tile's counts are stored (s2c_accumulate on zeroed
        counts, the insertion tables kept), formatted as text in ``TABLES`` order (before the vote,
        which leaves the counts zero and consumes the insertion tables), then every tile is voted
        from them (``vote_all``); ``fetch()`` yields the FASTA results as after ``run()``.  Returns
        {key: what the table's method returns} for exactly the keys of ``request``; a site rule
        that ``variants`` and ``links`` share is marked once.  ``deletions`` = min_reads (``True``:
        1) adds the per-run deletion table, which is no entry of ``TABLES``: ``deletions_table``'s
        pair under ``"deletions"``, formatted after the tables of ``request`` and before the vote."""
        if not self.keep_counts:
            raise ValueError("run_with_tables needs Workspace(keep_counts=True)")
        unknown = sorted(set(request) - {t.key for t in TABLES})
        if unknown:
            raise TypeError("no such table: " + ", ".join(unknown))
        if "lowcov" in request and int(request["lowcov"][0]) < 1:
            raise ValueError("run_with_tables: lowcov is the least coverage that passes, >= 1")
        make = {"counts": self.counts_table, "variants": self.sites_table, "depth": lambda min_cov: self.depth_table(0, min_cov),
                "lowcov": self.depth_table, "insertions": self.insertions_table, "links": self.links_table}
        self._counts_ready()
        # (set first: if a stage raises, a reused workspace zeroes its counts before its next run)
        self._counts_filled = True
        self.accumulate(keep_tables=True)
        self._site_masks = {}
        try:
            res = {t.key: make[t.key](*request[t.key]) for t in TABLES if t.key in request}
            if deletions is not None and deletions is not False:
                res[DEL_KEY] = self.deletions_table(1 if deletions is True else int(deletions))
        finally:
            self._site_masks = None
        self.vote_all()
        return res

    def run_with_counts(self):
        """``run_with_tables`` with the count tables alone.  Returns counts_table()'s (offs,
        device text)."""
        if not self.keep_counts:
            raise ValueError("run_with_counts needs Workspace(keep_counts=True)")
        return self.run_with_tables({"counts": ()})["counts"]

    def pileup_counts(self):
        """Diagnostic: k_reads, then every tile's counts stored to `counts` (no vote); needs
        keep_counts=True; returns counts[6][padded_len] as numpy u32."""
        if not self.keep_counts:
            raise ValueError("pileup_counts needs Workspace(keep_counts=True)")
        L.check(lib.s2c_pileup_counts(C.byref(self.dev), self.stream_handle()))
        self._counts_filled = True
        return self.counts_host()

    def counts_host(self):
        """counts[6][padded_len] as numpy u32 (for parity tests)."""
        Lp = self.db.info.padded_len
        return self.counts[: 6 * Lp * 4].view(torch.int32).cpu().numpy().view(np.uint32).reshape(6, Lp)

    def fetch(self, done=None):
        """Synchronise and copy results: (stats[R,T,4] u64, offs[T*nb+1] u64, out bytes).
        ``done`` (record_done): wait for that event only and copy on a side stream, so later
        batches' kernels on the compute stream neither delay nor are delayed by the copies.

        stats[r, t] = Σ over reference r's tiles of the device's per-tile statistics
        (tiles never straddle a reference; :352-397 sums)."""
        if done is None:
            torch.cuda.current_stream(self.db.device).synchronize()
            return self._fetch()
        side = _side_stream(self.db.device)
        side.wait_event(done)
        with torch.cuda.stream(side):
            return self._fetch()

    def _fetch(self):
        stats, offs, body = self.fetch_device()
        return stats, offs, to_host(body)

    def fetch_device(self):
        """Results with the FASTA bodies left on the device: (stats[R,T,4] u64, offs[T*nb+1]
        u64, body) — ``body`` a device uint8 tensor of exactly offs[-1] bytes, the fetched
        tiles' bodies compacted in [t][tile] order by ``s2c_gather_bodies_dev`` (only the
        statistics and the body lengths cross to the host here).  The current stream must
        have the kernels' results (``fetch`` arranges that).  stats: devargs.ref_stats."""
        i = self.db.info
        dev = self.db.device
        T, nb, tiles = self.T, i.n_tiles, self.db.hb.tiles
        t0, t1 = self.tile_range if self.tile_range is not None else (0, nb)
        nr = t1 - t0
        if T * nr == 0:
            return empty_result(i.n_refs, T) + (torch.empty(0, dtype=torch.uint8, device=dev),)
        ts = self.tile_stats[: T * nb * 32].view(torch.int64).cpu().numpy().view(np.uint64).reshape(T, nb, 4)
        stats = ref_stats(ts, tiles, i.n_refs, t0, t1)
        # each tile wrote its body into its slot; a reference's body is its tiles' pieces in
        # order: the slots (devargs.body_starts, uploaded once) compacted into [t][tile] order on the device
        lens = self.blk_len[: T * nb * 8].view(torch.int64).view(T, nb)[:, t0:t1].reshape(-1)
        offs_d = torch.zeros(T * nr + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offs_d[1:])
        offs = offs_d.cpu().numpy()
        total = int(offs[-1])
        body = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        if getattr(self, "_starts", None) is None:
            self._starts = _up(body_starts(tiles, T, self.fill_w, self.out_stride, t0, t1), dev)
        L.check(lib.s2c_gather_bodies_dev(_ptr(self.out), self.out.numel(), _ptr(self._starts), _ptr(offs_d),
                                          T * nr, _ptr(body), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return stats, offs.astype(np.uint64), body[:total]
