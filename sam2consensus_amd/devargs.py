"""The host-side layout of one run, shared by the torch-backed engine (engine.Workspace, Uploader)
and the torch-free whole-file CLI path (hiprun.Session): which arrays a batch uploads and where
each lies in an upload, the workspace's buffers and their sizes, the argument blocks ``s2c_dev`` /
``s2c_dense_ext`` / ``s2c_dense_lean`` (include/s2c.h), the fetch arithmetic and the device a run
names.  No torch here, and no device call: allocations, copies, launches and their order stay
with the two callers."""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

from . import _lib as L

# the packed batch's device arrays, in upload order (s2c_dev's pointer fields)
ARRAYS = ("pc", "ops", "bq", "bx", "rs", "tiles", "items", "dense", "deep", "lp", "wtile", "rlist", "ps",
          "lly", "lpc", "lops", "lbq", "lbx", "px", "dwin", "lpx", "dpc")
# the dense windows' extension (s2c_dense_ext), what k_tile_dense walks from.  dpc, the host's
# compact records it is written from, is read by no kernel and is not uploaded (UPLOAD: what a
# run uploads; s2c_dev.dpc stays NULL)
EXT_ARRAYS = ("drun", "dnev", "dxs", "drare", "dext")
# ... and its lean part (s2c_dense_lean: the rare pieces' op words, their offsets, the windows' rows)
LEAN_ARRAYS = ("rop", "roff", "drow")
UPLOAD = tuple(n for n in ARRAYS if n != "dpc") + EXT_ARRAYS + LEAN_ARRAYS
# the workspace buffers a run writes (s2c_workspace_sizes), plus the thresholds and fill
BUFFERS = ("runs", "ibkt", "ilong", "ilong_n", "counts", "ins_cols", "ins_chr", "blk_len", "tile_stats", "out")
# ... those a caller zeroes before the first run (s2c_dev: the insertion tables and the counts;
# every run leaves them zero)
ZEROED = ("ibkt", "ilong_n", "counts")
ALIGN = 256


def device_index(device=None):
    """The device of a run as an index: ``None`` (LOCAL_RANK, else 0), N, ``cuda`` or ``cuda:N``
    (a torch.device's text too)."""
    if device is None:
        return int(os.environ.get("LOCAL_RANK", "0"))
    if isinstance(device, int):
        return device
    s = str(device)
    if s.startswith("cuda"):
        return int(s.split(":")[1]) if ":" in s else 0
    raise RuntimeError("sam2consensus_amd needs a ROCm GPU device, not %r; no CPU fallback" % (device,))


def needs_dense_layers(fill=b"-", counts=False):
    """Whether a run takes the dense tiles through k_tile (so its batch needs its dense layers
    built): the counts-only modes, and a fill of length != 1 (k_tile_dense emits one char per
    position)."""
    return bool(counts) or len(fill.encode("latin-1") if isinstance(fill, str) else bytes(fill)) != 1


def upload_arrays(hb):
    """The batch's UPLOAD arrays as flat contiguous uint8 views, in order (the per-word arrays
    over the batch's word span only: HostBatch.device_view)."""
    return [np.ascontiguousarray(np.asarray(hb.device_view(n)).reshape(-1)).view(np.uint8) for n in UPLOAD]


def layout(sizes):
    """(offs, total) of buffers of ``sizes`` bytes in one allocation: ALIGN-byte slots of at
    least 16 bytes each, total >= ALIGN."""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (max(int(n), 16) + ALIGN - 1) // ALIGN * ALIGN
    return offs, max(total, ALIGN)


def padded_end(off, n):
    """The end of the zero pad behind ``n`` bytes at ``off``: the kernels read a buffer up to its
    end rounded to 16 bytes."""
    return off + (max(int(n), 16) + 15) // 16 * 16


# sizes: name → bytes of each of BUFFERS (out: out_cap), ``thresholds`` and ``fill``; fill_w: the
# bytes a position takes in a body; out_stride: a threshold's share of ``out``; ws: the s2c_ws_sizes
WorkspacePlan = collections.namedtuple("WorkspacePlan", "sizes fill_w out_cap out_stride ws")


def workspace_plan(info, n_thr, fill):
    """The workspace of a run of ``n_thr`` thresholds and ``fill`` over a batch of ``info``."""
    ws = L.WsSizes()
    L.check(L.lib.s2c_workspace_sizes(C.byref(info), int(n_thr), C.byref(ws)))
    # body slots: per threshold max(1, len(fill)) bytes per padded position + the columns
    fill_w = max(1, len(fill))
    out_cap = int(ws.out_per_fill) * fill_w + int(ws.out_fixed)
    sizes = {n: out_cap if n == "out" else int(getattr(ws, n)) for n in BUFFERS}
    sizes.update(thresholds=8 * int(n_thr), fill=fill_w)
    return WorkspacePlan(sizes, fill_w, out_cap, fill_w * info.padded_len + info.n_cols, ws)


def fill_dev(info, arrays, bufs, n_thr, min_depth, fill, maxdel_active, maxdel, out_cap):
    """``arrays``: name → device address of each of ARRAYS; ``bufs``: name → device address of
    each of BUFFERS and of ``thresholds`` (n_thr f64) and ``fill`` (its bytes)."""
    i = info
    d = L.Dev()
    for name in ARRAYS:
        setattr(d, name, arrays.get(name))   # (dpc: None, i.e. NULL — no longer read)
    d.n_pieces, d.n_ops, d.n_qwords, d.n_tiles = i.n_pieces, i.n_ops, i.n_qwords, i.n_tiles
    d.n_items, d.n_dense, d.n_deep = i.n_items, i.n_dense, i.n_deep
    d.padded_len, d.chunk, d.kwin, d.tile_max = i.padded_len, i.chunk, i.kwin, i.tile_max
    d.dense_lds = i.dense_lds
    d.n_rlist = i.n_rlist
    d.n_layers, d.n_lpieces, d.n_lops, d.n_lqwords = i.n_layers, i.n_lpieces, i.n_lops, i.n_lqwords
    d.layers_dense, d.layers_built = i.layers_dense, i.layers_built
    d.word_lo, d.word_hi = i.word_lo, i.word_hi
    d.walk_queue, d.tile_events, d.n_rlist_run = i.walk_queue, i.tile_events, i.n_rlist_run
    d.maxdel_active, d.maxdel = 1 if maxdel_active else 0, int(maxdel)
    d.thresholds, d.n_thr = bufs["thresholds"], int(n_thr)
    d.min_depth = int(max(min(min_depth, 2**31 - 1), -2**31))
    fill = bytes(fill)
    d.fill_len, d.fill_nondash = len(fill), sum(1 for c in fill if c != ord("-"))
    d.fill = bufs["fill"]
    for name in BUFFERS:
        setattr(d, name, bufs[name])
    d.n_cols = i.n_cols
    d.out_cap = int(out_cap)
    return d


def fill_ext(hb, arrays):
    """The ``s2c_dense_ext`` of a run: ``arrays``: name → device address of each of EXT_ARRAYS
    (the batch ``hb``'s, whole)."""
    x = L.DenseExt()
    for name in EXT_ARRAYS:
        setattr(x, name, arrays[name])
    x.n_drun, x.n_dnev, x.n_dxs, x.n_drare, x.n_dext = (len(getattr(hb, n)) for n in EXT_ARRAYS)
    return x


def fill_lean(hb, arrays):
    """The ``s2c_dense_lean`` beside it: ``arrays``: name → device address of each of LEAN_ARRAYS
    (the scalars are the whole batch's: they hold for any subset of its windows)."""
    y = L.DenseLean()
    y.rop, y.roff, y.row = arrays["rop"], arrays["roff"], arrays["drow"]
    y.n_rop, y.n_roff, y.n_row = len(hb.rop), len(hb.roff), len(hb.drow)
    y.lds, y.count_max, y.pairs = hb.lean_lds, hb.lean_count, hb.lean_pairs
    return y


def run_args(hb, info, arrays, bufs, n_thr, min_depth, fill, out_cap, maxdel_active=None, maxdel=None):
    """(s2c_dev, s2c_dense_ext, s2c_dense_lean) of one run over the whole batch: ``arrays``: name →
    device address of each of UPLOAD, ``bufs`` as ``fill_dev``'s.  The maxdel rule (:210) runs
    on the device: the parser's setting unless overridden."""
    if maxdel_active is None:
        maxdel_active = getattr(hb, "maxdel_active", True)
    if maxdel is None:
        maxdel = getattr(hb, "maxdel", 150)
    return (fill_dev(info, arrays, bufs, n_thr, min_depth, fill, maxdel_active, maxdel, out_cap),
            fill_ext(hb, arrays), fill_lean(hb, arrays))


def empty_result(n_refs, n_thr):
    """(stats, offs) of a fetch without a (threshold, tile) block."""
    return np.zeros((n_refs, n_thr, 4), dtype=np.uint64), np.zeros(1, dtype=np.uint64)


def ref_stats(ts, tiles, n_refs, t0, t1):
    """stats[R, T, 4] u64: stats[r, t] = Σ over reference r's tiles in [t0, t1) of the device's
    per-tile statistics ``ts[T, n_tiles, 4]`` u64 (tiles never straddle a reference; :352-397 sums)."""
    stats = empty_result(n_refs, ts.shape[0])[0]
    ref = tiles[t0:t1, 2].astype(np.int64)
    for t in range(ts.shape[0]):
        np.add.at(stats[:, t, :], ref, ts[t, t0:t1])
    return stats


def body_starts(tiles, n_thr, fill_w, out_stride, t0, t1):
    """int64 [T·(t1 − t0)]: the slot in ``out`` of each (threshold, tile) body of tiles [t0, t1),
    t·out_stride + F·a + cb0 (s2c.h s2c_dev.out), in [t][tile] order."""
    a, cb0 = (tiles[t0:t1, c].astype(np.int64) for c in (0, 8))   # (no int64 copy of the whole table: profiles/layout_fold_ab.json)
    slot = fill_w * a + cb0
    return (np.arange(n_thr, dtype=np.int64)[:, None] * out_stride + slot[None, :]).reshape(-1)
