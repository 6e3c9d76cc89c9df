"""The dense windows' extension (s2c.h s2c_dense_ext): the run records, 'N' events, X-run slots
and rare pieces' records the host writes beside the compact piece records, and k_tile_dense's
walk from them (s2c_run_lean / s2c_pileup_lean).

Without a GPU: the five arrays equal a numpy model built from pc, px, dwin and tiles alone — on
every case of test_dense_walk, on one more case of many 'N' events, on a C5-like batch and on
its shards; the X-run queue of the rare pass stays inside its capacity; the C-ABI refuses a
malformed extension before any launch.  On the GPU: the walk gives the batch model's statistics,
offsets and body bytes and the oracle's FASTA files, twice on one workspace; through a tile range
it gives the same bytes and the whole batch's statistics of those tiles."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import batch_model as bm
import s2c_oracle as o
import test_dense_walk as tdw
from test_host import _host_dev

from sam2consensus_amd import _lib as L
from sam2consensus_amd import batch, configs, shard

WT, WGD = tdw.WT, tdw.WGD
S, X, F, D, LONG = L.S2C_PF_SIMPLE, L.S2C_PF_X, L.S2C_PF_XFEW, L.S2C_PF_DASH, L.S2C_PF_LONG


def _n_events(rng):
    """A 30-base one-token read at every position of a 1,600-position reference, each with two
    'N' (some at offset 0 and at the last base): more 'N' events per window than WT, events at a
    tile's first and last position and just outside it."""
    kinds = [(0, 29), (0, 14), (7, 29), (3, 21), (28, 29), (0, 1)]
    return tdw._sam(1600, [(p, "30M", tdw._put(tdw._bases(rng, p, 30), kinds[i % len(kinds)], "N"))
                           for i, p in enumerate(range(1, 1571))])


CASES = dict(tdw.CASES, n_events=(_n_events, []))


@functools.lru_cache(maxsize=None)
def _case(name):
    """As test_dense_walk._case (shared with it for its own cases)."""
    if name in tdw.CASES:
        return tdw._case(name)
    build, args = CASES[name]
    sam = build(random.Random(name))
    opt = o.parse_argv(["-i", "case.sam"] + args)
    hb = batch.parse_text(sam, opt.maxdel_active, 150)
    want = bm.model_pipeline(hb, opt.thresholds, opt.min_depth, opt.fill.encode())
    ref = o.run_case(sam, args, name="case.sam")
    assert ref["status"] == "ok"
    return sam, opt, hb, want, ref


def _model_ext(hb):
    """The five arrays from pc, px, dwin and tiles alone, and per window the piece indices of
    its SIMPLE, rare and LONG pieces."""
    pc, px, tiles = hb.pc.astype(np.int64), hb.px.astype(np.int64), hb.tiles.astype(np.int64)
    drun, dnev, dxs, drare, dext, kinds = [], [], [], [], [], []
    n_run = n_nev = n_xs = n_rare = 0
    for w in hb.dwin.astype(np.int64):
        a, b = tiles[w[0], 0], tiles[w[0], 1]
        T0, TL = 32 * (a >> 5), 32 * ((b - a + 31) // 32)
        k = np.arange(w[6], w[7])
        nslot = int(w[9] - w[8])
        fl, slen = pc[k, 3] >> 24, pc[k, 3] & 0xFFFFFF
        rs, qh, oj, nops = pc[k, 0] - T0 + 2048, pc[k, 1] - 2 * w[10], pc[k, 2] - w[8], pc[k + 1, 2] - pc[k, 2]
        simple = (fl & S) != 0
        rare = ~simple & ((fl & LONG) == 0)
        run = np.zeros((nslot + (nslot & 1), 2), dtype=np.int64)
        run[oj[simple], 0] = rs[simple] | (rs[simple] + slen[simple]) << 16
        run[oj[simple], 1] = (16 * qh[simple] - rs[simple]) & 0xFFFFFFFF
        few = simple & ((fl & F) != 0)
        off = np.stack([px[k] & 0xFFFF, (px[k] >> 16) & 0xFFFF], axis=1)
        r = rs[:, None] + off - 2048
        keep = few[:, None] & (off < slen[:, None]) & (r >= 0) & (r < TL)
        nev = r[keep]            # (row-major: piece order, offset 0 before offset 1)
        xs = oj[simple & ((fl & X) != 0) & ((fl & F) == 0)]
        rec = np.stack([rs | qh << 12 | nops << 25, oj | slen << 13 | fl << 24, px[k]], axis=1)[rare]
        dext.append([n_run, nslot, n_nev, len(nev), n_xs, len(xs), n_rare, len(rec)])
        n_run, n_nev, n_xs, n_rare = n_run + len(run), n_nev + len(nev), n_xs + len(xs), n_rare + len(rec)
        drun.append(run), dnev.append(nev), dxs.append(xs), drare.append(rec)
        kinds.append((k[simple], k[rare], k[~simple & ~rare], oj, nops, simple))
    cat = lambda parts, shape: (np.concatenate(parts) if parts else np.zeros(shape, dtype=np.int64)).astype(np.uint32)  # noqa: E731
    return (cat(drun, (0, 2)), cat(dnev, (0,)), cat(dxs, (0,)), cat(drare, (0, 3)),
            np.array(dext, dtype=np.uint32).reshape(-1, L.S2C_DEXT_WORDS)), kinds


def _check_ext(hb):
    (drun, dnev, dxs, drare, dext), kinds = _model_ext(hb)
    assert hb.dext.shape == (hb.info.n_dense, L.S2C_DEXT_WORDS)
    assert (hb.dext == dext).all()
    assert hb.drun.shape == drun.shape and (hb.drun == drun).all()
    assert hb.dnev.shape == dnev.shape and (hb.dnev == dnev).all()
    assert hb.dxs.shape == dxs.shape and (hb.dxs == dxs).all()
    assert hb.drare.shape == drare.shape and (hb.drare == drare).all()
    assert (hb.dext[:, 0] % 2 == 0).all()                    # 8-byte records: every block on 16 bytes
    assert hb.drun.ctypes.data % 16 == 0 or len(hb.drun) == 0
    n_long = 0
    for x, (ks, kr, kl, oj, nops, simple) in zip(hb.dext.astype(np.int64), kinds):
        blk = hb.drun[x[0]:x[0] + x[1] + (x[1] & 1)]
        zero = ~blk.any(axis=1)
        want_zero = np.ones(len(blk), dtype=bool)
        want_zero[oj[simple]] = False
        assert (zero == want_zero).all()                     # zero records exactly at the non-SIMPLE slots
        assert (nops[simple] == 1).all()
        assert x[7] == len(kr)
        n_long += len(kl)
    assert not ((hb.drare[:, 1] >> 24) & (S | LONG)).any()   # neither SIMPLE nor LONG pieces among the rare
    return n_long


@pytest.mark.parametrize("name", list(CASES))
def test_extension_equals_numpy_model(name):
    _, _, hb, _, _ = _case(name)
    assert hb.info.n_dense > 0
    _check_ext(hb)
    if name == "n_events":
        tiles = hb.tiles.astype(np.int64)
        first = last = 0
        for x, w in zip(hb.dext.astype(np.int64), hb.dwin.astype(np.int64)):
            ev = hb.dnev[x[2]:x[2] + x[3]].astype(np.int64)
            TL = 32 * ((tiles[w[0], 1] - tiles[w[0], 0] + 31) // 32)
            assert len(ev) > WT
            first, last = first + int((ev == 0).sum()), last + int((ev == TL - 1).sum())
            # events just outside the tile's words were dropped: fewer than 2 per window piece
            assert len(ev) < 2 * (w[7] - w[6])
        assert first and last and len(hb.dwin) > 1
    if name == "many_dels":
        assert (hb.dext[:, 7] > WT).any()        # more rare pieces than threads
    if name == "big_window":
        # (windows of more than 256 pieces; more 'N' events and more rare pieces than threads are
        # n_events' and many_dels')
        assert (hb.dwin[:, 7].astype(np.int64) - hb.dwin[:, 6] > tdw.BIG_WINDOW).any() and hb.dext[:, 3].any() and hb.dext[:, 7].any()


def test_extension_equals_numpy_model_c5_and_shards():
    hb = configs.synth_batch("c5", ref_len=200_000, ins_frac=0.01)
    try:
        n_long = 0
        for b in [hb] + [shard.sub_batch(hb, r, 3) for r in range(3)]:
            assert b.info.n_dense > 0
            n_long += _check_ext(b)
            assert b.dext[:, 3].any() and b.dext[:, 7].any()
            if b is not hb:
                b.free()
        assert n_long    # long pieces start in dense windows here: left out of drare, their slots zero
    finally:
        hb.free()


@pytest.mark.parametrize("name", ["many_dels", "many_dels_x"])
def test_x_run_queue_stays_inside_its_capacity(name):
    """The rare pass's X-run queue (s2c_dense.hip) replayed: thread i takes rare piece i, wave 0
    writes its deletion reads' X runs from the front, wave 1 from the back of qcap = min(2·rare,
    op slots + 128) entries; the two ends never meet."""
    _, _, hb, _, _ = _case(name)
    wrote = 0
    for x, (w, k, fl, nops, pos, px) in zip(hb.dext.astype(np.int64), tdw._windows(hb)):
        rare = [i for i in range(len(k)) if not fl[i] & (S | LONG)]
        assert len(rare) == x[7]
        qcap = min(2 * len(rare), int(x[1]) + 128)
        end = [0, 0]
        for n, i in enumerate(rare):
            kk = int(k[i])
            if tdw._is_del_read(hb, kk, int(fl[i]), int(nops[i])) and fl[i] & X and not fl[i] & F \
                    and not (fl[i] & D and hb.maxdel_active):
                (_, l), _, (_, l2) = tdw._ops(hb, kk)
                slen = int(hb.pc[kk, 3]) & 0xFFFFFF
                end[(n % WT) // WGD] += 1 + (1 if l < slen and min(l2, slen - l) > 0 else 0)
        assert end[0] + end[1] <= qcap               # entries [0, end0) and [qcap − end1, qcap) are disjoint
        assert qcap <= int(x[1]) + 128               # ... and inside the queue's share of the window's LDS
        wrote += end[0] + end[1]
    assert wrote


def _ext_of(hb):
    x = L.DenseExt()
    L.check(L.lib.s2c_batch_dense_ext_get(hb._b, C.byref(x)))
    return x


def _lean_of(hb):
    y = L.DenseLean()
    L.check(L.lib.s2c_batch_dense_lean_get(hb._b, C.byref(y)))
    return y


def test_run_lean_refuses_a_malformed_extension_before_launch():
    """S2C_ERR_ARG over host pointers (never dereferenced: the calls return before any launch),
    with a valid lean part beside the extension: the extension is checked first."""
    _, _, hb, _, _ = _case("dels_maxdel_on")
    hb.ensure_layers()
    d, keep = _host_dev(hb)
    y = _lean_of(hb)
    for g in (L.lib.s2c_run_lean, L.lib.s2c_pileup_lean):
        f = lambda dv, x, stream, g=g: g(dv, x, C.byref(y), stream)  # noqa: E731
        for name in ("drun", "dnev", "dxs", "drare", "dext"):
            x = _ext_of(hb)
            setattr(x, "n_" + name, max(getattr(x, "n_" + name), 1))
            setattr(x, name, None)
            assert f(C.byref(d), C.byref(x), None) == L.S2C_ERR_ARG
            assert name in L.last_error() and "NULL" in L.last_error()
            x = _ext_of(hb)
            setattr(x, "n_" + name, -1)
            assert f(C.byref(d), C.byref(x), None) == L.S2C_ERR_ARG
        for dn in (-1, 1):
            x = _ext_of(hb)
            x.n_dext += dn
            assert f(C.byref(d), C.byref(x), None) == L.S2C_ERR_ARG
            assert "n_dense" in L.last_error()
        # s2c_dev's own guards come first, with their messages
        bad = L.Dev.from_buffer_copy(d)
        bad.n_thr = 0
        x = _ext_of(hb)
        x.dext = None
        assert f(C.byref(bad), C.byref(x), None) == L.S2C_ERR_ARG
        assert "no thresholds" in L.last_error()


def _workspace(hb, opt, tile_range=None):
    """The case's workspace (its run is s2c_run_lean with the batch's extension)."""
    from sam2consensus_amd import engine
    fill = opt.fill.encode()
    db = engine.DeviceBatch(hb, dense_layers=engine.needs_dense_layers(fill, False))
    return engine.Workspace(db, opt.thresholds, opt.min_depth, fill, False, tile_range=tile_range)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_extension_walk_equals_model_and_oracle(name):
    _, opt, hb, want, ref = _case(name)
    ws = _workspace(hb, opt)
    for _ in range(2):
        ws.out.zero_(), ws.tile_stats.zero_(), ws.blk_len.zero_()   # (nothing of the earlier run is left)
        ws.run()
        st, offs, out = ws.fetch()
        assert (st == want[0]).all()
        assert (offs == want[1]).all()
        assert out == want[2]
    assert tdw._files(hb, opt, st, offs, out) == ref["files"]


def _tile_stats(ws, T, nb):
    """The device's per-tile statistics of a finished run, [T][n_tiles][4] u64."""
    import torch
    return ws.tile_stats[: T * nb * 32].view(torch.int64).cpu().numpy().view(np.uint64).reshape(T, nb, 4)


@pytest.mark.gpu
def test_extension_walk_through_a_tile_range():
    """A workspace over tiles [1, n): dext filtered like dwin; it gives the model's bytes, and its
    per-tile statistics of tiles [1, n) are the rows of a whole-batch workspace's run."""
    _, opt, hb, want, _ = _case("big_window")
    nb, T = int(hb.info.n_tiles), len(opt.thresholds)
    assert nb > 2 and hb.info.n_dense == nb
    t0, t1 = 1, nb
    ws = _workspace(hb, opt, tile_range=(t0, t1))
    assert ws.ext.n_dext == ws.dev.n_dense == t1 - t0
    wo = want[1].astype(np.int64)
    body = b"".join(bytes(want[2][wo[t * nb + t0]:wo[t * nb + t1]]) for t in range(T))
    lens = np.concatenate([np.diff(wo)[t * nb + t0:t * nb + t1] for t in range(T)])
    ws.out.zero_(), ws.tile_stats.zero_(), ws.blk_len.zero_()
    ws.run()
    st, offs, out = ws.fetch()
    assert (np.diff(offs.astype(np.int64)) == lens).all()
    assert bytes(out) == body
    part = _tile_stats(ws, T, nb)
    whole = _workspace(hb, opt)
    whole.tile_stats.zero_()
    whole.run()
    st_all, _, _ = whole.fetch()
    assert (st_all == want[0]).all()
    rows = _tile_stats(whole, T, nb)
    assert rows[:, t0:t1].any() and (part[:, t0:t1] == rows[:, t0:t1]).all()
    assert not part[:, :t0].any()                     # (the range's run wrote no other tile's row)
