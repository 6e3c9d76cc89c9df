"""The lean part of the dense windows' extension (s2c.h s2c_dense_lean): the rare pieces' op
words the host writes per window (k_tile_dense stages no other op word), their per-piece offsets,
the windows' rows, and the three numbers that size the launch — the largest lean window, the
largest count a lane can reach, the plane pairs of the counters' exchange.

Without a GPU: all of it equals a numpy model built from dwin, dext, drare, rs and ops alone (for
the lane count the model restates the host's rule, so it pins the host's arithmetic and the edges;
that the rule is the kernel's own is pinned by the GPU runs below: a kernel that exchanged more
plane pairs than the launch was sized for would write past its LDS and lose parity) — on
every case of test_dense_walk and test_dense_ext, on a C5-like batch and its shards, and on
cases that sit on the edges: rare pieces of 4, 5 and 48 op slots (48 = S2C_CHUNK_RECS / 4 is the
most a rare piece holds: the plan makes a piece of more slots a long piece, so the piece of
exactly S2C_DPC_NOPS_MAX = 127 slots built here is checked to be long, in no dense window — its
tile runs through k_tile — and its op words not in the block), windows with no rare piece, and
largest lane counts of 15 | 16 (2 → 3 plane pairs) and 63 | 64 (3 → 4) on the 64-word instantiation
and 16 and 64 on the 32-word one, each checked on the host to land on its side of the edge; in
the count cases the exchange's bytes exceed the window's; s2c_run / s2c_pileup refuse a batch
that would launch k_tile_dense (dense tiles, a one-char fill) and take one that would not (a
longer fill over built dense layers).  On the GPU, for each edge case: the run gives the batch
model's statistics, offsets and bytes and the oracle's files, twice on one workspace and once
through a tile range."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import batch_model as bm
import s2c_oracle as o
import test_dense_ext as tde
import test_dense_walk as tdw
from test_host import _host_dev

from sam2consensus_amd import _lib as L
from sam2consensus_amd import batch, configs, shard

NOPS_RARE_MAX = 48          # s2c.h S2C_CHUNK_RECS / 4: a piece of more op slots is long
NOPS_MAX = 127              # s2c.h S2C_DPC_NOPS_MAX
DENSE_LDS = 32768           # s2c.h S2C_DENSE_LDS


def _nwp(tile_max):
    return 16 if tile_max <= 512 else 32 if tile_max <= 1024 else 64


def _slots(n):              # s2c.h S2C_DENSE_SLOTS
    return 8 * (n // 8) + (8 if n % 8 > 4 else 4 if n % 8 else 0)


def _pairs(c):              # s2c.h S2C_DENSE_PAIRS
    return 1 if c < 4 else 2 if c < 16 else 3 if c < 64 else 4


def _xch_bytes(pairs, nwp):  # s2c.h S2C_DENSE_XCH_BYTES
    return 2 * max(2080 * pairs, 80 * nwp)


def _model_lean(hb):
    """(rop, roff, row, per-window lean bytes, per-window largest lane count) from dwin, dext,
    drare, rs and ops alone."""
    nwp = _nwp(int(hb.info.tile_max))
    G, K, pad = 128 // nwp, int(hb.info.kwin), 1024 // nwp
    rs, ops = hb.rs.astype(np.int64), hb.ops
    rop, roff, row, nbytes, counts = [], [], [], [], []
    n_rop = 0
    for w, x in zip(hb.dwin.astype(np.int64), hb.dext.astype(np.int64)):
        rec = hb.drare[x[6]:x[6] + x[7]].astype(np.int64)
        oj, nops = rec[:, 1] & 0x1FFF, rec[:, 0] >> 25
        blk = [ops[w[8] + j:w[8] + j + n] for j, n in zip(oj, nops)]
        roff.append(np.cumsum(nops) - nops)
        nrop = int(nops.sum())
        row.append([n_rop, nrop])
        n_rop += nrop
        rop += blk
        ns, nq, nrare = int(x[1]), int(w[11] - w[10]), int(x[7])
        nbytes.append((((8 * nq + 30) & ~15) + ((4 * nrop + 30) & ~15) + 8 * (ns + pad) + 4 * min(2 * nrare, ns + 128) + 15) & ~15)
        # per wave (nwp / 2 words): the record slots its longest lane reads, plus the long rounds
        W0, nwords, ntr = int(w[1]) >> 5, int(w[2] - w[1] + 31) // 32, int(w[5] - w[4] + G - 1) // G
        c = 0
        for wa in range(0, nwords, nwp // 2):
            Ws = np.arange(W0 + wa, W0 + min(wa + nwp // 2, nwords))
            cand = rs[Ws + 1] - rs[np.maximum(Ws - K, 0)]
            c = max(c, _slots(int(((cand + G - 1) // G).max())) + ntr)
        counts.append(c)
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)).astype(np.uint32)  # noqa: E731
    return cat(rop), cat(roff), np.array(row, dtype=np.uint32).reshape(-1, L.S2C_DLEAN_WORDS), nbytes, counts


def _check_lean(hb):
    rop, roff, row, nbytes, counts = _model_lean(hb)
    assert hb.rop.shape == rop.shape and (hb.rop == rop).all()
    assert hb.roff.shape == roff.shape == (len(hb.drare),) and (hb.roff == roff).all()
    assert hb.drow.shape == row.shape == (hb.info.n_dense, L.S2C_DLEAN_WORDS) and (hb.drow == row).all()
    assert hb.lean_lds == max(nbytes) and hb.lean_lds % 16 == 0
    assert hb.lean_lds <= hb.info.dense_lds <= DENSE_LDS       # never more than the window with its op words
    assert hb.lean_count == max(counts)
    assert hb.lean_pairs == _pairs(max(counts)) and 1 <= hb.lean_pairs <= 4
    return nbytes, counts


# ---- the edge cases: 30-base reads on references of at most 1,600 positions

def _ops_edges(rng):
    """One-token reads over the first 600 positions only (windows with no rare piece); from 700
    on, among them, deletion reads of 3 op slots and rare pieces of 4, 5 and NOPS_RARE_MAX slots;
    one piece of NOPS_MAX slots (a long piece)."""
    reads = [(p, "30M", tdw._bases(rng, p, 30)) for p in range(1, 1560, 2)]
    for i, p in enumerate(range(700, 1500, 9)):
        s = tdw._bases(rng, p, 30)
        cig = ["12M2D18M", "5M1D5M2D20M", "4S10M3D16M", "6M1D6M1N6M1D12M"][i % 4]
        reads.append((p, cig, tdw._put(s, [7], "N") if i % 3 == 0 else s))
    many = lambda nd: "".join("1M1D" if k < nd else "1M" for k in range(29)) + "1M"  # noqa: E731  (30 M tokens, nd D tokens)
    reads.append((1300, many(NOPS_RARE_MAX - 30), tdw._bases(rng, 1300, 30)))
    # 30 M tokens and 97 D / N / P tokens between them
    gaps = ["1D1N1P1D" if k < 10 else "1D1N1P" for k in range(29)]
    reads.append((1100, "".join("1M" + g for g in gaps) + "1M", tdw._bases(rng, 1100, 30)))
    return tdw._sam(1600, sorted(reads))


def _spike(n_spike, n_long, ln=1600):
    """A sparse reference of ln positions — 1,600: one tile of 50 words, k_tile_dense<64>, two
    lanes per word; 1,000: one tile of 32 words, k_tile_dense<32>, four lanes per word — with
    n_spike one-token reads starting in one word, and n_long reads whose deletion spans more than
    1,024 positions (long pieces: a long round per two of them)."""
    def build(rng):
        reads = [(p, "30M", tdw._bases(rng, p, 30)) for p in range(1, ln - 40, 16)]
        reads += [(801 + i % 30, "30M", tdw._put(tdw._bases(rng, 801 + i % 30, 30), [i % 30], "N") if i % 9 == 4
                   else tdw._bases(rng, 801 + i % 30, 30)) for i in range(n_spike)]
        reads += [(40 + 70 * i, "15M1100N15M", tdw._bases(rng, 40 + 70 * i, 30)) for i in range(n_long)]
        reads.append((ln - 300, "12M2D18M", tdw._bases(rng, ln - 300, 30)))
        return tdw._sam(ln, sorted(reads))
    return build


EDGE = {
    "ops_edges": (_ops_edges, []),
    "count_15": (_spike(18, 5), []),
    "count_16": (_spike(26, 0), []),
    "count_63": (_spike(114, 5), []),
    "count_64": (_spike(122, 0), []),
    # the same edges' upper sides on the 32-word instantiation (C5's).  Their lower sides need three
    # long rounds there, i.e. nine long pieces: a span over 1,024 does not fit 1,000 positions, and
    # a piece long by its op slots brings 49 candidates to its word — more than the count allows
    "count_16_w32": (_spike(54, 0, 1000), []),
    "count_64_w32": (_spike(244, 0, 1000), []),
}
WANT_COUNT = {"count_15": 15, "count_16": 16, "count_63": 63, "count_64": 64, "count_16_w32": 16, "count_64_w32": 64}


@functools.lru_cache(maxsize=None)
def _edge(name):
    build, args = EDGE[name]
    sam = build(random.Random(name))
    opt = o.parse_argv(["-i", "case.sam"] + args)
    hb = batch.parse_text(sam, opt.maxdel_active, 150)
    want = bm.model_pipeline(hb, opt.thresholds, opt.min_depth, opt.fill.encode())
    ref = o.run_case(sam, args, name="case.sam")
    assert ref["status"] == "ok"
    return sam, opt, hb, want, ref


@pytest.mark.parametrize("name", list(tde.CASES))
def test_lean_part_equals_numpy_model(name):
    _, _, hb, _, _ = tde._case(name)
    assert hb.info.n_dense > 0
    _check_lean(hb)
    if name == "many_dels":
        assert (hb.dext[:, 7] > tdw.WT).any()          # a window with more rare pieces than threads
        assert (hb.drow[:, 1] == 3 * hb.dext[:, 7]).all()


def test_lean_part_equals_numpy_model_c5_and_shards():
    hb = configs.synth_batch("c5", ref_len=200_000, ins_frac=0.01)
    try:
        for b in [hb] + [shard.sub_batch(hb, r, 3) for r in range(3)]:
            assert b.info.n_dense > 0 and len(b.rop) > 0
            nbytes, _ = _check_lean(b)
            assert b.lean_pairs < 4 and max(nbytes) < b.info.dense_lds
            if b is not hb:
                b.free()
    finally:
        hb.free()


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_cases_land_on_their_side(name):
    _, _, hb, want, ref = _edge(name)
    assert hb.info.n_dense > 0
    nbytes, counts = _check_lean(hb)
    nwp = _nwp(int(hb.info.tile_max))
    if name == "ops_edges":
        nops = hb.drare[:, 0] >> 25
        assert {3, 4, 5, NOPS_RARE_MAX} <= set(nops.tolist()) and nops.max() == NOPS_RARE_MAX
        assert (hb.dext[:, 7] == 0).any() and (hb.drow[hb.dext[:, 7] == 0, 1] == 0).all()   # windows with no rare piece
        assert hb.info.n_dense > 2
        # the piece of NOPS_MAX op slots is long: not among the rare, its op words not in the block
        pc = hb.pc.astype(np.int64)
        big = np.flatnonzero(pc[1:, 2] - pc[:-1, 2] == NOPS_MAX)
        assert len(big) == 1 and (pc[big[0], 3] >> 24) & L.S2C_PF_LONG
        assert len(hb.rop) == int(nops.sum())
        # ... and no dense window holds it: the tile it starts in goes to k_tile
        assert not ((hb.dwin[:, 6] <= big[0]) & (big[0] < hb.dwin[:, 7])).any() and hb.info.n_dense == hb.info.n_tiles - 1
    else:
        assert hb.info.n_tiles == hb.info.n_dense == 1 and nwp == (32 if name.endswith("w32") else 64)
        assert hb.lean_count == WANT_COUNT[name]
        assert hb.lean_pairs == {15: 2, 16: 3, 63: 3, 64: 4}[WANT_COUNT[name]]
        assert (hb.dwin[0, 5] - hb.dwin[0, 4] + 1) // 2 == (3 if WANT_COUNT[name] % 2 else 0)   # long rounds (G = 2)
        # the exchange's bytes exceed the window's: the launch is sized by the plane pairs
        assert _xch_bytes(hb.lean_pairs, nwp) > hb.lean_lds
        assert hb.dext[0, 7] > 0


_lean_of = tde._lean_of


def test_run_lean_refuses_a_malformed_lean_part_before_launch():
    """S2C_ERR_ARG over host pointers (never dereferenced: the calls return before any launch)."""
    _, _, hb, _, _ = tde._case("dels_maxdel_on")
    hb.ensure_layers()
    d, keep = _host_dev(hb)
    for f in (L.lib.s2c_run_lean, L.lib.s2c_pileup_lean):
        x, y = tde._ext_of(hb), _lean_of(hb)
        assert f(C.byref(d), C.byref(x), None, None) == L.S2C_ERR_ARG and "s2c_dense_lean" in L.last_error()
        assert f(C.byref(d), None, C.byref(y), None) == L.S2C_ERR_ARG
        for name in ("rop", "roff", "row"):
            y = _lean_of(hb)
            setattr(y, "n_" + name, max(getattr(y, "n_" + name), 1))
            setattr(y, name, None)
            assert f(C.byref(d), C.byref(x), C.byref(y), None) == L.S2C_ERR_ARG
            assert name in L.last_error() and "NULL" in L.last_error()
        for field, val in (("n_roff", x.n_drare + 1), ("n_row", d.n_dense + 1), ("lds", 0), ("lds", DENSE_LDS + 16),
                           ("lds", y.lds + 8), ("pairs", 0), ("pairs", 5), ("count_max", 64 if y.pairs < 4 else -1)):
            y = _lean_of(hb)
            setattr(y, field, val)
            assert f(C.byref(d), C.byref(x), C.byref(y), None) == L.S2C_ERR_ARG, field


def test_run_and_pileup_refuse_a_batch_that_needs_the_extension():
    """s2c_run / s2c_pileup (no extension) on dense tiles with a one-char fill: S2C_ERR_ARG naming
    the entries to call, over host pointers (never dereferenced: nothing is launched); so do the
    _lean entries given neither part.  s2c_dev's own guards still come first."""
    _, _, hb, _, _ = tde._case("dels_maxdel_on")
    hb.ensure_layers()
    d, keep = _host_dev(hb)
    assert d.n_dense > 0 and d.fill_len == 1
    for f, entry in ((L.lib.s2c_run, "s2c_run_lean"), (L.lib.s2c_pileup, "s2c_pileup_lean")):
        assert f(C.byref(d), None) == L.S2C_ERR_ARG
        assert entry in L.last_error() and "s2c_dense_ext" in L.last_error()
        bad = L.Dev.from_buffer_copy(d)
        bad.n_thr = 0
        assert f(C.byref(bad), None) == L.S2C_ERR_ARG and "no thresholds" in L.last_error()
    for f in (L.lib.s2c_run_lean, L.lib.s2c_pileup_lean):
        assert f(C.byref(d), None, None, None) == L.S2C_ERR_ARG and "s2c_pileup_lean" in L.last_error()


def test_pileup_takes_a_longer_fill_over_dense_layers_without_the_extension():
    """With -f NN and the dense tiles' layers built, k_tile takes the dense tiles: s2c_pileup does
    not ask for the extension.  Nothing is launched here: the s2c_dev claims 2^31 dense tiles, which
    the launch's own limit refuses on the host — after every argument check, the refusal included —
    while the same s2c_dev with a one-char fill is refused for its missing extension first."""
    sam, opt, _, _, _ = tde._case("dels_maxdel_on")
    hb = batch.parse_text(sam, opt.maxdel_active, 150)
    try:
        hb.ensure_layers(True)
        assert hb.info.n_dense > 0 and hb.info.layers_dense == 1
        d, keep = _host_dev(hb, fill=b"NN")
        d.n_dense = 1 << 31
        assert L.lib.s2c_pileup(C.byref(d), None) == L.S2C_ERR_LIMIT
        assert "too many work items" in L.last_error() and "s2c_pileup_lean" not in L.last_error()
        d, keep = _host_dev(hb, fill=b"N")
        d.n_dense = 1 << 31
        assert L.lib.s2c_pileup(C.byref(d), None) == L.S2C_ERR_ARG and "s2c_pileup_lean" in L.last_error()
    finally:
        hb.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE))
def test_edge_cases_on_the_gpu(name):
    _, opt, hb, want, ref = _edge(name)
    ws = tde._workspace(hb, opt)
    assert ws.lean.pairs == hb.lean_pairs and ws.lean.lds == hb.lean_lds
    for _ in range(2):                                      # twice on one workspace
        ws.out.zero_(), ws.tile_stats.zero_(), ws.blk_len.zero_()
        ws.run()
        st, offs, out = ws.fetch()
        assert (st == want[0]).all()
        assert (offs == want[1]).all()
        assert out == want[2]
        assert tdw._files(hb, opt, st, offs, out) == ref["files"]
    # ... and through a tile range: every tile but the first (a batch of one tile: that tile)
    nb, T = int(hb.info.n_tiles), len(opt.thresholds)
    t0, t1 = (1, nb) if nb > 1 else (0, 1)
    ws = tde._workspace(hb, opt, tile_range=(t0, t1))
    assert ws.lean.n_row == ws.ext.n_dext == ws.dev.n_dense == int(((hb.dwin[:, 0] >= t0) & (hb.dwin[:, 0] < t1)).sum()) > 0
    wo = want[1].astype(np.int64)
    body = b"".join(bytes(want[2][wo[t * nb + t0]:wo[t * nb + t1]]) for t in range(T))
    lens = np.concatenate([np.diff(wo)[t * nb + t0:t * nb + t1] for t in range(T)])
    ws.out.zero_(), ws.tile_stats.zero_(), ws.blk_len.zero_()
    ws.run()
    st, offs, out = ws.fetch()
    assert (np.diff(offs.astype(np.int64)) == lens).all()
    assert bytes(out) == body
