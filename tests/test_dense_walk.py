"""k_tile_dense's walk on hand-written SAMs: the one-token reads (with their 'N' offsets), the
rare pass over every other piece (deletion reads, '-' in SEQ, clipped and wrapped reads), more
rare pieces than a tile's threads, windows of more than 256 pieces, and a last tile that ends
mid-word.

Each case is checked twice: without a GPU, that its plan puts the stated feature into a dense
window and that the batch model equals the oracle on it; on the GPU, that the device pipeline
equals the batch model (stats, offsets, body bytes, two runs) and the oracle's FASTA files."""
import functools
import random

import numpy as np
import pytest

import batch_model as bm
import s2c_oracle as o

from sam2consensus_amd import _lib as L
from sam2consensus_amd import batch

OP_M, OP_D, OP_N, OP_S, OP_H, OP_P, OP_EQ, OP_X = 0, 2, 3, 4, 5, 6, 7, 8   # s2c.h S2C_OP_*
WT, WGD = 128, 64   # k_tile_dense: threads per tile, lanes per wave
BIG_WINDOW = 256    # pieces: big_window's windows hold more, with rare and 'N' pieces past that index


def _bases(rng, p, n):
    """n bases of the case's genome from position p (1-based; wrapping), 2 % of them changed."""
    if not hasattr(rng, "genome"):
        rng.genome = [rng.choice("ACGT") for _ in range(4096)]
    return "".join(rng.choice("ACGT") if rng.random() < 0.02 else rng.genome[(p - 1 + i) % 4096] for i in range(n))


def _put(seq, offs, ch):
    s = list(seq)
    for i in offs:
        s[i] = ch
    return "".join(s)


def _sam(ln, reads):
    """reads: (POS, CIGAR, SEQ), any order of POS."""
    return "@SQ\tSN:g\tLN:%d\n" % ln + "".join(
        "r%d\t0\tg\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (i, p, c, s) for i, (p, c, s) in enumerate(reads))


def _xfew(rng):
    """One-token reads only: one and two 'N' per read at SEQ offset 0, the last base, and at or
    past take (a token shorter than SEQ); a read every 3 positions, so reads of every kind
    start in the lookback words of a tile and cross a tile's end."""
    kinds = [(), (0,), (59,), (0, 59), (17, 41), (0, 1), (58, 59)]
    reads = []
    for i, p in enumerate(range(1, 2900, 3)):
        s = _put(_bases(rng, p, 60), kinds[i % len(kinds)], "N")
        if i % 11 == 5:      # 40M over a SEQ of 60: offsets 39 (the last base taken), 40 and 59 (≥ take)
            reads.append((p, "40M", _put(_bases(rng, p, 60), [(39, 59), (40,), (39, 40)][i % 3], "N")))
        else:
            reads.append((p, "60M", s))
    return _sam(3000, reads)


def _dash(rng):
    """One-token reads whose SEQ holds '-' (never S2C_PF_SIMPLE): a few '-', and SEQs of 320
    with exactly 150 and 151 '-' (the maxdel bound of :210 and one more)."""
    reads = []
    for i, p in enumerate(range(1, 2600, 4)):
        s = _bases(rng, p, 60)
        if i % 3 == 0:
            s = _put(s, rng.sample(range(60), 1 + i % 4), "-")
        if i % 5 == 0:
            s = _put(s, [rng.randrange(60)], "N")
        reads.append((p, "60M", s))
    for j, p in enumerate(range(40, 2200, 90)):
        s = _put(_bases(rng, p, 320), rng.sample(range(320), 150 + j % 2), "-")
        reads.append((p, "320M", s))
    return _sam(3000, sorted(reads))


def _dels(rng):
    """Deletion reads (bases, D / N / P, bases) among one-token reads: 'N' before and after the
    deletion (one or two: S2C_PF_XFEW; three and more: their runs queued for the plane scan),
    deletions of every length up to 40 at every phase of the tiles (so '-' runs cross tile
    ends), deletions of 150 and 151 (the maxdel bound and one more), and first tokens at or
    past len(SEQ) (an empty second run)."""
    reads = []
    for i, p in enumerate(range(1, 2800, 4)):
        s = _bases(rng, p, 50)
        m = i % 9
        if m == 0:
            reads.append((p, "50M", s))
        elif m == 1:
            reads.append((p, "20M%dD30M" % (1 + i % 40), _put(s, [3], "N")))
        elif m == 2:
            reads.append((p, "20M%dN30M" % (1 + i % 37), _put(s, [33], "N")))
        elif m == 3:
            reads.append((p, "25M%dD25M" % (1 + i % 40), _put(s, [0, 49], "N")))
        elif m == 4:
            reads.append((p, "25M%dP25M" % (2 + i % 5), _put(s, [1, 24, 25, 48], "N")))
        elif m == 5:
            reads.append((p, "10M%dD40M" % (1 + i % 40), _put(s, [2, 5, 7], "N")))   # all three before the deletion
        elif m == 6:
            reads.append((p, "50M%dD20M" % (1 + i % 12), s))                          # l = len(SEQ): no second run
        elif m == 7:
            reads.append((p, "60M%dD20M" % (1 + i % 12), _put(s, [49], "N")))         # l > len(SEQ)
        else:
            reads.append((p, "30M%dD20M" % (1 + i % 40), s))
    for j, p in enumerate(range(100, 2400, 260)):
        reads.append((p, "25M%dD25M" % (150 + j % 2), _put(_bases(rng, p, 50), [4, 40] if j % 4 < 2 else [], "N")))
    return _sam(3200, sorted(reads))


def _many_dels(rng):
    """Every read is a deletion read, one starting at each position: more than 64 rare pieces
    in each wave of a window, a quarter of them with three 'N' (X runs to queue)."""
    reads = []
    for i, p in enumerate(range(1, 1500)):
        s = _bases(rng, p, 24)
        if i % 4 == 0:
            s = _put(s, [1, 13, 22], "N")
        elif i % 4 == 1:
            s = _put(s, [11, 12], "N")
        reads.append((p, "12M%dD12M" % (1 + i % 6), s))
    return _sam(1600, reads)


def _many_dels_x(rng):
    """As _many_dels with every read holding three 'N': every read queues its X runs."""
    reads = []
    for i, p in enumerate(range(1, 1500)):
        reads.append((p, "12M%dD12M" % (1 + i % 6), _put(_bases(rng, p, 24), [1, 13, 22], "N")))
    return _sam(1600, reads)


def _big_window(rng):
    """Windows of more than 256 pieces: a one-token read at every position (some with 'N'), a
    deletion read and a read with '-' in SEQ here and there."""
    reads = []
    for i, p in enumerate(range(1, 1900)):
        s = _bases(rng, p, 30)
        if i % 7 == 3:
            s = _put(s, [i % 30], "N")
        if i % 13 == 6:
            reads.append((p, "14M3D16M", s))
        elif i % 17 == 9:
            reads.append((p, "30M", _put(s, [5], "-")))
        else:
            reads.append((p, "30M", s))
    return _sam(2000, reads)


def _clips(rng):
    """Soft- and hard-clipped reads and reads with POS ≤ 0 (their seqout wraps: a range piece
    at the reference's end) among one-token reads."""
    reads = [(-5, "40M", _bases(rng, -5, 40)), (0, "30M", _bases(rng, 0, 30)), (-20, "10S30M", _put(_bases(rng, -30, 40), [15], "N"))]
    for i, p in enumerate(range(1, 1500, 3)):
        s = _bases(rng, p, 50)
        m = i % 6
        if m == 0:
            reads.append((p, "5S45M", s))
        elif m == 1:
            reads.append((p, "3H47M3S", _put(s, [1, 48], "N")))
        elif m == 2:
            reads.append((p, "40M10S", _put(s, [45], "-")))
        elif m == 3:
            reads.append((p, "4S20M2D26M", s))
        else:
            reads.append((p, "50M", s))
    return _sam(1600, sorted(reads))


def _midword(rng):
    """A reference of 1,483 positions: its last tile ends 11 positions into a word; reads
    (one-token with 'N', deletion reads) run up to its last position."""
    reads = []
    for i, p in enumerate(range(1, 1440, 2)):
        s = _bases(rng, p, 40)
        if i % 5 == 1:
            s = _put(s, [0, 39], "N")
        reads.append((p, "18M4D22M" if i % 4 == 2 else "40M", s))
    reads += [(1440, "18M4D22M", _bases(rng, 1440, 40)), (1444, "40M", _put(_bases(rng, 1444, 40), [39], "N"))]
    return _sam(1483, reads)


# name → (SAM builder, CLI arguments); `-d` switches the maxdel rule (:210, bound 150) off
CASES = {
    "xfew": (_xfew, []),
    "dash_maxdel_off": (_dash, ["-d", "150"]),
    "dash_maxdel_on": (_dash, []),
    "dels_maxdel_on": (_dels, []),
    "dels_maxdel_off": (_dels, ["-d", "150"]),
    "many_dels": (_many_dels, []),
    "many_dels_x": (_many_dels_x, []),
    "big_window": (_big_window, []),
    "clips": (_clips, []),
    "midword": (_midword, ["--consensus-thresholds=0.25,0.75"]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's text, options, batch, batch model and oracle result: computed once, shared."""
    build, args = CASES[name]
    sam = build(random.Random(name))
    opt = o.parse_argv(["-i", "case.sam"] + args)
    hb = batch.parse_text(sam, opt.maxdel_active, 150)
    want = bm.model_pipeline(hb, opt.thresholds, opt.min_depth, opt.fill.encode())
    ref = o.run_case(sam, args, name="case.sam")
    assert ref["status"] == "ok"
    return sam, opt, hb, want, ref


def _files(hb, opt, st, offs, out):
    from sam2consensus_amd.records import build_records, render
    recs = build_records(hb, opt.thresholds, "case", st, offs, out)
    return {n + "__case.fasta": render(r, 0).decode("latin-1") for n, r in recs.items()}


def _windows(hb):
    """Per dense window: (window words, piece indices, flags, op slots, start positions, px)."""
    pc = hb.pc.astype(np.int64)
    for w in hb.dwin.astype(np.int64):
        k = np.arange(w[6], w[7])
        yield w, k, pc[k, 3] >> 24, pc[k + 1, 2] - pc[k, 2], pc[k, 0], hb.px[k].astype(np.int64)


def _ops(hb, k):
    return [(int(x) & 15, int(x) >> 4) for x in hb.ops[int(hb.pc[k, 2]):int(hb.pc[k + 1, 2])]]


def _is_del_read(hb, k, fl, nops):
    """The rare pass's deletion-read case: bases, D / N / P, bases and no other flag."""
    if nops != 3 or fl & ~(L.S2C_PF_X | L.S2C_PF_DASH | L.S2C_PF_XFEW):
        return False
    (a, _), (b, _), (c, _) = _ops(hb, k)
    bases, dash = (OP_M, OP_EQ, OP_X), (OP_D, OP_N, OP_P)
    return a in bases and b in dash and c in bases


def _check_plan(name, hb):
    S, X, F, D = L.S2C_PF_SIMPLE, L.S2C_PF_X, L.S2C_PF_XFEW, L.S2C_PF_DASH
    assert hb.info.n_dense > 0
    wins = list(_windows(hb))
    tiles = hb.tiles.astype(np.int64)
    if name == "xfew":
        assert len(wins) > 1
        n1 = n2 = before = after = past_take = last = 0
        for w, k, fl, nops, pos, px in wins:
            assert ((fl & S) != 0).all() and (nops == 1).all()
            T0, TL = 32 * (w[1] >> 5), 32 * ((w[2] - w[1] + 31) // 32)
            take = hb.pc[k, 3].astype(np.int64) & 0xFFFFFF
            for u in range(2):
                off = (px >> (16 * u)) & 0xFFFF
                has = ((fl & F) != 0) & (off != 0xFFFF)
                r = pos + off - T0
                before += int((has & (off < take) & (r < 0)).sum())
                after += int((has & (off < take) & (r >= TL)).sum())
                past_take += int((has & (off >= take)).sum())
                last += int((has & (off == take - 1)).sum())
            two = ((fl & F) != 0) & ((px >> 16) != 0xFFFF)
            n2 += int(two.sum())
            n1 += int((((fl & F) != 0) & ~two).sum())
            assert (((px & 0xFFFF) == 0) & ((fl & F) != 0)).any()
        assert n1 and n2 and before and after and past_take and last
    elif name.startswith("dash"):
        hit = deep = 0
        for w, k, fl, nops, pos, px in wins:
            one = (nops == 1) & ((fl & S) == 0) & ((fl & D) != 0)
            hit += int(one.sum())
            deep += int((one & ((hb.pc[k, 3].astype(np.int64) & 0xFFFFFF) == 320)).sum())
        assert hit and deep
    elif name.startswith("dels"):
        few = xq = cross = at = above = empty2 = 0
        for w, k, fl, nops, pos, px in wins:
            e = w[2]   # the tile's end
            for i in range(len(k)):
                if not _is_del_read(hb, int(k[i]), int(fl[i]), int(nops[i])):
                    continue
                assert not fl[i] & L.S2C_PF_LONG
                (_, l), (_, l1), (_, l2) = _ops(hb, int(k[i]))
                slen = int(hb.pc[int(k[i]), 3]) & 0xFFFFFF
                take = min(l, slen)
                few += bool(fl[i] & F)
                xq += bool(fl[i] & X and not fl[i] & F)
                cross += pos[i] + take < e < pos[i] + take + l1
                at += l1 == 150
                above += l1 == 151
                empty2 += l >= slen
        assert few and xq and cross and at and above and empty2
    elif name.startswith("many_dels"):
        # (the X-run queue of these two cases: test_dense_ext.test_x_run_queue_stays_inside_its_capacity)
        for w, k, fl, nops, pos, px in wins:
            assert all(_is_del_read(hb, int(k[i]), int(fl[i]), int(nops[i])) for i in range(len(k)))
            assert int(w[7] - w[6]) == len(k) and (hb.dpc[w[12]:w[12] + len(k), 1] >> 24 == fl).all()
    elif name == "big_window":
        npw = hb.dwin[:, 7].astype(np.int64) - hb.dwin[:, 6]
        assert (npw > BIG_WINDOW).any()
        late_rare = late_n = 0
        for w, k, fl, nops, pos, px in wins:
            late = np.arange(len(k)) >= BIG_WINDOW
            late_rare += int((late & ((fl & S) == 0)).sum())
            late_n += int((late & ((fl & S) != 0) & ((fl & F) != 0)).sum())
        assert late_rare and late_n
    elif name == "clips":
        rng_ = soft = 0
        for w, k, fl, nops, pos, px in wins:
            rng_ += int(((fl & L.S2C_PF_RANGE) != 0).sum())
            for i in np.nonzero((fl & S) == 0)[0]:
                soft += any(op == OP_S for op, _ in _ops(hb, int(k[i])))
        assert rng_ and soft
        assert any(op == OP_H for kk in range(int(hb.info.n_pieces)) for op, _ in _ops(hb, kk))
    elif name == "midword":
        dense = tiles[hb.dwin[:, 0].astype(np.int64)]
        assert ((dense[:, 1] - dense[:, 0]) % 32 != 0).any() and dense[:, 1].max() == 1483


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_its_path_and_model_equals_oracle(name):
    """Without a GPU: the plan holds the case's feature in a dense window, and the batch model
    writes the oracle's FASTA files."""
    _, opt, hb, want, ref = _case(name)
    _check_plan(name, hb)
    assert _files(hb, opt, *want) == ref["files"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_dense_walk_equals_batch_model_and_oracle(name):
    """The device pipeline == the batch model (stats, block offsets, body bytes; the second run
    sees no state of the first) and its FASTA files == the oracle's."""
    from sam2consensus_amd.engine import DeviceBatch, Workspace, needs_dense_layers
    _, opt, hb, want, ref = _case(name)
    _check_plan(name, hb)
    fill = opt.fill.encode()
    ws = Workspace(DeviceBatch(hb, dense_layers=needs_dense_layers(fill, False)), opt.thresholds, opt.min_depth, fill, False)
    for _ in range(2):
        ws.run()
        st, offs, out = ws.fetch()
        assert (st == want[0]).all()
        assert (offs == want[1]).all()
        assert out == want[2]
    assert _files(hb, opt, st, offs, out) == ref["files"]
