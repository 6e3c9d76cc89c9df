"""The pileup counters at the edges of their types, on stacks: n reads with the same POS on a
reference of their own, their SEQs written column by column, so the count of each of "-ACGNT" at
every position is known from the construction alone (no parser, no model).

  dense     k_tile_dense's bit-planes, packed bytes and 16-bit halves: coverage and counts of
            127 .. 255 (a byte's and a half's sign bits, and the last dense depth)
  single    the first depths past the dense class (256, 257, 255 + an insertion read) and
            k_tile's 8-bit lane counters: their flush rule and DPP pre-reduction, up to the
            largest stack the plan keeps in one work item, and one read more
  deep      u32 HBM sums and k_consensus at a coverage of 70,000
  long      65,535 .. 65,537 long pieces' runs over one position: the u16 halves of a work
            item's LDS histogram (the plan shares a tile's long list among its items)
  totals    k_consensus over running totals of 2^28 − 1 .. 2^28 + 1 and sums past 2^31: the
            vote's 32-bit fast path and the one beyond it

Every case is checked twice.  Without a GPU: the plan puts it on the path it is named for (tile
flags, n_dense, n_deep, work items, long-list entries — a case that misses its path fails), and
the batch model's counts == the construction == the oracle's, its files == the oracle's.  On the
GPU: the device's results == the batch model's (two runs), its counts == the construction, its
files == the oracle's."""
import builtins
import fractions
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import batch_model as bm
import s2c_oracle as o

from sam2consensus_amd import _lib as L
from sam2consensus_amd import batch

SYM = "-ACGNT"
THR = "0.25,0.5,0.75,1.0"
POS = 27          # the stacks' POS: their columns cross from the high halves of word 0 into word 1
LN = 320
PY_ORACLE_SPAN = 2000000   # positions the reads span (the Python oracle's work): above, the C restatement stands in
WV, GS = 4, 8     # k_tile: waves per work item, records per counting group


# ------------------------------------------------------------------ columns
def _col(n, **k):
    """A column's counts in "-ACGNT" order (d: '-'), summing to n."""
    c = [k.get(x, 0) for x in ("d", "A", "C", "G", "N", "T")]
    assert sum(c) == n and min(c) >= 0, (n, k)
    return c


def _spread(n, parts):
    return [n // parts + (i < n % parts) for i in range(parts)]


def _mixed_cols(n):
    """20 columns of n reads: (name, counts).  The named edges: an exact tie (n even), a largest
    count of cov/2 and of cov/2 + 1, three-way splits whose greater-sums are floor(cov/2) and
    floor(3·cov/4), and a six-way one whose largest count is floor(cov/4) — on t·cov for t =
    0.5, 0.75, 0.25 where cov divides, one read below it elsewhere."""
    h, q3, q = n // 2, 3 * n // 4, n // 4
    r = n - h
    s5 = _spread(n - q, 5)
    return [
        ("allA", _col(n, A=n)), ("allC", _col(n, C=n)), ("allG", _col(n, G=n)), ("allT", _col(n, T=n)),
        ("allN", _col(n, N=n)), ("all-", _col(n, d=n)),
        ("tieAC", _col(n, A=h, C=r)), ("tie-T", _col(n, d=h, T=r)),
        ("half", _col(n, T=h, G=r // 2, N=r - r // 2)),
        ("plus", _col(n, C=h + 1, A=(r - 1) // 2, N=r - 1 - (r - 1) // 2)),
        ("tri", _col(n, T=h, G=q3 - h, A=n - q3)),
        ("triX", _col(n, d=h, N=q3 - h, C=n - q3)),
        ("quart", _col(n, T=q, d=s5[0], A=s5[1], C=s5[2], G=s5[3], N=s5[4])),
        ("tieGN", _col(n, G=h, N=r)),
        ("tri-", _col(n, A=h, T=q3 - h, d=n - q3)),
        ("allT2", _col(n, T=n)), ("allA2", _col(n, A=n)),
        ("oneN", _col(n, N=1, C=n - 1)), ("one-", _col(n, d=1, G=n - 1)), ("allC2", _col(n, C=n)),
    ]


def _plain_cols(n):
    """Columns of ACGT only (reads the dense kernel takes on its lean path), one 'N' in one read."""
    h, q3 = n // 2, 3 * n // 4
    r = n - h
    return [
        ("allA", _col(n, A=n)), ("allC", _col(n, C=n)), ("allG", _col(n, G=n)), ("allT", _col(n, T=n)),
        ("tieAC", _col(n, A=h, C=r)), ("half", _col(n, T=h, G=r // 2, A=r - r // 2)),
        ("plus", _col(n, C=h + 1, A=(r - 1) // 2, G=r - 1 - (r - 1) // 2)),
        ("tri", _col(n, T=h, G=q3 - h, A=n - q3)), ("oneN", _col(n, N=1, A=n - 1)), ("allG2", _col(n, G=n)),
    ]


EDGE_COLS = ("half", "tri", "triX", "quart", "tri-")


def _letters(c, thr):
    return [o.AMB_TABLE[o.vote_closed(c, sum(c), t)] for t in thr]


def _on_edge(c, thr):
    """Whether one read more or fewer of some symbol changes a letter of column c (the oracle's
    closed form on the perturbed counts)."""
    base = _letters(c, thr)
    for i in range(6):
        for d in (1, -1):
            if c[i] + d >= 0:
                c2 = list(c)
                c2[i] += d
                if _letters(c2, thr) != base:
                    return True
    return False


# ------------------------------------------------------------------ two-decimal thresholds
@functools.lru_cache(maxsize=None)
def _twodec():
    """{kind: (k, cov, g)}: thresholds k/100 and coverages cov <= 255 with k·cov/100 = g an
    integer (exact, by Fraction) that a column's greater-sum can equal (g − 1, g and g + 1
    the column's strict majority, below cov), where the double product float(k/100)·cov lies below, on and above
    g.  The first of each kind in (cov, k) order, thresholds exact in binary left out."""
    found = {}
    for cov in range(4, 256):
        for k in range(1, 100):
            x = fractions.Fraction(k, 100) * cov
            if x.denominator != 1 or k in (25, 50, 75) or not (2 * x > cov + 2 and x + 1 < cov):
                continue
            g = int(x)
            f = float("0.%02d" % k) * float(cov)
            kind = "below" if f < g else "above" if f > g else "on"
            if kind not in found and k not in [v[0] for v in found.values()]:
                found[kind] = (k, cov, g)
    return found


def _twodec_thr():
    return ",".join("0.%02d" % v[0] for _, v in sorted(_twodec().items()))


# ------------------------------------------------------------------ SAM text and construction
class _Sam:
    def __init__(self):
        self.refs, self.reads, self.want, self.paths, self.span = [], [], {}, {}, 0

    def ref(self, name, ln, path):
        """A reference and the path its (single) tile must take: (kind, work items, long-list entries)."""
        self.refs.append((name, ln))
        self.want[name] = np.zeros((6, ln), dtype=np.int64)
        self.paths[name] = path
        return name

    def stack(self, ref, pos, cols, n, gap=None):
        """n reads at POS pos whose SEQ column j holds cols[j] of each symbol; gap (k, len, op,
        counted): `len op` after k bases (counted: its '-' are counted at those positions; not
        counted: a gap past the default -d, which drops the reads' '-' of SEQ too, :210)."""
        cols = [c for _, c in cols] if cols and isinstance(cols[0], tuple) else cols
        m = np.array([np.repeat(np.frombuffer(SYM.encode(), dtype="S1"), c) for c in cols])
        seqs = [row.tobytes().decode() for row in np.ascontiguousarray(m.T)]
        nc = len(cols)
        self.span += n * (nc + (gap[1] if gap is not None else 0))
        cigar = "%dM" % nc if gap is None else "%dM%d%s%dM" % (gap[0], gap[1], gap[2], nc - gap[0])
        self.reads += [(ref, pos, cigar, s) for s in seqs]
        w = self.want[ref]
        for j, c in enumerate(cols):
            p = pos - 1 + j + (gap[1] if gap is not None and j >= gap[0] else 0)
            w[:, p] += c
            if gap is not None and not gap[3]:
                w[0, p] -= c[0]
        if gap is not None and gap[3]:
            w[0, pos - 1 + gap[0]:pos - 1 + gap[0] + gap[1]] += n

    def read(self, ref, pos, cigar, seq, counted):
        """One more read: counted = [(offset from POS, symbol), ...]."""
        self.reads.append((ref, pos, cigar, seq))
        for off, ch in counted:
            self.want[ref][SYM.index(ch), pos - 1 + off] += 1

    def text(self):
        return "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in self.refs) + "".join(
            "r%d\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % ((i,) + r) for i, r in enumerate(self.reads))


DCOLS = [_col(1, A=1), _col(1, C=1), _col(1, G=1), _col(1, T=1)] * 2


def _dstack(s, n, path):
    """A stack of n reads 4M3D4M on its own reference: 3 run slots a read, '-' of a D run."""
    s.stack(s.ref("gd", LN, path), POS, [[n * x for x in c] for c in DCOLS], n, gap=(4, 3, "D", True))


def _dense(n, kind="stack"):
    """Dense tiles whose candidates per word are n <= 255 (mixed, plain) and 3·(n // 3) (gd)."""
    s = _Sam()
    if kind == "stack":
        s.stack(s.ref("mixed", LN, ("dense", 0, 0)), POS, _mixed_cols(n), n)
        s.stack(s.ref("plain", LN, ("dense", 0, 0)), POS, _plain_cols(n), n)
    elif kind == "lookback":
        # 55 reads starting in word 0, 200 in word 1 (the window looks back one word): 255
        # candidates for word 1, a coverage of 200 at the most
        assert n == 255
        s.ref("mixed", LN, ("dense", 0, 0))
        s.stack("mixed", 1, _mixed_cols(55) * 2, 55)
        s.stack("mixed", 41, _mixed_cols(200) * 2, 200)
    elif kind == "long":
        # 225 one-token reads and 5 long pieces 10M1100N10M: 225 + 2·15 = 255 (the long pieces'
        # slots are among the words' and the tile's long list); the dense tile walks the 5
        assert n == 255
        s.ref("mixed", 1400, ("dense", 0, 5))
        s.stack("mixed", POS, _mixed_cols(225), 225)
        s.stack("mixed", POS, _mixed_cols(5), 5, gap=(10, 1100, "N", False))
    _dstack(s, n // 3, ("dense", 0, 0))
    return s


def _single(n, ins=False):
    """The same stacks past the dense class: single-item k_tile tiles."""
    s = _Sam()
    s.stack(s.ref("mixed", LN, ("single", 1, 0)), POS, _mixed_cols(n), n)
    s.stack(s.ref("plain", LN, ("single", 1, 0)), POS, _plain_cols(n), n)
    if ins:   # (255 candidates, but an insertion key: nev != 0)
        for r in ("mixed", "plain"):
            s.read(r, 100, "2M1I2M", "ACGTA", [(0, "A"), (1, "C"), (2, "T"), (3, "A")])
    _dstack(s, n // 3, ("dense" if 3 * (n // 3) <= 255 else "single", int(3 * (n // 3) > 255), 0))
    return s


def _flush(n, items=1, width=20):
    """One stack of n reads of `width` bases (past the 20 columns: all T, A, C, G in turn; longer
    reads fill a layer's planes with fewer pieces, so a layer adds less to the lane counters)."""
    s = _Sam()
    cols = _mixed_cols(n) + [("pad", _col(n, **{"TACG"[j % 4]: n})) for j in range(width - 20)]
    path = ("dense", 0, 0) if n <= 255 else ("single" if items == 1 else "deep", items, 0)
    s.stack(s.ref("mixed", LN, path), POS, cols, n)
    return s


def _twodec_case(ins):
    """One stack per kind of _twodec: columns whose largest count is g − 1, g, g + 1 (the other
    symbol's greater-sum), cov reads; ins: an insertion read elsewhere sends the tiles to k_tile."""
    s = _Sam()
    for kind, (k, cov, g) in sorted(_twodec().items()):
        r = s.ref(kind, LN, ("single", 1, 0) if ins else ("dense", 0, 0))
        s.stack(r, POS, [_col(cov, T=g + d, C=cov - g - d) for d in (-1, 0, 1)]
                + [_col(cov, d=g + d, N=cov - g - d) for d in (-1, 0, 1)], cov)
        if ins:
            s.read(r, 100, "2M1I2M", "ACGTA", [(0, "A"), (1, "C"), (2, "T"), (3, "A")])
    return s


LONG_COLS = [_col(1, T=1), _col(1, C=1), _col(1, G=1), _col(1, A=1)] * 2
LONG_LN = 1300


def _long(n, shift, first="T"):
    """n reads 4M1100N4M (long pieces: the default -d drops their '-', so only base runs count)
    whose first column is bit 3 + shift of word 1, and 7 short reads 16 positions on: a carry out
    of a low u16 half lands in their counts."""
    s = _Sam()
    # (3·n long-list entries a tile, n > S2C_ITEM_RECS long pieces over a word: shares of <= 60,000)
    s.ref("g", LONG_LN, ("deep", -(-3 * n // bm.ITEM_RECS), 3 * n))
    cols = [[n * x for x in c] for c in LONG_COLS]
    cols[0] = _col(n, **{first: n})
    s.stack("g", 36 + shift, cols, n, gap=(4, 1100, "N", False))
    s.stack("g", 36 + shift + 16, [[7 * x for x in c] for c in LONG_COLS[1:5]], 7)
    return s


# ------------------------------------------------------------------ the flush rule, replayed
def _flush_replay(hb, t=0):
    """k_tile's flush rule on the layers of single-item tile t, as the kernel assigns them: wave
    wv counts layers wv, wv + 4, ...; a layer adds, to every lane's `acc`, its most records of a
    lane (lane g of G = 64 / nwp of a word takes every G-th record of the word's window) rounded
    to groups of 8 and a half group of 4.  Returns [(acc, add)]: acc at each flush and the add
    that forced it (0: the wave's last flush), and the largest acc + add that did not flush."""
    hb.ensure_layers(dense=True)
    row = hb.tiles[t].astype(np.int64)
    assert row[20] != bm.LY_MAIN and row[19] > 1
    nwp = 8
    while nwp * 32 < hb.info.tile_max:
        nwp *= 2
    G, K = 64 // nwp, int(hb.info.kwin)
    S0, W0, W1, lays = bm.layer_ranges(hb, t)
    pc = hb.pc.astype(np.int64)
    short = ((pc[:, 3] >> 24) & bm.PF_LONG) == 0
    nops = np.concatenate([[0], np.cumsum(np.where(short[:-1], pc[1:, 2] - pc[:-1, 2], 0))])
    flushes, kept = [], 0
    for wv in range(WV):
        acc = 0
        for l in range(wv, len(lays), WV):
            lo, hi = lays[l]
            recs = nops[hi] - nops[lo]
            nmx = max(-(-int(recs[max(W - K, S0) - S0:W - S0 + 1].sum()) // G) for W in range(W0, W1))
            add = GS * (nmx // GS + (nmx % GS > 4)) + (4 if 0 < nmx % GS <= 4 else 0)
            if acc + add > 255:
                flushes.append((acc, add))
                acc = 0
            else:
                kept = max(kept, acc + add)
            acc += add
        if acc:
            flushes.append((acc, 0))
    return flushes, kept


@functools.lru_cache(maxsize=None)
def _plan_of_flush(n):
    hb = batch.parse_text(_flush(n).text())
    return int(hb.info.n_deep), int((hb.items[:, 0] == 0).sum())


@functools.lru_cache(maxsize=None)
def _largest_single():
    """The largest stack the plan keeps in one work item (bisection on n_deep)."""
    lo, hi = 2049, 16384
    assert _plan_of_flush(lo)[0] == 0 and _plan_of_flush(hi)[0] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _plan_of_flush(mid)[0] == 0:
            lo = mid
        else:
            hi = mid
    return lo


# (reads, read length) at which the replay puts a wave's last flush on both sides of 64 (60 and 80)
# and of 128 (120 and 140), and an acc + add of 252 kept (adds are multiples of 4: the largest
# value the rule lets a lane counter reach below 255) and the next one flushed: asserted in
# test_flush_sizes_reach_their_edges
FLUSH_EDGES = ((1100, 224), (2020, 224), (4200, 160))
FLUSH_SIZES = [(n, 20) for n in sorted({256 * k + d for k in range(1, 9) for d in (-1, 0, 1)})] + list(FLUSH_EDGES)
FLUSH_IDS = ["%dx%d" % c for c in FLUSH_SIZES]


def _flush_key(n, width=20):
    return (n, 1, width)


# ------------------------------------------------------------------ the cases
ARGS = {
    "m1": ["-c", THR],
    "m128N": ["-c", THR, "-m", "128", "-f", "N"],
    "m255empty": ["-c", THR, "-m", "255", "--fill="],
    "m256": ["-c", THR, "-m", "256"],
    "m32767N": ["-c", THR, "-m", "32767", "-f", "N"],
    "m32768empty": ["-c", THR, "-m", "32768", "--fill="],
    "m40000": ["-c", THR, "-m", "40000"],
    "above1": ["--consensus-thresholds=1.5,2.0"],
    "outside": ["--consensus-thresholds=0.0,-0.5,0.5"],
    "twodec": None,   # (_twodec_thr())
}
DEEP_N = 70000
DEEP_ARGS = {"m%d" % m: ["-c", THR, "-m", str(m)] for m in (65535, 65536, 70000, 70001)}

CASES = {}
for _n in (127, 128, 129, 254, 255):
    CASES["dense%d" % _n] = (functools.partial(_dense, _n), ARGS)
CASES["dense255_lookback"] = (functools.partial(_dense, 255, "lookback"), ARGS)
CASES["dense255_long"] = (functools.partial(_dense, 255, "long"), ARGS)
CASES["dense_twodec"] = (functools.partial(_twodec_case, False), {"twodec": None})
CASES["single_twodec"] = (functools.partial(_twodec_case, True), {"twodec": None})
CASES["single256"] = (functools.partial(_single, 256), ARGS)
CASES["single257"] = (functools.partial(_single, 257), ARGS)
CASES["single255_ins"] = (functools.partial(_single, 255, True), ARGS)
CASES["deep70000"] = (functools.partial(_flush, DEEP_N, 18), DEEP_ARGS)
LONG_CASES = {"long%d_%s%s" % (n, "hi" if sh else "lo", "" if f == "T" else f): (n, sh, f)
              for n, sh, f in [(65535, 0, "T"), (65536, 0, "T"), (65537, 0, "T"), (65535, 16, "T"), (65536, 16, "T"),
                               (65537, 16, "T"), (65537, 0, "N")]}
for _name, _a in LONG_CASES.items():
    CASES[_name] = (functools.partial(_long, *_a), {"m1": ["-c", THR]})


def _argv(args_name, args):
    return ["--consensus-thresholds=" + _twodec_thr()] if args is None else args


@functools.lru_cache(maxsize=4)
def _built(name):
    """The case's construction, text and batch (the few last ones kept: the long cases' are large)."""
    s = (CASES[name][0] if name in CASES else functools.partial(_flush, *name))()
    sam = s.text()
    hb = batch.parse_text(sam, True, 150)
    return s, sam, hb


@functools.lru_cache(maxsize=None)
def _mc_bin():
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "build", "s2c_oracle_mc")


@functools.lru_cache(maxsize=2)
def _oracle_pileup(name):
    """The Python oracle's read pass on a case (the same for every argument set here: default -d)."""
    lines = o._lines(_built(name)[1])
    refs = o.read_header(lines)
    return (refs,) + o.pileup(lines, refs, o.parse_argv(["-i", "case.sam"]))


@functools.lru_cache(maxsize=2)
def _model_reads(name):
    return bm.model_reads(_built(name)[2])


def _oracle(name, s, sam, argv):
    """The oracle's {"status", "files"}: the Python one (run_case on the shared read pass), the C
    restatement for the large stacks."""
    if s.span <= PY_ORACLE_SPAN:
        opt = o.parse_argv(["-i", "case.sam"] + list(argv))
        assert opt.maxdel_active
        try:
            return {"status": "ok", "files": o.render(o.consensus(*_oracle_pileup(name), opt), opt)}
        except (KeyError, IndexError, ValueError, ZeroDivisionError, OverflowError) as e:
            return {"status": type(e).__name__, "files": {}}
    with tempfile.TemporaryDirectory() as td:
        p, out = os.path.join(td, "case.sam"), os.path.join(td, "out")
        with open(p, "w", encoding="latin-1", newline="") as fh:
            fh.write(sam)
        r = subprocess.run([_mc_bin(), "4", "-i", p, "-o", out] + list(argv), capture_output=True, text=True)
        assert "status: " in r.stdout, (r.returncode, r.stderr[-500:])
        status = r.stdout.split("status: ")[1].split()[0]
        files = {}
        if status == "ok" and os.path.isdir(out):
            for f in sorted(os.listdir(out)):
                with open(os.path.join(out, f), encoding="latin-1", newline="") as fh:
                    files[f] = fh.read()
        return {"status": status, "files": files}


@functools.lru_cache(maxsize=None)
def _expect(name, args_name):
    """(options, the batch model's (stats, offs, out), the oracle's result) of a case's argument set."""
    s, sam, hb = _built(name)
    argv = _argv(args_name, (CASES[name][1] if name in CASES else ARGS)[args_name])
    opt = o.parse_argv(["-i", "case.sam"] + argv)
    want = bm.model_pipeline(hb, opt.thresholds, opt.min_depth, opt.fill.encode(), reads=_model_reads(name))
    return opt, want, _oracle(name, s, sam, argv)


def _check_files(hb, opt, st, offs, out, ref):
    """The files of (stats, offs, out) == the oracle's, or its exception class."""
    from sam2consensus_amd.records import build_records, render
    if ref["status"] != "ok":
        with pytest.raises(getattr(builtins, ref["status"])):
            build_records(hb, opt.thresholds, "case", st, offs, out)
        return
    recs = build_records(hb, opt.thresholds, "case", st, offs, out)
    assert {n + "__case.fasta": render(r, 0).decode("latin-1") for n, r in recs.items()} == ref["files"]


def _check_path(s, hb):
    """Every tile that holds a reference's reads takes the path the case names (flags, work items,
    long-list entries); the other tiles are empty; n_dense, n_deep and the item count follow."""
    T = hb.tiles.astype(np.int64)
    items = hb.items.astype(np.int64)
    n_dense = n_deep = n_items = 0
    for r, (name, _) in enumerate(s.refs):
        kind, nit, nlong = s.paths[name]
        a = int(hb.ref_off[r])
        hit = False
        for t in np.nonzero(T[:, 2] == r)[0]:
            if not s.want[name][:, T[t, 0] - a:T[t, 1] - a].any() and not T[t, 11] - T[t, 10]:
                assert T[t, 3] in (0, L.S2C_TILE_DENSE), (name, t)   # (no read)
                n_dense += T[t, 3] == L.S2C_TILE_DENSE
                n_items += T[t, 3] == 0
                continue
            hit = True
            assert T[t, 3] == {"dense": L.S2C_TILE_DENSE, "single": 0, "deep": L.S2C_TILE_DEEP}[kind], (name, t, T[t, 3])
            assert int((items[:, 0] == t).sum()) == nit, (name, t, int((items[:, 0] == t).sum()))
            assert T[t, 11] - T[t, 10] == nlong, (name, t, T[t, 11] - T[t, 10])
            n_dense += kind == "dense"
            n_deep += kind == "deep"
            n_items += nit
        assert hit, name
    assert (hb.info.n_dense, hb.info.n_deep, hb.info.n_items) == (n_dense, n_deep, n_items)


def _check_counts(s, hb, counts):
    for r, (name, ln) in enumerate(s.refs):
        a = int(hb.ref_off[r])
        got = counts[:, a:a + ln].astype(np.int64)
        bad = np.nonzero((got != s.want[name]).any(axis=0))[0]
        assert not len(bad), "%s: first wrong position %d: %s, constructed %s" % (
            name, bad[0], got[:, bad[0]].tolist(), s.want[name][:, bad[0]].tolist())


# ------------------------------------------------------------------ totals at 2^28 and beyond
B28 = 1 << 28
SEED_AT = 100   # the first seeded position of reference "mixed" (no read covers it)


def _seed_targets():
    """Count totals "-ACGNT" on both sides of the vote's 32-bit fast path (every count and the
    coverage < 2^28) and where its sums pass 2^31: a lone symbol, three-way splits whose
    greater-sums are t·cov for t = 0.5 and 0.75 at cov = 2^28 and one read either side."""
    return [_col(B28 - 1, T=B28 - 1), _col(B28, T=B28), _col(B28 + 1, T=B28 + 1),
            _col(B28, T=B28 // 2, G=B28 // 4, A=B28 // 4), _col(B28 - 1, T=B28 // 2 - 1, G=B28 // 4, A=B28 // 4),
            _col(B28 + 1, T=B28 // 2 + 1, G=B28 // 4, A=B28 // 4),
            _col(B28, d=B28 // 2, N=B28 // 4, C=B28 // 4), _col(B28 - 1, d=B28 // 2, N=B28 // 4 - 1, C=B28 // 4),
            _col(8 * B28, d=4 * B28, N=2 * B28, C=2 * B28), _col(13 * B28, T=12 * B28, d=B28),
            _col(15 * B28 + 3, A=3 * B28, C=3 * B28 + 1, G=3 * B28 + 2, T=3 * B28, d=3 * B28)]


@functools.lru_cache(maxsize=None)
def _seeded():
    """The dense128 batch, running totals to add to its counts (the targets at positions no read
    covers; under the all-T column, 2^28 − 128 − 1: the batch's 128 reads bring it to 2^28 − 1;
    under the second, 2^28 − 128), and the totals."""
    s, sam, hb = _built("dense128")
    seed = np.zeros((6, int(hb.info.padded_len)), dtype=np.int64)
    a = int(hb.ref_off[0])
    for j, c in enumerate(_seed_targets()):
        seed[:, a + SEED_AT + j] = c
    names = [n for n, _ in _mixed_cols(128)]
    seed[5, a + POS - 1 + names.index("allT")] = B28 - 128 - 1
    seed[5, a + POS - 1 + names.index("allT2")] = B28 - 128
    total = seed.copy()
    total[:, a:a + LN] += s.want["mixed"]
    return hb, seed, total


SEED_ARGS = (("-c", THR), ("-c", THR, "-m", str(B28)), ("-c", THR, "-m", str(B28 + 1), "-f", "N"))


@functools.lru_cache(maxsize=None)
def _seeded_expect(args):
    hb, seed, _ = _seeded()
    opt = o.parse_argv(["-i", "case.sam"] + list(args))
    return opt, bm.model_pipeline(hb, opt.thresholds, opt.min_depth, opt.fill.encode(), counts_add=seed, reads=_model_reads("dense128"))


def test_seeded_totals_straddle_the_fast_path_and_model_equals_closed_form():
    """The seeded totals lie on both sides of 2^28 (counts and coverage) and past 2^31, their
    split columns on t·cov; the batch model's letters there == the oracle's closed form."""
    hb, seed, total = _seeded()
    thr = [float(x) for x in THR.split(",")]
    a = int(hb.ref_off[0])
    cov = total.sum(axis=0)
    assert {B28 - 1, B28, B28 + 1} <= set(cov.tolist()) and cov.max() >= 1 << 31 and cov.max() < 1 << 32
    assert sum(_on_edge(c, thr) for c in _seed_targets()) >= 5
    opt, (st, offs, out) = _seeded_expect(SEED_ARGS[0])
    body = out[int(offs[0]):int(offs[1])]   # (threshold 0, tile 0: reference "mixed", one char a position)
    assert len(body) == LN
    for p in list(range(SEED_AT, SEED_AT + len(_seed_targets()))) + [POS + 2, POS + 14]:
        c = [int(x) for x in total[:, a + p]]
        assert chr(body[p]) == o.AMB_TABLE[o.vote_closed(c, sum(c), thr[0])], p


@pytest.mark.gpu
@pytest.mark.parametrize("args", SEED_ARGS, ids=["m1", "m2p28", "m2p28plus1"])
def test_vote_of_totals_at_2p28_equals_model(args):
    """k_consensus over running totals (the streamed path: accumulate, vote_all) whose counts and
    coverage straddle 2^28 and whose sums pass 2^31 == the batch model, -m compared at 2^28."""
    import torch
    from sam2consensus_amd.engine import DeviceBatch, Workspace
    hb, seed, _ = _seeded()
    opt, want = _seeded_expect(args)
    db = DeviceBatch(hb, dense_layers=True)
    for _ in range(2):
        counts = torch.from_numpy(seed.astype(np.uint32).view(np.uint8).reshape(-1).copy()).to(db.device)
        ws = Workspace(db, opt.thresholds, opt.min_depth, opt.fill.encode(), counts=counts)
        ws.accumulate(keep_tables=True)
        ws.vote_all()
        st, offs, out = ws.fetch()
        assert (st == want[0]).all()
        assert (offs == want[1]).all()
        assert out == want[2]


# ------------------------------------------------------------------ CPU tier
def test_twodec_thresholds_lie_below_on_and_above():
    """The two-decimal set holds a threshold whose double product with a coverage lies below the
    integer it equals exactly, one on it and one above it (0.7 × 90 = 62.99999999999999 is a
    'below'), and the stacks built on them put a greater-sum on that integer."""
    f = _twodec()
    assert sorted(f) == ["above", "below", "on"]
    assert float("0.7") * 90.0 < 63 == fractions.Fraction(7, 10) * 90
    for kind, (k, cov, g) in f.items():
        t = float("0.%02d" % k)
        assert fractions.Fraction(k, 100) * cov == g and cov <= 255
        assert {"below": t * cov < g, "on": t * cov == g, "above": t * cov > g}[kind]
        # the second symbol's letter: in by the double product only where it lies above
        c = _col(cov, T=g, C=cov - g)
        assert (o.AMB_TABLE[o.vote_closed(c, cov, t)] == "Y") == (kind == "above")
        assert o.AMB_TABLE[o.vote_closed(_col(cov, T=g - 1, C=cov - g + 1), cov, t)] == "Y"
        assert o.AMB_TABLE[o.vote_closed(_col(cov, T=g + 1, C=cov - g - 1), cov, t)] == "T"


@pytest.mark.parametrize("n", [127, 128, 129, 254, 255, 256, 257, 2048, 16383, DEEP_N])
def test_edge_columns_sit_on_their_thresholds(n):
    """In every edge column one read more or fewer of some symbol changes a letter; an even stack
    holds exact ties and a largest count of exactly cov/2."""
    thr = [float(x) for x in THR.split(",")]
    cols = dict(_mixed_cols(n))
    for name in EDGE_COLS:
        assert _on_edge(cols[name], thr), (n, name, cols[name])
    for name in ("half", "tri"):
        assert _on_edge(dict(_plain_cols(n))[name], thr), (n, name)
    if n % 2 == 0:
        assert cols["tieAC"][1] == cols["tieAC"][2] == cols["half"][5] == n // 2
    assert max(cols["plus"]) == n // 2 + 1
    for c in list(cols.values()) + [c for _, c in _plain_cols(n)]:
        assert None not in _letters(c, thr)   # (no vote error: the files are compared)


@pytest.mark.parametrize("name", list(CASES))
def test_case_takes_its_path_and_model_equals_construction_and_oracle(name):
    """Without a GPU: the plan puts every stack on the path its case names; the batch model's
    counts == the construction == the oracle's read pass; its files == the oracle's per
    argument set (or the oracle's exception class)."""
    s, sam, hb = _built(name)
    _check_path(s, hb)
    if name == "dense255_lookback":   # 255 candidates, coverage 200
        assert int(hb.rs[2]) - int(hb.rs[0]) == 255 and hb.info.kwin == 1 and s.want["mixed"].sum(axis=0).max() == 200
    if name == "dense255_long":
        assert int(hb.rs[1]) + 15 == 255 and s.want["mixed"].sum(axis=0).max() == 230
    if name in LONG_CASES:
        T = hb.tiles.astype(np.int64)
        assert (T[:, 11] - T[:, 10] >= 65535 * 3).all() and (T[:, 19] == 1).all()
    _check_counts(s, hb, bm.model_counts(hb, _model_reads(name)[0]))
    if s.span <= PY_ORACLE_SPAN:
        oc = _oracle_pileup(name)[1]
        for r, _ in s.refs:
            assert (np.array(oc[r], dtype=np.int64).T == s.want[r]).all(), r
    for args_name in CASES[name][1]:
        opt, want, ref = _expect(name, args_name)
        assert ref["status"] == "ok" or args_name not in ("m1", "m128N", "above1", "twodec"), (args_name, ref["status"])
        _check_files(hb, opt, *want, ref)


@pytest.mark.parametrize("name", list(CASES) + [_flush_key(*c) for c in FLUSH_SIZES], ids=list(CASES) + FLUSH_IDS)
def test_every_item_keeps_its_u16_bound(name):
    """The plan's invariant (batch_model.check_items): what a work item adds to a position's u16
    halves — its layers' records and its share of the long list — is at most S2C_ITEM_RECS; the
    long cases' items are cut by it (65,535 runs and more over a position, shares of 49,152 to
    58,983 entries)."""
    s, sam, hb = _built(name)
    most = bm.check_items(hb)
    if name in LONG_CASES:
        assert 3 * LONG_CASES[name][0] // 4 - 1 <= most <= bm.ITEM_RECS, most


def test_largest_single_item_stack():
    """The bisection's result: n reads in one work item, n + 1 in several; not 16,384."""
    n = _largest_single()
    assert _plan_of_flush(n) == (0, 1) and _plan_of_flush(n + 1)[0] == 1 and _plan_of_flush(n + 1)[1] > 1
    assert 2049 < n < 16384
    assert bm.check_items(batch.parse_text(_flush(n).text())) == n   # (all its records over one word)
    assert bm.check_items(batch.parse_text(_flush(n + 1).text())) < n


def test_flush_sizes_reach_their_edges():
    """The replayed flush rule over the flush sizes: flushes with acc just below and at 64 and
    128 (the DPP pre-reductions' bounds), an acc + add of 255 kept and one past it flushed."""
    accs, kepts, forced = set(), set(), set()
    for n, width in FLUSH_SIZES + [(_largest_single(), 20)]:
        s, sam, hb = _built(_flush_key(n, width))
        _check_path(s, hb)
        if n == 255:
            continue   # (two layers: a wave counts one)
        fl, kept = _flush_replay(hb)
        accs |= {a for a, _ in fl}
        forced |= {(a, a + d) for a, d in fl if d}
        kepts.add(kept)
        if (n, width) in FLUSH_EDGES:
            edge = {0: {60, 80}, 1: {120, 140}, 2: {252}}[FLUSH_EDGES.index((n, width))]
            assert edge <= {a for a, _ in fl}, (n, width, fl)
    assert {32, 64, 128, 224} <= accs, sorted(accs)          # (the 20-base stacks' own)
    assert max(kepts) == 252 and (252, 280) in forced and (224, 256) in forced, (sorted(kepts), sorted(forced))


@pytest.mark.parametrize("n,width", FLUSH_SIZES, ids=FLUSH_IDS)
def test_flush_stack_model_equals_construction(n, width):
    """Without a GPU: a flush stack is one work item of k_tile (255: dense) and the batch model's
    counts == the construction."""
    s, sam, hb = _built(_flush_key(n, width))
    _check_path(s, hb)
    _check_counts(s, hb, bm.model_counts(hb))


# ------------------------------------------------------------------ GPU tier
def _workspace(hb, opt, counts=False):
    from sam2consensus_amd.engine import DeviceBatch, Workspace, needs_dense_layers
    fill = opt.fill.encode()
    return Workspace(DeviceBatch(hb, dense_layers=needs_dense_layers(fill, counts)), opt.thresholds, opt.min_depth, fill, counts)


def _run_twice(ws, want):
    for _ in range(2):
        ws.run()
        st, offs, out = ws.fetch()
        assert (st == want[0]).all()
        assert (offs == want[1]).all()
        assert out == want[2]
    return st, offs, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_model_construction_and_oracle(name):
    """Per argument set: the device pipeline == the batch model (stats, block offsets, body bytes;
    two runs) and its files == the oracle's; the counts-only pileup == the construction."""
    s, sam, hb = _built(name)
    _check_path(s, hb)
    _check_counts(s, hb, _workspace(hb, o.parse_argv(["-i", "case.sam"]), counts=True).pileup_counts())
    for args_name in CASES[name][1]:
        opt, want, ref = _expect(name, args_name)
        st, offs, out = _run_twice(_workspace(hb, opt), want)
        _check_files(hb, opt, st, offs, out, ref)


def _flush_gpu(n, width):
    s, sam, hb = _built(_flush_key(n, width))
    _check_path(s, hb)
    opt, want, ref = _expect(_flush_key(n, width), "m1")
    _check_counts(s, hb, _workspace(hb, opt, counts=True).pileup_counts())
    st, offs, out = _run_twice(_workspace(hb, opt), want)
    if s.span <= PY_ORACLE_SPAN:
        _check_files(hb, opt, st, offs, out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n,width", FLUSH_SIZES, ids=FLUSH_IDS)
def test_flush_stack_counts_and_letters(n, width):
    """k_tile's lane counters over its flush rule: counts == construction, letters == model."""
    _flush_gpu(n, width)


@pytest.mark.gpu
@pytest.mark.parametrize("more", [0, 1])
def test_largest_single_item_stack_counts_and_letters(more):
    """The largest stack of one work item, and one read more (several items: deep)."""
    n = _largest_single() + more
    _built.cache_clear()
    s = _flush(n, _plan_of_flush(n)[1])
    sam = s.text()
    hb = batch.parse_text(sam, True, 150)
    _check_path(s, hb)
    opt = o.parse_argv(["-i", "case.sam", "-c", THR])
    want = bm.model_pipeline(hb, opt.thresholds, opt.min_depth, opt.fill.encode())
    _check_counts(s, hb, _workspace(hb, opt, counts=True).pileup_counts())
    _run_twice(_workspace(hb, opt), want)
