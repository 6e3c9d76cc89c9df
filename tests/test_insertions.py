"""--insertions: the insertion motif tables (sam2consensus_amd/table.py, csrc/s2c_ins.hip).

Without a GPU: a literal file for a hand-written SAM, the model against a restatement (a dict
of dicts and sorted() with an explicit key) on every golden case, the numeric edges, the flags
and their refused combinations, the bindings.  On the GPU: the two kernels alone on hand-built
tile records, hash tables, long-event lists, planes and counts (empty tiles, slot layouts and
event orders, equal long events, motifs differing in their last base, the 16 / 17 seam, plane
offsets, a 300-base motif, N and -, ties, the digit steps, position 2047, cov 0 and cov < reads,
min_reads, 1,500 entries in a tile; the guards), the golden cases end to end, hand-written SAM
texts against the oracle, every tile kind against the batch model, a reused workspace, all five
tables at once, and the CLI process on a C1-sized file."""
import os

import numpy as np
import pytest

import batch_model as bm
from devmem import _ptr
import golden_io
import s2c_oracle as o
import test_table as tt

from sam2consensus_amd import table

CASES = tt.CASES
KAT = len(golden_io.load("kat"))
INS_HEADER = b"pos\tcov\treads\tlen\tmotif\n"
SYM = "-ACGNT"


# ---------------------------------------------------------------------------- expectations
def _grouped(ins_list, ln):
    """[(pos, motif, reads)] of an oracle insertion list: the events the device keeps (key in
    [0, LN), a non-empty motif), equal ones counted together."""
    d = {}
    for key, motif in ins_list:
        if 0 <= key < ln and motif:
            d[(key, motif)] = d.get((key, motif), 0) + 1
    return [(k, m, n) for (k, m), n in d.items()]


def _oracle_text(sam_text, args):
    """(refs, counts, inserts, prefix) of the oracle's two passes over a SAM text."""
    opt = o.parse_argv(["-i", "in.sam"] + list(args))
    lines = o._lines(sam_text)
    refs = o.read_header(lines)
    counts, inserts = o.pileup(lines, refs, opt)
    return refs, counts, inserts, opt.prefix


def _oracle_files(refs, counts, inserts, prefix, min_reads=1):
    """{file name: content}: one table per reference with Σcoverage > 0; and the entries."""
    out, entries = {}, []
    for r, ln in refs.items():
        cov = [sum(c) for c in counts[r]]
        if sum(cov) > 0:
            e = _grouped(inserts[r], ln)
            entries += [(x, cov[x[0]]) for x in e]
            out[r + "__" + prefix + ".insertions.tsv"] = (INS_HEADER + table.format_insertions(e, cov, 1, min_reads)).decode()
    return out, entries


class _Totals:
    """What the golden check must hold (the issue's floor): lines, reads > cov, non-ACGT."""

    def __init__(self):
        self.lines = self.above = self.other = self.cases = 0

    def add(self, entries):
        self.cases += bool(entries)
        for (pos, motif, reads), cov in entries:
            self.lines += 1
            self.above += reads > cov
            self.other += any(ch not in "ACGT" for ch in motif)

    def check(self):
        assert self.lines >= 700 and self.above >= 50 and self.other >= 40, vars(self)


# ---------------------------------------------------------------------------- CPU tier
HAND_SAM = ("@SQ\tSN:g1\tLN:12\n"
            "a\t0\tg1\t1\t60\t2M2I2M\t*\t0\t0\tACGTAC\t*\n"
            "b\t0\tg1\t1\t60\t2M2I2M\t*\t0\t0\tACGTAC\t*\n"
            "c\t0\tg1\t1\t60\t2M1I3M\t*\t0\t0\tACNTAC\t*\n"
            "d\t0\tg1\t1\t60\t2M2I2M\t*\t0\t0\tACGAAC\t*\n"
            "e\t0\tg1\t3\t60\t2M3I\t*\t0\t0\tTACC-\t*\n")
HAND_TABLE = ("pos\tcov\treads\tlen\tmotif\n"
              "3\t5\t2\t2\tGT\n"
              "3\t5\t1\t1\tN\n"
              "3\t5\t1\t2\tGA\n"
              "5\t1\t1\t3\tCC-\n")


def test_constants():
    assert (table.INS_HEADER, table.INS_SUFFIX) == (INS_HEADER, b".insertions.tsv")


def test_hand_written_literal():
    """The key is the reference's start_ref at the I token (the bases consumed before it), printed
    plus 1; reads falling, then length, then the motif; a read ending in I keys the position
    after its last base, which it does not cover."""
    refs, counts, inserts, prefix = _oracle_text(HAND_SAM, [])
    files, entries = _oracle_files(refs, counts, inserts, prefix)
    assert files == {"g1__in.insertions.tsv": HAND_TABLE}
    assert sorted(e[0] for e in entries) == [(2, "GA", 1), (2, "GT", 2), (2, "N", 1), (4, "CC-", 1)]
    assert _oracle_files(refs, counts, inserts, prefix, 2)[0] == {
        "g1__in.insertions.tsv": "pos\tcov\treads\tlen\tmotif\n3\t5\t2\t2\tGT\n"}
    assert _oracle_files(refs, counts, inserts, prefix, 3)[0] == {"g1__in.insertions.tsv": INS_HEADER.decode()}


def test_order_literal():
    cov = [7] * 10
    e = [(3, "T", 2), (3, "AC", 2), (3, "-", 2), (3, "N", 2), (3, "A", 2), (3, "G", 5), (1, "TTTT", 1), (3, "AA", 2),
         (3, "A-", 2), (3, "AN", 2)]
    want = [(1, "TTTT", 1), (3, "G", 5), (3, "-", 2), (3, "A", 2), (3, "N", 2), (3, "T", 2), (3, "A-", 2), (3, "AA", 2),
            (3, "AC", 2), (3, "AN", 2)]
    assert table.format_insertions(e, cov) == "".join(
        "%d\t7\t%d\t%d\t%s\n" % (p + 1, n, len(m), m) for p, m, n in want).encode()
    assert table.format_insertions(e[::-1], cov) == table.format_insertions(e, cov)
    assert table.format_insertions([], cov) == b""


def test_numeric_edges():
    assert table.format_insertions([(0, "A", 4294967295)], [0], 9999999999) == b"9999999999\t0\t4294967295\t1\tA\n"
    assert table.format_insertions([(1, "AC-N", 3)], [5, 25769803770]) == b"2\t25769803770\t3\t4\tAC-N\n"
    assert table.format_insertions([(0, "A", 2), (0, "C", 3)], [1], 1, 3) == b"1\t1\t3\t1\tC\n"
    assert table.format_insertions([(0, b"AT", 1)], [1]) == b"1\t1\t1\t2\tAT\n"
    for bad in ("", "a", "AX"):
        with pytest.raises(ValueError):
            table.format_insertions([(0, bad, 1)], [1])


def _restated(e, cov, min_reads=1):
    """The order and format restated: {pos: {motif: reads}}, sorted() with an explicit key."""
    by_pos = {}
    for pos, motif, reads in e:
        by_pos.setdefault(pos, {})[motif] = reads
    lines = []
    for pos in sorted(by_pos):
        d = by_pos[pos]
        for motif in sorted(d, key=lambda m: (-d[m], len(m), tuple(SYM.index(ch) for ch in m))):
            if d[motif] >= min_reads:
                lines.append("\t".join([str(pos + 1), str(cov[pos]), str(d[motif]), str(len(motif)), motif]) + "\n")
    return "".join(lines).encode()


def test_model_against_the_restatement_on_every_ok_case():
    tot = _Totals()
    longest = multi = 0
    for idx, case in enumerate(CASES):
        if case["status"] != "ok":
            continue
        refs, counts, inserts, _ = _oracle_text(case["sam"], case["args"])
        entries = []
        for r, ln in refs.items():
            cov = [sum(c) for c in counts[r]]
            e = _grouped(inserts[r], ln)
            for mr in (1, 2):
                assert table.format_insertions(e, cov, 1, mr) == _restated(e, cov, mr), (case["name"], r)
            if sum(cov) > 0:
                entries += [(x, cov[x[0]]) for x in e]
        tot.add(entries)
        longest = max([longest] + [len(m) for (_, m, _), _ in entries])
        multi += sum(n > 1 for (_, _, n), _ in entries)
    tot.check()
    assert tot.cases >= 400 and longest >= 2 and multi >= 1


def test_parser_has_the_flags(capsys):
    from sam2consensus_amd.cli import build_parser, insertions_of
    p = build_parser()
    a = p.parse_args(["-i", "x.sam"])
    assert a.insertions is False and a.min_ins_reads is None and insertions_of(p, a) is None
    assert insertions_of(p, p.parse_args(["-i", "x.sam", "--insertions"])) == 1
    assert insertions_of(p, p.parse_args(["-i", "x.sam", "--insertions", "--min-ins-reads", "3"])) == 3
    a = p.parse_args(["-i", "x.sam", "--insertions", "--counts", "--depth", "--variants", "--lowcov"])
    assert a.insertions and a.counts and a.depth and a.variants and a.lowcov
    for argv in (["--min-ins-reads", "2"], ["--insertions", "--min-ins-reads", "0"], ["--insertions", "--min-ins-reads", "-1"]):
        with pytest.raises(SystemExit) as e:
            insertions_of(p, p.parse_args(["-i", "x.sam"] + argv))
        assert e.value.code == 2 and "--min-ins-reads" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["-i", "x.sam", "--insertions", "--min-ins-reads", "x"])
    assert "--insertions" in p.format_help() and "--min-ins-reads" in p.format_help()


@pytest.mark.parametrize("env,extra", [({"WORLD_SIZE": "2"}, []), ({"S2C_STREAM": "1M"}, []), ({}, ["--min-ins-reads", "0"])],
                         ids=["world2", "stream", "min0"])
def test_refused_combinations(env, extra, tmp_path, monkeypatch, capsys):
    """The argparse error, before a folder is made or a device touched."""
    from sam2consensus_amd.cli import main
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2C_STREAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sam = tmp_path / "in.sam"
    sam.write_text("@SQ\tSN:g1\tLN:10\nr\t0\tg1\t1\t60\t4M\t*\t0\t0\tAATG\t*\n")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(["-i", str(sam), "-o", str(tmp_path / "out"), "--insertions"] + extra)
    assert e.value.code == 2
    assert ("--min-ins-reads" if extra else "--insertions") in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == ["in.sam"]


def test_min_ins_reads_needs_insertions(tmp_path, monkeypatch, capsys):
    from sam2consensus_amd.cli import main
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2C_STREAM"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(["-i", "in.sam", "-o", str(tmp_path / "out"), "--min-ins-reads", "2"])
    assert e.value.code == 2 and "--min-ins-reads needs --insertions" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []


def test_ins_symbols_declared_and_bound():
    from sam2consensus_amd import _lib
    lib = _lib.lib
    assert {"s2c_ins_len", "s2c_ins_write"} <= set(_lib.EXPORTS)
    assert lib.s2c_abi_version() == 14
    assert [len(getattr(lib, f).argtypes) for f in ("s2c_ins_len", "s2c_ins_write")] == [17, 15]
    OK, ARG = _lib.S2C_OK, _lib.S2C_ERR_ARG   # (argument errors need no device)
    ln = lambda nt=0, nb=0, nl=0, nq=0, pl=16, mr=1: lib.s2c_ins_len(  # noqa: E731
        None, nt, None, nb, None, nl, None, None, None, nq, None, pl, None, mr, None, None, None)
    wr = lambda nt=0, nb=0, nl=0, nq=0, pl=16, dl=0: lib.s2c_ins_write(  # noqa: E731
        None, nt, nb, nl, None, None, nq, None, pl, None, None, None, None, dl, None)
    assert ln() == OK and wr() == OK
    assert ln(nt=-1) == ARG and ln(nb=-1) == ARG and ln(nl=-1) == ARG and ln(nq=-1) == ARG and ln(pl=-1) == ARG
    assert ln(mr=0) == ARG and ln(mr=2 ** 32) == ARG and ln(nb=2 ** 32) == ARG and ln(nt=1) == ARG
    assert wr(nt=-1) == ARG and wr(nb=-1) == ARG and wr(nl=2 ** 32) == ARG and wr(dl=-1) == ARG and wr(nt=1) == ARG


# ---------------------------------------------------------------------------- GPU tier: the kernels
CODE_BITS = {"A": (0, 0, 0), "C": (1, 0, 0), "G": (0, 1, 0), "T": (1, 1, 0), "N": (0, 0, 1), "-": (1, 0, 1)}   # p0, p1, x


class Scene:
    """Hand-built inputs of the kernels.  A tile: dict(a, n, p0, short=[(pos, motif, reads)],
    long=[(pos, motif, q % 32)] (one event each)).  `slots` / `order` seed the hash slots the
    short entries land in and the order of the long events."""

    def __init__(self, tiles, padded, cov=None, slots=0, order=0, ilong_n=None):
        self.tiles, self.padded = tiles, padded
        nt = len(tiles)
        rng_s, rng_o = np.random.default_rng(1000 + slots), np.random.default_rng(2000 + order)
        bases = []          # the planes' bases, a char each ('A' where nothing was put)
        rec = np.zeros((nt, 24), dtype=np.uint32)
        ibkt, ilong = [], []
        self.ilong_n = np.zeros(max(nt, 1), dtype=np.uint32)
        for t, T in enumerate(tiles):
            sh, lg = T.get("short", []), T.get("long", [])
            raw_s, raw_l = T.get("raw_short", []), T.get("raw_long", [])   # (garbage: slots and events as given)
            ns = len(sh) + len(raw_s)
            bcap = 0 if not ns else 1 << int(np.ceil(np.log2(2 * ns)))
            tab = np.zeros((bcap, 4), dtype=np.uint32)
            perm = rng_s.permutation(bcap)
            for slot, row in zip(perm[len(sh):ns], raw_s):
                tab[slot] = row
            for slot, (pos, motif, reads) in zip(perm[:len(sh)], sh):
                assert 1 <= len(motif) <= 16 and pos < 2048
                key = pos | len(motif) << 11
                for c, ch in enumerate(motif):
                    key |= SYM.index(ch) << (16 + 3 * c)
                tab[slot] = (key & 0xFFFFFFFF, key >> 32, reads, 0)
            ev = []
            for pos, motif, align in lg:
                while len(bases) % 32 != align:
                    bases.append("ACGT"[len(bases) % 4])
                ev.append((pos, len(motif), len(bases) & 0xFFFFFFFF, len(bases) >> 32))
                bases += list(motif)
            ev += [tuple(r) for r in raw_l]
            ev = [ev[k] for k in rng_o.permutation(len(ev))]
            rec[t, :8] = (T["a"], T["a"] + T["n"], 0, 0, len(ibkt), bcap, len(ilong), len(ev))
            ibkt += tab.tolist()
            ilong += ev
            self.ilong_n[t] = len(ev)
        if ilong_n:
            for t, v in ilong_n.items():
                self.ilong_n[t] = v
        self.n_bkt, self.n_lng = len(ibkt), len(ilong)
        self.ibkt = np.array(ibkt, dtype=np.uint32).reshape(-1, 4)
        self.ilong = np.array(ilong, dtype=np.uint32).reshape(-1, 4)
        self.rec = rec
        nq = (len(bases) + 31) // 32 + 1
        self.n_qwords = nq
        self.bq, self.bx = np.zeros((nq, 2), dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
        for q, ch in enumerate(bases):
            p0, p1, x = CODE_BITS[ch]
            self.bq[q >> 5, 0] |= np.uint32(p0 << (q & 31))
            self.bq[q >> 5, 1] |= np.uint32(p1 << (q & 31))
            self.bx[q >> 5] |= np.uint32(x << (q & 31))
        self.counts = np.zeros((6, padded), dtype=np.uint32) if cov is None else cov
        self.blocks = np.array([(T["a"], T["a"] + T["n"], T["p0"]) for T in tiles], dtype=np.int64).reshape(-1, 3)

    def want(self, min_reads=1, blocks=None):
        """The model's text per tile."""
        cov = self.counts.astype(np.uint64).sum(axis=0)
        out = []
        for t, T in enumerate(self.tiles):
            a, b, p0 = (int(v) for v in (self.blocks if blocks is None else blocks)[t])
            d = {}
            for pos, motif, reads in T.get("short", []):
                d[(pos, motif)] = reads
            for pos, motif, _ in T.get("long", []):
                d[(pos, motif)] = d.get((pos, motif), 0) + 1
            ok = 0 <= a <= b <= self.padded and 0 <= p0 <= 10 ** 10 - (b - a)
            e = [(pos, m, n) for (pos, m), n in d.items() if pos < b - a] if ok else []
            out.append(table.format_insertions(e, [int(v) for v in cov[a:b]] if ok else [], p0, min_reads))
        return out


def _u32(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    if a.size < 4:
        a = np.concatenate([a, np.zeros(4 - a.size, dtype=np.uint32)])
    return torch.from_numpy(a.view(np.int32)).cuda()


def run_kernels(sc, min_reads=1, blocks=None, offs=None, dst_len=None, shift=0, n_bkt=None, n_lng=None):
    """(lens, dst bytes with 64 guard bytes behind, offs): s2c_ins_len, the prefix sum,
    s2c_ins_write; the four tables are bit-identical after both calls."""
    import torch
    from sam2consensus_amd import _lib
    lib = _lib.lib
    import ctypes as C
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nt = len(sc.tiles)
    ins = {k: _u32(getattr(sc, k)) for k in ("rec", "ibkt", "ilong", "ilong_n", "bq", "bx", "counts")}
    before = {k: v.clone() for k, v in ins.items()}
    b = tt._dev_i64(sc.blocks if blocks is None else blocks)
    nb, nl = sc.n_bkt if n_bkt is None else n_bkt, sc.n_lng if n_lng is None else n_lng
    scratch = torch.full((max(32 * (sc.n_bkt + sc.n_lng), 16) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    lens = torch.full((nt,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.s2c_ins_len(_ptr(ins["rec"]), nt, _ptr(ins["ibkt"]), nb, _ptr(ins["ilong"]), nl, _ptr(ins["ilong_n"]),
                               _ptr(ins["bq"]), _ptr(ins["bx"]), sc.n_qwords, _ptr(ins["counts"]), sc.padded, _ptr(b),
                               min_reads, _ptr(scratch), _ptr(lens), st))
    lens = lens.cpu().numpy()
    assert scratch[-64:].cpu().numpy().tobytes() == b"\xEE" * 64
    if offs is None:
        offs = np.concatenate([[0], np.cumsum(lens)]) + shift
    total = int(offs[-1]) if dst_len is None else dst_len
    dst = torch.full((max(total, int(np.max(offs)), 0) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    f = tt._dev_i64(offs)
    _lib.check(lib.s2c_ins_write(_ptr(ins["rec"]), nt, nb, nl, _ptr(ins["bq"]), _ptr(ins["bx"]), sc.n_qwords,
                                 _ptr(ins["counts"]), sc.padded, _ptr(b), _ptr(scratch), _ptr(f), _ptr(dst), total, st))
    torch.cuda.synchronize()
    for k in ins:
        assert torch.equal(ins[k], before[k]), k
    return lens, dst.cpu().numpy().tobytes(), offs


def check_scene(sc, min_reads=1, shift=0):
    want = sc.want(min_reads)
    lens, got, offs = run_kernels(sc, min_reads, shift=shift)
    assert lens.tolist() == [len(w) for w in want], [(t, int(lens[t]), len(want[t])) for t in range(len(want)) if lens[t] != len(want[t])][:5]
    total = int(offs[-1])
    assert got[:shift] == b"\xEE" * shift and got[total:] == b"\xEE" * 64
    for t, w in enumerate(want):
        assert got[offs[t]:offs[t + 1]] == w, (t, tt._first_diff(got[offs[t]:offs[t + 1]], w))
    return b"".join(want)


M20 = "ACGTACGTACGTACGTACGA"
M300 = "".join("ACGTN-"[k] for k in np.random.default_rng(3).integers(0, 6, size=300))
PAD_A = 64 + 64 + 64 + 2048 + 64 + 64   # the main scene's positions
RICH = dict(a=192, n=2048, p0=1, short=[
    (5, "AC", 3),                                    # short beside the long motifs of position 5
    (7, "ACGTACGTACGTACGT", 2),                      # 16 bases, reads 2: before the 17-base motif with reads 2
    (9, "A", 4), (9, "C", 4), (9, "-", 4), (9, "N", 4), (9, "T", 4), (9, "AA", 4), (9, "G", 7),   # ties in reads
    (20, "A", 9), (20, "C", 10), (21, "A", 99), (21, "C", 100), (22, "A", 999), (22, "C", 1000),
    (23, "N-", 4294967295), (30, "T", 5), (31, "T", 5), (2047, "GG", 1), (0, "T", 1), (40, "-N-N", 2), (41, "ACGTN-ACGTN-ACGT", 1),
], long=[
    (5, M20, 3), (5, M20, 17), (5, M20, 31),         # three equal events → reads 3
    (5, M20[:-1] + "C", 5),                          # differs from them in the last base alone
    (6, M20[:-1] + "T", 9), (6, M20[:-1] + "G", 11),  # equal reads: ordered by the last base
    (7, "ACGTACGTACGTACGTA", 0), (7, "ACGTACGTACGTACGTA", 1),
    (8, "T" * 17, 0), (8, "G" * 18, 31),             # plane offsets 0 and 31
    (8, "ACGTTGCA" * 5, 30),                         # 40 bases from offset 30: three plane words
    (50, M300, 13),
    (51, "N" * 17 + "-" * 3 + "ACGT", 2), (51, "N" * 17 + "-" * 3 + "ACGT", 29), (51, "-" * 20, 7),
    (2047, "C" * 33, 31), (2047, "C" * 32 + "A", 0),
])


def _main_tiles():
    return [dict(a=0, n=64, p0=1), dict(a=64, n=64, p0=17, short=[(63, "ACG", 1)]), dict(a=128, n=64, p0=1), RICH,
            dict(a=2240, n=64, p0=9999999936, short=[(63, "A", 1)], long=[(63, "A" * 17, 0)]), dict(a=2304, n=64, p0=1)]


def _main_cov():
    c = np.zeros((6, PAD_A), dtype=np.uint32)
    c[1, 192:192 + 2048] = 50
    c[:, 192 + 23] = 4294967295          # coverage 25769803770
    c[:, 192 + 30] = 0                   # cov 0
    c[2, 192 + 31] = 4
    c[1, 192 + 31] = 0                   # cov 4 < reads 5
    c[3, 2240 + 63] = 7
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("min_reads", [1, 2, 3])
def test_kernels_on_the_main_scene(min_reads):
    """Empty tiles, a tile of one entry, a tile between two empty ones and the rich tile, in
    two hash slot layouts and two orders of the long events: the model's bytes, and the same
    bytes from every layout."""
    texts = set()
    for k, (slots, order) in enumerate(((0, 0), (1, 1), (0, 1))):
        sc = Scene(_main_tiles(), PAD_A, _main_cov(), slots, order)
        texts.add(check_scene(sc, min_reads, shift=k))
    assert len(texts) == 1
    text = texts.pop()
    if min_reads == 1:
        assert sc.want()[0] == b"" and sc.want()[2] == b"" and sc.want()[1] == b"80\t0\t1\t3\tACG\n"
        assert (b"6\t50\t3\t2\tAC\n6\t50\t3\t20\t" + M20.encode() + b"\n6\t50\t1\t20\t" + M20[:-1].encode() + b"C\n") in text
        assert (M20[:-1].encode() + b"G\n7\t50\t1\t20\t" + M20[:-1].encode() + b"T\n") in text
        assert b"8\t50\t2\t16\tACGTACGTACGTACGT\n8\t50\t2\t17\tACGTACGTACGTACGTA\n" in text
        assert b"9\t50\t1\t17\t" + b"T" * 17 + b"\n9\t50\t1\t18\t" + b"G" * 18 + b"\n9\t50\t1\t40\t" + b"ACGTTGCA" * 5 + b"\n" in text
        assert b"10\t50\t7\t1\tG\n10\t50\t4\t1\t-\n10\t50\t4\t1\tA\n10\t50\t4\t1\tC\n10\t50\t4\t1\tN\n10\t50\t4\t1\tT\n10\t50\t4\t2\tAA\n" in text
        assert b"21\t50\t10\t1\tC\n21\t50\t9\t1\tA\n22\t50\t100\t1\tC\n22\t50\t99\t1\tA\n23\t50\t1000\t1\tC\n23\t50\t999\t1\tA\n" in text
        assert b"24\t25769803770\t4294967295\t2\tN-\n" in text and b"31\t0\t5\t1\tT\n32\t4\t5\t1\tT\n" in text
        assert b"51\t50\t1\t300\t" + M300.encode() + b"\n" in text
        assert b"52\t50\t2\t24\t" + b"N" * 17 + b"---ACGT\n52\t50\t1\t20\t" + b"-" * 20 + b"\n" in text
        assert b"2048\t50\t1\t2\tGG\n2048\t50\t1\t33\t" + b"C" * 32 + b"A\n2048\t50\t1\t33\t" + b"C" * 33 + b"\n" in text
        assert b"9999999999\t7\t1\t1\tA\n9999999999\t7\t1\t17\t" + b"A" * 17 + b"\n" in text
    assert all(int(ln.split(b"\t")[2]) >= min_reads for ln in text.split(b"\n")[:-1])
    if min_reads == 3:
        assert b"6\t50\t3\t2\tAC\n6\t50\t3\t20\t" + M20.encode() + b"\n7\t" not in text and b"6\t50\t3\t20\t" in text
        assert b"\n8\t" not in text and b"\n10\t50\t4\t2\tAA\n21\t50\t10\t1\tC\n" in text


def _big_tile():
    """1,500 distinct entries in one tile: 600 at position 100 (more than a workgroup's 256
    lanes in ONE bucket: every lane ranks its entry against the whole bucket in a loop), 300
    long events of 150 distinct 17-base motifs at position 101, the rest over the positions."""
    rng = np.random.default_rng(7)
    short, seen = [], set()
    while len(short) < 600:
        m = "".join(SYM[k] for k in rng.integers(0, 6, size=int(rng.integers(1, 6))))
        if m not in seen:
            seen.add(m)
            short.append((100, m, int(rng.integers(1, 4))))
    for k in range(750):
        short.append((200 + k, "ACGT"[k % 4] * (1 + k % 16), 1 + k % 3))
    lg = []
    for k in range(150):
        m = "".join(SYM[(k // 6 ** j) % 6] for j in range(4)) + "ACGTACGTACGTA"
        lg += [(101, m, int(rng.integers(0, 32)))] * (1 + (k % 3 == 0) * 2)
    return dict(a=64, n=2048, p0=1, short=short, long=lg)


@pytest.mark.gpu
@pytest.mark.parametrize("min_reads", [1, 2])
def test_kernels_on_a_tile_of_1500_entries(min_reads):
    """More entries than a workgroup has lanes.  The kernels hold no entry in LDS — they bucket
    the entries by position in the HBM scratch and rank each inside its bucket — so there is no
    LDS sort whose capacity could be passed and this tile takes the one path every tile takes,
    with 600 entries in one bucket and 250 events grouped into 150 entries in the next."""
    T = _big_tile()
    assert len({(p, m) for p, m, _ in T["short"]} | {(p, m) for p, m, _ in T["long"]}) == 1500
    cov = np.zeros((6, 64 + 2048 + 64), dtype=np.uint32)
    cov[5, 64:64 + 2048] = 1234
    texts = {check_scene(Scene([dict(a=0, n=64, p0=1), T], 64 + 2048 + 64, cov, s, s), min_reads) for s in (0, 1)}
    assert len(texts) == 1
    assert texts.pop().count(b"\n") == (1500 if min_reads == 1 else sum(
        n >= 2 for _, _, n in T["short"]) + sum(k % 3 == 0 for k in range(150)))


@pytest.mark.gpu
def test_guards():
    """Invalid blocks and tile records past the tables get lens = 0 and no byte; garbage in the
    tables is not listed and ilong_n is clamped to lcap; ranges of offs that do not match the
    lengths cut or pad the text; the guard bytes around dst stay."""
    tiles = _main_tiles()
    cov = _main_cov()
    sc = Scene(tiles, PAD_A, cov)
    good = sc.want()
    bad_blocks = sc.blocks.copy()
    bad_blocks[1] = (64, PAD_A + 1, 17)            # b > padded_len
    bad_blocks[3] = (192, 191, 1)                  # b < a
    bad_blocks[4] = (2240, 2304, 10 ** 10 - 63)    # a printed position of 11 digits
    lens, got, offs = run_kernels(sc, blocks=bad_blocks, shift=3)
    assert lens.tolist() == [0] * 6
    assert got == b"\xEE" * len(got)
    ok_blocks = sc.blocks.copy()
    ok_blocks[3] = (192, 192 + 24, 1)              # the block ends inside the tile: positions >= 24 are not listed
    ok_blocks[4] = (2240, 2240, 1)                 # b == a: a reference without coverage
    lens, got, offs = run_kernels(sc, blocks=ok_blocks)
    want = sc.want(blocks=ok_blocks)
    assert want[4] == b"" and want[3] and want[3] != good[3] and want[3].endswith(b"24\t25769803770\t4294967295\t2\tN-\n")
    assert lens.tolist() == [len(w) for w in want] and got[:int(offs[-1])] == b"".join(want)
    # tile records reaching past n_bkt / n_lng: those tiles are skipped, the others unchanged
    lens, got, offs = run_kernels(sc, n_bkt=sc.n_bkt - 1, n_lng=sc.n_lng)
    assert lens.tolist() == [len(w) for w in good[:4]] + [0, len(good[5])]
    lens, got, offs = run_kernels(sc, n_bkt=sc.n_bkt, n_lng=sc.n_lng - 1)
    assert lens.tolist() == [len(w) for w in good[:4]] + [0, len(good[5])]
    assert got[:int(offs[-1])] == b"".join(good[:4])
    # garbage: ilong_n far above lcap, a long event outside the planes, one with length 0, a
    # position past the tile, a slot with a length of 0 and one of 17, a slot with count 0
    sc2 = Scene(tiles, PAD_A, cov, ilong_n={3: 0xFFFFFFF0, 4: 0xFFFFFFFF})
    assert check_scene(sc2) == b"".join(good)
    junk = dict(RICH, raw_long=[(5, 20, 0xFFFFFF00, 0), (5, 20, 0, 0x10000), (5, 0, 0, 0), (2048, 20, 0, 0), (7, 1 << 24, 0, 0),
                                (0xFFFFFFFF, 20, 0, 0)],
                raw_short=[(9 | 0 << 11, 1, 5, 0), (9 | 17 << 11, 0, 5, 0), (9 | 1 << 11 | 1 << 16, 0, 0, 0), (0, 1 << 16, 5, 0)])
    for seed in (0, 1):
        sc3 = Scene(tiles[:3] + [junk] + tiles[4:], PAD_A, cov, seed, seed)
        assert sc3.n_lng == sc.n_lng + 6 and sc3.n_bkt >= sc.n_bkt
        assert check_scene(sc3) == b"".join(good)
    # offs that do not match: a range 7 bytes short, one 5 bytes long, one that is none
    room = [len(good[0]), len(good[1]) + 5, 0, len(good[3]) - 7, len(good[4]), 0]
    offs = np.concatenate([[0], np.cumsum(room)]) + 100
    total = int(offs[-1])
    lens, got, _ = run_kernels(sc, offs=offs, dst_len=total)
    assert got[:100] == b"\xEE" * 100 and got[total:] == b"\xEE" * 64
    assert got[offs[1]:offs[2]] == good[1] + b"\xEE" * 5 and got[offs[3]:offs[4]] == good[3][:-7] and got[offs[4]:offs[5]] == good[4]
    offs_bad = np.array([50, 40, -5, 10, total + 200, total + 300, total + 400], dtype=np.int64)
    lens, got, _ = run_kernels(sc, offs=offs_bad, dst_len=total)
    assert got == b"\xEE" * len(got)


# ---------------------------------------------------------------------------- GPU tier: end to end
def _check_case(idx, extra, tot, **kw):
    from sam2consensus_amd.cli import run_text
    case = CASES[idx]
    status, files = run_text(case["sam"], list(case["args"]) + extra, **kw)
    assert status == case["status"], case["name"]
    if status != "ok":
        assert files == {}, case["name"]
        return
    assert {k: v for k, v in files.items() if k.endswith(".fasta")} == case["files"], case["name"]
    want, entries = _oracle_files(*_oracle_text(case["sam"], case["args"]))
    assert {k: v for k, v in files.items() if not k.endswith(".fasta")} == want, case["name"]
    tot.add(entries)


CHUNK = 100   # golden cases per test: a run takes milliseconds, most of a test of one would be its set-up
FIRSTS = list(range(0, len(CASES), CHUNK))
DONE = {}     # first case of a chunk → its totals


def _chunk(first):
    tot = _Totals()
    for idx in range(first, min(first + CHUNK, len(CASES))):
        _check_case(idx, ["--insertions"], tot)
    DONE[first] = tot


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRSTS)
def test_golden_cases_with_insertions(first):
    """run_text(..., ["--insertions"]) on every golden case, CHUNK to a test: the case's status;
    on ok the reference's FASTA files and an insertion table per reference with Σcoverage > 0,
    equal to the oracle's insertion lists through the model."""
    _chunk(first)


@pytest.mark.gpu
def test_golden_cases_hold_the_totals():
    """The lines the chunks compared, summed: the CPU tier's floor (a chunk that did not run in
    this session is run here)."""
    total = _Totals()
    for first in FIRSTS:
        if first not in DONE:
            _chunk(first)
        for k in ("lines", "above", "other", "cases"):
            setattr(total, k, getattr(total, k) + getattr(DONE[first], k))
    total.check()


def _run_sam(sam, extra=()):
    from sam2consensus_amd.cli import run_text
    status, files = run_text(sam, ["--insertions"] + list(extra))
    assert status == "ok"
    refs, counts, inserts, prefix = _oracle_text(sam, [])
    mr = int(extra[1]) if extra else 1
    want, entries = _oracle_files(refs, counts, inserts, prefix, mr)
    got = {k: v for k, v in files.items() if not k.endswith(".fasta")}
    assert got == want, (got, want)
    return got, entries


def _read(name, ref, pos, cigar, seq):
    return "%s\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (name, ref, pos, cigar, seq)


@pytest.mark.gpu
def test_hand_written_sam_texts():
    """Against the oracle: long motifs grouped, the last-base difference, a short motif at the
    same position; an insertion at the read's end (cov < reads); a soft clip before the
    insertion; SEQ shorter than the CIGAR (a truncated and an empty motif); a negative key; a
    second reference with coverage and no insertion; a third without reads."""
    hdr = "@SQ\tSN:g1\tLN:60\n@SQ\tSN:g2\tLN:30\n@SQ\tSN:g3\tLN:20\n"
    m20, flank = "ACGTTGCAACGTTGCAACGT", "ACGTACGTAC"
    sam = hdr
    for k in range(5):
        sam += _read("a%d" % k, "g1", 3, "10M20I10M", flank + m20 + flank)
    sam += _read("b0", "g1", 3, "10M20I10M", flank + m20[:-1] + "A" + flank)
    sam += _read("b1", "g1", 3, "10M20I10M", flank + m20[:-1] + "G" + flank)
    for k in range(3):
        sam += _read("c%d" % k, "g1", 3, "10M2I10M", flank + "TN" + flank)
    sam += _read("d0", "g1", 31, "10M3I", flank + "GGA")                 # ends in I: keys position 41, covered by nobody
    sam += _read("d1", "g1", 31, "10M3I", flank + "GGA")
    sam += _read("e0", "g1", 45, "4S5M2I3M", "TTTT" + "ACGTA" + "CC" + "GTA")      # a soft clip before the insertion
    sam += _read("f0", "g1", 50, "4M6I", "ACGTGG")                       # SEQ ends inside the motif: GG
    sam += _read("f1", "g1", 50, "4M6I", "ACGT")                         # the motif is empty: not listed
    sam += _read("g0", "g1", 0, "3I4M", "TTTACGT")                       # POS 0: key -1, not listed
    sam += _read("h0", "g2", 2, "12M", "ACGTACGTACGT")
    got, entries = _run_sam(sam)
    assert sorted(got) == ["g1__in.insertions.tsv", "g2__in.insertions.tsv"]
    assert got["g2__in.insertions.tsv"] == INS_HEADER.decode()
    t = got["g1__in.insertions.tsv"]
    assert ("13\t10\t5\t20\t%s\n13\t10\t3\t2\tTN\n13\t10\t1\t20\t%sA\n13\t10\t1\t20\t%sG\n" % (m20, m20[:-1], m20[:-1])) in t
    assert "41\t0\t2\t3\tGGA\n" in t and "50\t3\t1\t2\tCC\n" in t and "54\t0\t1\t2\tGG\n" in t
    assert t.count("\n") == 1 + 7 and len(entries) == 7
    assert "TTT" not in t
    got2, _ = _run_sam(sam, ["--min-ins-reads", "2"])
    assert got2["g1__in.insertions.tsv"].count("\n") == 1 + 3


def _model_ins(hb, prefix, min_reads=1):
    """{file: bytes} from batch_model: the events grouped per reference and formatted with the
    model's coverage; and the number of lines with reads > 1."""
    runs, events = bm.model_reads(hb)
    cov = bm.model_counts(hb, runs).sum(axis=0)
    off = np.asarray(hb.ref_off, dtype=np.int64)
    per = {}
    for gkey, syms in events:
        r = int(np.searchsorted(off, gkey, side="right")) - 1
        pos = gkey - int(off[r])
        assert 0 <= pos < int(hb.ref_len[r]) and syms
        k = (pos, "".join(SYM[s] for s in syms))
        d = per.setdefault(r, {})
        d[k] = d.get(k, 0) + 1
    assert sum(sum(d.values()) for d in per.values()) == hb.info.n_ins
    out, multi = {}, 0
    for r in range(hb.info.n_refs):
        if hb.ref_reads[r] > 0:
            a, ln = int(off[r]), int(hb.ref_len[r])
            e = [(p, m, n) for (p, m), n in per.get(r, {}).items()]
            multi += sum(n > 1 for _, _, n in e)
            out[hb.names[r].encode() + b"__" + prefix + b".insertions.tsv"] = INS_HEADER + table.format_insertions(
                e, [int(v) for v in cov[a:a + ln]], 1, min_reads)
    return out, multi


INS_KINDS = [("c2", {"n_refs": 18}), ("c2", {"n_refs": 18, "ins_max": 40, "ins_frac": 0.3}), ("c5", {"ref_len": 400_000}),
             ("c4", {"ref_len": 2000, "depth": 12000.0, "ins_frac": 0.05, "ins_max": 4})]


@pytest.mark.gpu
@pytest.mark.parametrize("name,over", INS_KINDS, ids=["c2", "c2-long", "c5", "c4"])
def test_every_tile_kind(name, over):
    """General tiles (c2), the long lists filled (c2 with motifs up to 40 bases), dense tiles
    (c5), deep tiles with many entries and repeated motifs (c4): the tables == the batch model's
    events grouped and formatted with its coverage, after the FASTA files, which equal the
    fused route's."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch(name, **over)
    if "ins_max" in over and name == "c2":
        assert hb.info.n_lng > 0
    if name == "c5":
        assert hb.info.n_dense > 0
    plain = consensus_batch(hb, [0.25, 0.75], b"x")
    both = consensus_batch(hb, [0.25, 0.75], b"x", insertions=1)
    nf = len(plain)
    assert plain and list(both)[:nf] == list(plain)
    for k, v in plain.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
    want, multi = _model_ins(hb, b"x")
    assert list(both)[nf:] == list(want)
    for k, v in want.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
    if name == "c4":
        assert multi > 0, "the deep configuration must repeat motifs"
    if name != "c5":
        assert sum(v.count(b"\n") - 1 for v in want.values()) > len(want)


@pytest.mark.gpu
def test_workspace_reuse():
    """run_with_tables(insertions=1) twice on one workspace: the same bytes and FASTA results;
    a plain run() on a fresh workspace is unchanged; insertions_table raises before anything
    filled the tables and after vote_all()."""
    import torch
    from sam2consensus_amd import configs
    from sam2consensus_amd.engine import DeviceBatch, Workspace

    def fetched(ws):
        stats, offs, out = ws.fetch()
        return stats.tobytes(), offs.tobytes(), bytes(out)

    hb = configs.synth_batch("c2", n_refs=18, ins_max=40, ins_frac=0.3)
    ws0 = Workspace(DeviceBatch(hb), [0.25])
    ws0.run()
    base = fetched(ws0)
    ws = Workspace(DeviceBatch(hb, dense_layers=True), [0.25], keep_counts=True)
    with pytest.raises(ValueError):
        ws.insertions_table()          # (nothing has filled the counts or the tables)
    runs = []
    for _ in range(2):
        res = ws.run_with_tables({"insertions": (1,)})
        assert set(res) == {"insertions"}
        offs, text = res["insertions"]
        runs.append((offs.tobytes(), text.cpu().numpy().tobytes(), fetched(ws)))
        with pytest.raises(ValueError):
            ws.insertions_table()      # (vote_all consumed the tables)
    assert runs[0] == runs[1] and runs[0][2] == base
    want, _ = _model_ins(hb, b"x")
    assert table.table_files(hb, b"x", offs, runs[0][1], table.INS_HEADER, table.INS_SUFFIX) == want
    three = ws.run_with_tables({"counts": (), "depth": (1,), "insertions": (2,)})
    assert list(three) == ["counts", "depth", "insertions"] and fetched(ws) == base
    assert table.table_files(hb, b"x", three["insertions"][0], three["insertions"][1].cpu().numpy().tobytes(), table.INS_HEADER,
                             table.INS_SUFFIX) == _model_ins(hb, b"x", 2)[0]
    two = ws.run_with_tables({"counts": ()})
    assert set(two) == {"counts"} and fetched(ws) == base
    ws.accumulate(keep_tables=True)   # (onto the counts the vote left zero)
    with pytest.raises(ValueError):
        ws.insertions_table(0)
    again = ws.insertions_table()
    assert again[1].cpu().numpy().tobytes() == runs[0][1]
    ws.vote_all()
    ws1 = Workspace(DeviceBatch(hb), [0.25])
    ws1.run()
    assert fetched(ws1) == base
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_all_five_tables_equal_the_separate_runs():
    """--counts --variants --depth --lowcov --insertions in one run: every file what the run with
    its flag alone gives; the insertion tables come last, after the depth summary."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch("c2", n_refs=3)
    kw = dict(min_depth=30)
    plain = consensus_batch(hb, [0.25], b"x", **kw)
    alone = [consensus_batch(hb, [0.25], b"x", counts=True, **kw), consensus_batch(hb, [0.25], b"x", variants=(1, 0.0), **kw),
             consensus_batch(hb, [0.25], b"x", depth=True, **kw), consensus_batch(hb, [0.25], b"x", lowcov=True, **kw),
             consensus_batch(hb, [0.25], b"x", insertions=1, **kw)]
    every = consensus_batch(hb, [0.25], b"x", counts=True, variants=(1, 0.0), depth=True, lowcov=True, insertions=1, **kw)
    order = list(plain)
    for files in alone:
        assert list(files)[:len(plain)] == list(plain) and len(files) > len(plain)
        order += list(files)[len(plain):]
    summary = order.pop(order.index(b"x.depth_summary.tsv"))
    ins = [k for k in order if k.endswith(b".insertions.tsv")]
    assert len(ins) == 3
    assert list(every) == [k for k in order if k not in ins] + [summary] + ins
    for files in alone:
        for k, v in files.items():
            assert every[k] == v, (k, tt._first_diff(every[k], v))
    assert {k: v for k, v in every.items() if k in ins} == _model_ins(hb, b"x")[0]
    assert consensus_batch(hb, [0.75], b"x", min_depth=1, fill=b"N", insertions=1)[ins[0]] == every[ins[0]]   # (-c, -m, -f change nothing)


@pytest.mark.gpu
def test_cli_process(tmp_path):
    """sam2consensus.py on a C1-sized file with insertions, with --insertions beside --counts and
    --depth: the stdout lines in order (the insertion tables' last, after the depth summary and
    before Done.), one .insertions.tsv per FASTA file, equal to the oracle's lists formatted, Σ
    reads of each table == the events the oracle counts for its reference; without the flags no
    such file and no such line, and the same FASTA files."""
    import subprocess
    import sys
    from sam2consensus_amd import configs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sam = str(tmp_path / "c1.sam")
    configs.synth_write("c1", sam, depth=30.0, ins_frac=0.2, ins_max=24)
    refs, counts, inserts, _ = _oracle_text(open(sam).read(), ["-c", "0.25"])
    names = list(refs)
    assert len(names) == 10
    outs = {}
    for tag, extra in (("plain", []), ("every", ["--depth", "--insertions", "--counts", "--min-ins-reads", "1"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(root, "sam2consensus.py"), "-i", sam, "-o", str(out), "-c", "0.25"] +
                           extra, capture_output=True, text=True, timeout=240, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (r.stdout.split("\n"), {fn: open(os.path.join(out, fn), "rb").read() for fn in os.listdir(out)})
    head, plain = outs["plain"]
    kp = head.index("Done.")
    assert not any("nsertion" in ln for ln in head) and sorted(plain) == sorted(n + "__c1.fasta" for n in names)
    so, files = outs["every"]
    d = str(tmp_path / "every")
    k = so.index("Done.")
    assert so[k:] == head[kp:] and so[:k - 41] == head[:kp - 10]

    def saved(what, suffix):
        return ["%s saved for %s in: %s/%s__c1.%s" % (what, n, d, n, suffix) for n in names]

    assert so[k - 41:k] == (saved("Consensus sequence at 25%", "fasta") + saved("Count table", "counts.tsv") +
                            saved("Depth table", "depth.tsv") + ["Depth summary saved in: %s/c1.depth_summary.tsv" % d] +
                            saved("Insertion table", "insertions.tsv"))
    assert len(files) == 41 and {k2: v for k2, v in files.items() if k2.endswith(".fasta")} == plain
    n_long = 0
    for n in names:
        rows = files[n + "__c1.insertions.tsv"].split(b"\n")
        assert rows[0] + b"\n" == INS_HEADER and rows[-1] == b""
        f = [row.split(b"\t") for row in rows[1:-1]]
        kept = [(key, m) for key, m in inserts[n] if 0 <= key < refs[n] and m]
        assert sum(int(x[2]) for x in f) == len(kept) > 0
        assert all(int(x[3]) == len(x[4]) for x in f)
        n_long += sum(int(x[3]) > 16 for x in f)
    assert n_long > 0
    want, _ = _oracle_files(refs, counts, inserts, "c1")
    assert {k2: v.decode() for k2, v in files.items() if k2.endswith(".insertions.tsv")} == want
