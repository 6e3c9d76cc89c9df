"""--deletions: the gap events the reads carry (sam2consensus_amd/table.py, csrc/s2c_dels.hip).

Without a GPU: the issue's two literal tables through the model, the model against a restatement
on every ok golden case (gap characters from the oracle's tokeniser, the rebuilt seqout equal to
the oracle's parsecigar, cov from the oracle's pileup), the order, the flags and their refused
combinations, the bindings and their argument errors.  On the GPU: the walks through run_text on
hand-written SAM texts (tile and word edges, the tokens that split a run and those that do not,
reads over -d, the POS <= 0 wrap, a long N skip, 10,000 contended adds, 300 lengths at one start,
two references, no event, --min-del-reads), the bucket and format kernels alone on a synthetic
table (the digit ladder, a cov past 2^32, empty and full tiles, a long name, shifted dst; the
guards), the golden cases end to end, every tile kind against a numpy walk of the pieces, a
reused workspace and the CLI process.  Every comparison is exact."""
import functools
import os
import re

import numpy as np
import pytest

import batch_model as bm
from devmem import _dev_i64, _ptr, _stream
import s2c_oracle as o
import test_table as tt

from sam2consensus_amd import table

CASES = tt.CASES
DEL_HEADER = b"ref\tstart\tend\tlen\treads\tdropped\tcov\n"
HEAD = DEL_HEADER.decode()
NAME = "in.deletions.tsv"


# ---------------------------------------------------------------------------- expectations
def _reads(sam_text, args):
    """(refs, counts, opt, [(rname, pos0, seqout, gap flags, dropped)]) of a SAM text: per read the
    oracle's tokens, seqout rebuilt from them with a flag per character — whether a D, N or P
    token produced it — and checked against the oracle's parsecigar."""
    opt = o.parse_argv(["-i", "in.sam"] + list(args))
    lines = o._lines(sam_text)
    refs = o.read_header(lines)
    counts, _ = o.pileup(lines, refs, opt)
    reads = []
    for line in lines:
        if line[0] == "@":
            continue
        f = line.split("\t")
        if f[5] == "*":
            continue
        rname, pos = o.py2_split(f[2])[0], o.py2_int(f[3]) - 1
        chars, gaps, start = [], [], 0
        for op, ln in o.tokenize_cigar(f[5]):
            if op in "M=X":
                piece = f[9][start:start + ln]
                chars.append(piece)
                gaps += [False] * len(piece)
                start += ln
            elif op in "DNP":
                chars.append("-" * ln)
                gaps += [True] * ln
            elif op in "IS":
                start += ln
        seqout = "".join(chars)
        assert seqout == o.parsecigar(f[5], f[9], pos)[0]
        reads.append((rname, pos, seqout, gaps, bool(opt.maxdel_active and seqout.count("-") > opt.maxdel)))
    return refs, counts, opt, reads


def _fragments(refs, reads):
    """{ref: [(chars, dropped)]} for table.gap_events: a read's span from its first counted
    character to its last, cut at the wrap (index 0 starts the second fragment)."""
    frags = {r: [] for r in refs}
    for rname, pos, seqout, gaps, drop in reads:
        counted = [k for k, ch in enumerate(seqout) if not (drop and ch == "-")]
        if not counted:
            continue
        wrapped, straight = [], []
        for k in range(counted[0], counted[-1] + 1):
            p = pos + k
            (wrapped if p < 0 else straight).append((p + refs[rname] if p < 0 else p, gaps[k]))
        frags[rname] += [(wrapped, drop), (straight, drop)]
    return frags


def _cov(refs, counts):
    return {r: [sum(c) for c in counts[r]] for r in refs}


def _model_text(sam_text, args=(), min_reads=1):
    """The deletion file's content through the model."""
    refs, counts, _, reads = _reads(sam_text, args)
    frags = _fragments(refs, reads)
    events = {r: table.gap_events(frags[r]) for r in refs}
    return (DEL_HEADER + table.format_deletions(events, _cov(refs, counts), min_reads)).decode()


def _restated(sam_text, args=(), min_reads=1):
    """The definition restated: a read's span as a string of 'g' (gap character) and 'b', cut at
    the wrap, its runs found by a regular expression; the events counted in a dict and printed
    through sorted() with an explicit key."""
    refs, counts, _, reads = _reads(sam_text, args)
    order = list(refs)
    n = {}
    for rname, pos, seqout, gaps, drop in reads:
        kept = [not (drop and ch == "-") for ch in seqout]
        if not any(kept):
            continue
        k0, k1 = kept.index(True), len(kept) - kept[::-1].index(True)
        marks = "".join("g" if g else "b" for g in gaps)
        cut = min(max(-pos, k0), k1)   # seqout index of reference index 0, inside the span
        for lo, hi in ((k0, cut), (cut, k1)):
            for m in re.finditer("g+", marks[lo:hi]):
                p = pos + lo + m.start()
                key = (order.index(rname), p + refs[rname] if p < 0 else p, m.end() - m.start())
                e = n.setdefault(key, [0, 0])
                e[0] += 1
                e[1] += int(drop)
    out = [HEAD]
    for r, s, ln in sorted(n, key=lambda k: (k[0], k[1], k[2])):
        if n[(r, s, ln)][0] >= min_reads:
            out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (order[r], s + 1, s + ln, ln, n[(r, s, ln)][0], n[(r, s, ln)][1],
                                                         sum(counts[order[r]][s])))
    return "".join(out)


def _read(name, ref, pos, cigar, seq):
    return "%s\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (name, ref, pos, cigar, seq)


def _issue_sam():
    sam = "@SQ\tSN:g1\tLN:400\n@SQ\tSN:g2\tLN:40\n"
    for k in range(3):
        sam += _read("a%d" % k, "g1", 5, "10M3D10M", "A" * 20)
    sam += _read("b0", "g1", 11, "4M2D1I2D4M", "ACGTACGTA")
    sam += _read("c0", "g1", 5, "10M3D10M160N10M", "C" * 30)
    sam += _read("d0", "g2", 3, "5M1P5M", "G" * 10)
    return sam


ISSUE_TABLE = HEAD + "g1\t15\t17\t3\t4\t1\t4\ng1\t15\t18\t4\t1\t0\t4\ng1\t28\t187\t160\t1\t1\t0\ng2\t8\t8\t1\t1\t0\t1\n"
ISSUE_RULE_OFF = HEAD + "g1\t15\t17\t3\t4\t0\t5\ng1\t15\t18\t4\t1\t0\t5\ng1\t28\t187\t160\t1\t0\t1\ng2\t8\t8\t1\t1\t0\t1\n"
WRAP_SAM = "@SQ\tSN:w\tLN:50\n" + _read("w0", "w", -2, "2M4D3M", "ACGTA") + _read("w1", "w", 1, "2D3M2D", "AAA")
WRAP_TABLE = HEAD + "w\t1\t2\t2\t1\t0\t2\nw\t1\t3\t3\t1\t0\t2\nw\t6\t7\t2\t1\t0\t2\nw\t50\t50\t1\t1\t0\t1\n"


# ---------------------------------------------------------------------------- CPU tier
def test_constants_and_registry():
    assert (table.DEL_HEADER, table.DEL_SUFFIX) == (DEL_HEADER, b".deletions.tsv")
    assert [t.key for t in table.TABLES] == ["counts", "variants", "depth", "lowcov", "insertions", "links"]
    with pytest.raises(TypeError):
        table.request(deletions=1)   # (no seventh entry: the deletion table is a per-run file)


def test_issue_literals_through_the_model():
    assert _model_text(_issue_sam()) == ISSUE_TABLE
    assert _model_text(_issue_sam(), ["-d", "150"]) == ISSUE_RULE_OFF
    assert _model_text(_issue_sam(), min_reads=2) == ISSUE_TABLE[:ISSUE_TABLE.index("g1\t15\t18")]
    assert _model_text(WRAP_SAM) == WRAP_TABLE
    for sam, args in ((_issue_sam(), []), (_issue_sam(), ["-d", "150"]), (WRAP_SAM, [])):
        assert _restated(sam, args) == _model_text(sam, args)


def test_model_against_the_restatement_on_every_ok_case():
    lines = cases = multi = 0
    for case in CASES:
        if case["status"] != "ok":
            continue
        for mr in (1, 2):
            want = _restated(case["sam"], case["args"], mr)
            assert _model_text(case["sam"], case["args"], mr) == want, case["name"]
        body = _restated(case["sam"], case["args"]).split("\n")[1:-1]
        lines += len(body)
        cases += bool(body)
        multi += sum(int(ln.split("\t")[4]) >= 2 for ln in body)
    assert lines >= 50 and cases >= 10 and multi >= 1, (lines, cases, multi)


def test_order_and_ties():
    """Several lengths at one start, two references in the mapping's order, ties in reads."""
    ev = {"zz": {(9, 3): [2, 0], (9, 1): [2, 1], (9, 20): [7, 7], (2, 5): [2, 0]}, "aa": {(0, 1): [1, 0], (0, 2): [1, 1]}}
    cov = {"zz": list(range(100, 140)), "aa": [0, 4]}
    assert table.format_deletions(ev, cov) == (b"zz\t3\t7\t5\t2\t0\t102\nzz\t10\t10\t1\t2\t1\t109\nzz\t10\t12\t3\t2\t0\t109\n"
                                               b"zz\t10\t29\t20\t7\t7\t109\naa\t1\t1\t1\t1\t0\t0\naa\t1\t2\t2\t1\t1\t0\n")
    assert table.format_deletions(ev, cov, 3) == b"zz\t10\t29\t20\t7\t7\t109\n" and table.format_deletions(ev, cov, 8) == b""
    with pytest.raises(ValueError):
        table.format_deletions(ev, cov, 0)
    got = table.gap_events([([(4, False), (5, True), (6, True), (7, False), (8, True)], False), ([(5, True), (6, True)], True), ([], True)])
    assert got == {(5, 2): [2, 1], (8, 1): [1, 0]}


def test_parser_has_the_flags(capsys):
    from sam2consensus_amd.cli import build_parser, deletions_of, tables_of
    p = build_parser()
    a = p.parse_args(["-i", "x.sam"])
    assert a.deletions is False and a.min_del_reads is None and deletions_of(p, a) is None
    assert deletions_of(p, p.parse_args(["-i", "x.sam", "--deletions"])) == 1
    a = p.parse_args(["-i", "x.sam", "--deletions", "--min-del-reads", "3"])
    assert deletions_of(p, a) == 3 and tables_of(p, a) == {}
    assert deletions_of(p, p.parse_args(["-i", "x.sam", "--deletions", "--min-del-reads", str(2 ** 32 - 1)])) == 2 ** 32 - 1
    for argv, word in ((["--min-del-reads", "2"], "--min-del-reads needs --deletions"), (["--deletions", "--min-del-reads", "0"], "--min-del-reads"),
                       (["--deletions", "--min-del-reads", str(2 ** 32)], "--min-del-reads")):
        with pytest.raises(SystemExit) as e:
            deletions_of(p, p.parse_args(["-i", "x.sam"] + argv))
        assert e.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["-i", "x.sam", "--deletions", "--min-del-reads", "x"])
    h = p.format_help()
    assert "--deletions" in h and "--min-del-reads" in h and "PREFIX.deletions.tsv" in h


@pytest.mark.parametrize("env,extra,word", [({"WORLD_SIZE": "2"}, ["--deletions"], "--deletions is not available with more than one process"),
                                            ({"S2C_STREAM": "1M"}, ["--deletions"], "--deletions is not available with streamed batches"),
                                            ({"WORLD_SIZE": "2"}, ["--counts", "--deletions"], "--counts is not available with more than one process"),
                                            ({}, ["--deletions", "--min-del-reads", "0"], "--min-del-reads must be at least 1 and below 2^32"),
                                            ({}, ["--deletions", "--min-del-reads", str(2 ** 32)], "--min-del-reads must be at least 1 and below 2^32"),
                                            ({}, ["--min-del-reads", "2"], "--min-del-reads needs --deletions")],
                         ids=["world2", "stream", "world2-counts", "min0", "min2p32", "alone"])
def test_refused_combinations(env, extra, word, tmp_path, monkeypatch, capsys):
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
        main(["-i", str(sam), "-o", str(tmp_path / "out")] + extra)
    assert e.value.code == 2 and word in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == ["in.sam"]


NAMES = ["s2c_dels_count", "s2c_dels_collect", "s2c_dels_tiles", "s2c_dels_scatter", "s2c_dels_len", "s2c_dels_write"]


def test_dels_symbols_declared_and_bound():
    from sam2consensus_amd import _lib
    lib = _lib.lib
    assert set(NAMES) <= set(_lib.EXPORTS) and lib.s2c_abi_version() == 14 and _lib.ABI_VERSION == 14
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2c.h")).read()
    assert all("int " + n + "(" in header for n in NAMES) and "k_dels_*" in header and "#define S2C_ABI_VERSION 14" in header
    assert [len(getattr(lib, f).argtypes) for f in NAMES] == [7, 14, 7, 10, 17, 17]
    OK, ARG = _lib.S2C_OK, _lib.S2C_ERR_ARG   # (argument errors need no device)
    cnt = lambda npc=0, no=0, pl=64: lib.s2c_dels_count(None, None, npc, no, pl, None, None)  # noqa: E731
    col = lambda npc=0, no=0, nq=0, pl=64, ns=2: lib.s2c_dels_collect(None, None, None, None, npc, no, nq, 1, 150, pl, None, ns, None, None)  # noqa: E731
    til = lambda ns=0, nw=1, nt=1: lib.s2c_dels_tiles(None, ns, None, nw, nt, None, None)  # noqa: E731
    sca = lambda ns=0, nw=1, nt=1, ne=1: lib.s2c_dels_scatter(None, ns, None, nw, nt, None, None, None, ne, None)  # noqa: E731
    ln = lambda ne=0, nt=0, nl=0, nr=0, pl=64, mr=1: lib.s2c_dels_len(None, None, ne, None, None, nt, None, None, nl, None, nr, None, pl, mr, None, None, None)  # noqa: E731
    wr = lambda ne=0, nt=0, nl=0, nr=0, pl=64, dl=0: lib.s2c_dels_write(None, ne, None, None, None, nt, None, None, nl, None, nr, None, pl, None, None, dl, None)  # noqa: E731
    assert cnt() == OK and cnt(npc=-1) == ARG and cnt(no=-1) == ARG and cnt(pl=-1) == ARG and cnt(pl=2 ** 32) == ARG and cnt(npc=1) == ARG
    assert col() == OK and col(npc=-1) == ARG and col(no=-1) == ARG and col(nq=-1) == ARG and col(pl=-1) == ARG and col(npc=1) == ARG
    assert col(ns=0) == ARG and col(ns=3) == ARG and col(ns=-2) == ARG
    assert til() == OK and til(ns=-1) == ARG and til(nw=-1) == ARG and til(nt=-1) == ARG and til(ns=1) == ARG
    assert sca() == OK and sca(ns=-1) == ARG and sca(nw=-1) == ARG and sca(nt=-1) == ARG and sca(ne=-1) == ARG and sca(ne=2 ** 32) == ARG and sca(ns=1) == ARG
    assert ln() == OK and ln(ne=-1) == ARG and ln(nt=-1) == ARG and ln(nl=-1) == ARG and ln(nr=-1) == ARG and ln(pl=-1) == ARG
    assert ln(mr=0) == ARG and ln(mr=2 ** 32) == ARG and ln(nt=1) == ARG and ln(ne=2 ** 32) == ARG
    assert wr() == OK and wr(ne=-1) == ARG and wr(nt=-1) == ARG and wr(nl=-1) == ARG and wr(nr=-1) == ARG and wr(pl=-1) == ARG
    assert wr(dl=-1) == ARG and wr(nt=1) == ARG


# ---------------------------------------------------------------------------- GPU tier: the walks through run_text
def _check_sam(sam, base=(), extra=(), min_reads=1):
    """run_text(sam, base + --deletions + extra): the deletion file is the model's at `base`, it is
    the files' last, and the other files are those of the run without the flag."""
    from sam2consensus_amd.cli import run_text
    status, files = run_text(sam, list(base) + ["--deletions"] + list(extra))
    assert status == "ok" and list(files)[-1] == NAME
    want = _model_text(sam, base, min_reads)
    assert files[NAME] == want, (files[NAME], want)
    return files[NAME]


def _body(*lines):
    return HEAD + "".join(ln + "\n" for ln in lines)


@pytest.mark.gpu
def test_issue_example_rule_on_and_off():
    from sam2consensus_amd.cli import run_text
    assert _check_sam(_issue_sam()) == ISSUE_TABLE
    assert _check_sam(_issue_sam(), base=["-d", "150"]) == ISSUE_RULE_OFF
    assert _check_sam(WRAP_SAM) == WRAP_TABLE
    plain = run_text(_issue_sam(), [])[1]
    both = run_text(_issue_sam(), ["--deletions"])[1]
    assert list(both) == list(plain) + [NAME] and all(both[k] == v for k, v in plain.items())
    assert run_text(_issue_sam(), [], deletions=2)[1][NAME] == ISSUE_TABLE[:ISSUE_TABLE.index("g1\t15\t18")]
    assert run_text(_issue_sam(), ["--deletions"], deletions=2)[1][NAME] == ISSUE_TABLE   # (the flag wins)


@pytest.mark.gpu
@pytest.mark.parametrize("mr", [1, 2, 2 ** 32 - 1])
def test_min_del_reads(mr):
    got = _check_sam(_issue_sam(), extra=["--min-del-reads", str(mr)], min_reads=mr)
    assert got.count("\n") == {1: 5, 2: 2, 2 ** 32 - 1: 1}[mr]


@pytest.mark.gpu
def test_events_at_tile_and_word_edges():
    """Tiles of 64 positions: events that start on the last position of a 32-position word (32),
    of a tile (64, 128) and reach into the next, in the reference's first tile and in its last."""
    from sam2consensus_amd import _lib
    from sam2consensus_amd.batch import Parser
    from sam2consensus_amd.cli import consensus_batch
    sam = "@SQ\tSN:g1\tLN:400\n"
    sam += _read("a", "g1", 1, "2M3D20M", "A" * 22)            # first tile: 3 .. 5
    sam += _read("b", "g1", 20, "12M5D10M", "C" * 22)          # 32 .. 36: over the word edge
    sam += _read("c", "g1", 50, "14M4D10M", "G" * 24) * 2      # 64 .. 67: the tile's last position into the next
    sam += _read("d", "g1", 100, "28M70D5M", "T" * 33)         # 128 .. 197: over a whole tile
    sam += _read("e", "g1", 380, "10M2D9M", "A" * 19)          # last tile: 390 .. 391
    sam += _read("f", "g1", 390, "8M3D", "A" * 8)              # a trailing D to the reference's end: 398 .. 400
    p = Parser(True, 150)
    try:
        _lib.check(_lib.lib.s2c_parser_set_tile_width(p._p, 64))
        p.feed(sam.encode())
        hb = p.finish()
    finally:
        p.close()
    assert hb.info.n_tiles >= 7 and [int(v) for v in hb.tiles[1, :2]] == [64, 128]
    files = consensus_batch(hb, [0.25], b"in", deletions=1)
    want = _model_text(sam)
    assert list(files)[-1] == NAME.encode() and files[NAME.encode()].decode() == want
    assert want == _body("g1\t3\t5\t3\t1\t0\t1", "g1\t32\t36\t5\t1\t0\t1", "g1\t64\t67\t4\t2\t0\t2", "g1\t128\t197\t70\t1\t0\t1",
                         "g1\t390\t391\t2\t1\t0\t2", "g1\t398\t400\t3\t1\t0\t2")


@pytest.mark.gpu
def test_tokens_that_do_not_split_a_run_and_those_that_do():
    sam = "@SQ\tSN:g1\tLN:200\n"
    sam += _read("i", "g1", 11, "4M2D1I2D4M", "ACGTACGTA")
    sam += _read("s", "g1", 31, "4M2D3S2D4M", "ACGTNNNACGT")
    sam += _read("h", "g1", 51, "4M2D2H2D4M", "ACGTACGT")
    sam += _read("m", "g1", 71, "4M2D5M2D", "ACGT")            # the second M takes nothing: SEQ ran out
    sam += _read("x", "g1", 91, "4M2D1M2D4M", "ACGT-ACGT")     # a '-' of SEQ is a base: two events
    sam += _read("b", "g1", 111, "4M2D1M2D4M", "ACGTAACGT")
    got = _check_sam(sam)
    assert got == _body("g1\t15\t18\t4\t1\t0\t1", "g1\t35\t38\t4\t1\t0\t1", "g1\t55\t58\t4\t1\t0\t1", "g1\t75\t78\t4\t1\t0\t1",
                        "g1\t95\t96\t2\t1\t0\t1", "g1\t98\t99\t2\t1\t0\t1", "g1\t115\t116\t2\t1\t0\t1", "g1\t118\t119\t2\t1\t0\t1")


@pytest.mark.gpu
def test_reads_over_maxdel():
    """A dropped read lists its interior gap with dropped 1 and neither its leading nor its
    trailing D; the same event from a counted read sums; a dropped read of D only lists nothing;
    the '-' of SEQ count towards the rule."""
    sam = "@SQ\tSN:g1\tLN:900\n"
    sam += _read("d", "g1", 1, "7D10M3D10M160N10M9D", "C" * 30)     # leading 1 .. 7, trailing: absent
    sam += _read("k", "g1", 8, "10M3D10M", "A" * 20)                 # the same 18 .. 20 from a counted read
    sam += _read("o", "g1", 300, "200D", "A")                        # nothing counted: no line
    sam += _read("q", "g1", 500, "2D5M2D3M146D4M", "AC--TGGGACGT")   # 150 D/N/P + 2 '-' of SEQ: dropped
    sam += _read("r", "g1", 700, "5M150D5M", "A" * 10)               # exactly 150: counted
    got = _check_sam(sam)
    assert got == _body("g1\t18\t20\t3\t2\t1\t1", "g1\t31\t190\t160\t1\t1\t0", "g1\t507\t508\t2\t1\t1\t0", "g1\t512\t657\t146\t1\t1\t0",
                        "g1\t705\t854\t150\t1\t0\t1")
    off = _check_sam(sam, base=["-d", "150"])
    assert "g1\t1\t7\t7\t1\t0\t1\n" in off and "g1\t300\t499\t200\t1\t0\t1\n" in off
    assert all(ln.split("\t")[5] == "0" for ln in off.split("\n")[1:-1]) and off.count("\n") == 1 + 9


@pytest.mark.gpu
def test_wrap_with_a_deletion_across_it():
    got = _check_sam(WRAP_SAM)
    assert got == WRAP_TABLE
    sam = "@SQ\tSN:w\tLN:60\n@SQ\tSN:v\tLN:60\n" + _read("w0", "v", -4, "2M6D3M", "ACGTA") * 3
    assert _check_sam(sam) == _body("v\t1\t3\t3\t3\t0\t3", "v\t58\t60\t3\t3\t0\t3")


@pytest.mark.gpu
def test_long_skip_beyond_the_window():
    from sam2consensus_amd import _lib
    from sam2consensus_amd.batch import parse_text
    sam = "@SQ\tSN:g1\tLN:3200\n"
    for k in range(3):
        sam += _read("n%d" % k, "g1", 1, "10M3000N10M", "A" * 20)
    sam += _read("m", "g1", 5, "6M3000N2D10M", "C" * 16)
    hb = parse_text(sam)
    assert hb.info.n_long > 0 and any((int(w) >> 24) & _lib.S2C_PF_LONG for w in hb.pc[:hb.info.n_pieces, 3])
    assert _check_sam(sam) == _body("g1\t11\t3010\t3000\t3\t3\t0", "g1\t11\t3012\t3002\t1\t1\t0")
    assert _check_sam(sam, base=["-d", "9"]) == _body("g1\t11\t3010\t3000\t3\t0\t4", "g1\t11\t3012\t3002\t1\t0\t4")


@pytest.mark.gpu
def test_ten_thousand_contended_adds_are_exact():
    sam = "@SQ\tSN:g1\tLN:100\n" + "".join(_read("r%d" % k, "g1", 1, "10M3D10M", "A" * 20) for k in range(10000))
    assert _check_sam(sam) == _body("g1\t11\t13\t3\t10000\t0\t10000")


@pytest.mark.gpu
def test_three_hundred_lengths_at_one_start():
    sam = "@SQ\tSN:g1\tLN:700\n"
    order = [(7 * k) % 300 + 1 for k in range(300)]   # every length 1 .. 300 once, not in order
    assert sorted(order) == list(range(1, 301))
    sam += "".join(_read("r%d" % ln, "g1", 91, "10M%dD5M" % ln, "A" * 15) for ln in order)
    got = _check_sam(sam, base=["-d", "9"])
    lines = got.split("\n")[1:-1]
    assert [ln.split("\t")[1:4] for ln in lines] == [["101", str(100 + n), str(n)] for n in range(1, 301)]


@pytest.mark.gpu
def test_two_references_events_in_the_second_only_and_none():
    long_name = "L" * 40
    sam = "@SQ\tSN:a\tLN:70\n@SQ\tSN:%s\tLN:70\n@SQ\tSN:c\tLN:70\n" % long_name
    sam += _read("x", "a", 1, "20M", "A" * 20) + _read("y", long_name, 5, "5M2D5M", "C" * 10) * 2
    assert _check_sam(sam) == _body(long_name + "\t10\t11\t2\t2\t0\t2")
    none = "@SQ\tSN:a\tLN:70\n" + _read("x", "a", 1, "20M", "A" * 20) + _read("i", "a", 3, "5M2I5M", "C" * 12)
    assert _check_sam(none) == HEAD


# ---------------------------------------------------------------------------- GPU tier: the bucket and format kernels alone
DIGITS = [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [4294967295]
TW = 2048
PAD_L = 7 * TW


def _u32(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    if a.size < 4:
        a = np.concatenate([a, np.zeros(4 - a.size, dtype=np.uint32)])
    return torch.from_numpy(a.view(np.int32)).cuda()


class DelScene:
    """A hand-built event table over seven tiles of 2,048 positions.  Tile 0 (reference "r", one
    character, printed from 1): the digit ladder for len, reads and dropped at its first positions,
    three lengths at one start, and starts of 3 and 4 digits; tiles 5 and 6 print from 99,990 and
    9,999,990, their events' starts going from 5 to 6 and from 7 to 8 digits (tile 3: 9 to 10).  Tile 1 (a name of 300 characters, printed up to 9999999999):
    every position an event, so a step's lines are more than the LDS image holds and go out byte
    by byte; its last events end past 10^10.  Tile 2: no entry.  Tile 3 ("r3"): an event on each
    of its first and last positions, the coverage 25769803770 there.  Tile 4: a block cut to
    nothing (a reference without coverage): its entries are skipped.  Slots that are no entry: a
    zero length, a position in the padding (wtile 0xFFFFFFFF), a tile past n_tiles."""

    def __init__(self):
        ev = {}
        for k, v in enumerate(DIGITS):
            ev[(3 * k, (v % 4000) + 1)] = (v, DIGITS[-1 - k])
            ev[(3 * k + 1, v)] = (1 + k, k)
        ev[(100, 7)] = (5, 0)
        ev[(100, 2)] = (5, 5)
        ev[(100, 4000000000)] = (9, 1)
        for p in range(TW):
            ev[(TW + p, 1 + (p * 37) % 50)] = (p + 1, p % 3)
        ev[(3 * TW, 3)] = (2, 1)
        for g in (998, 999, 2046, 5 * TW + 5, 5 * TW + 9, 5 * TW + 10, 6 * TW + 9, 6 * TW + 10):
            ev[(g, 1)] = (1, 0)
        ev[(4 * TW - 1, 9)] = (4294967295, 4294967295)
        self.skipped = {(4 * TW + 5, 2): (3, 0), (4 * TW + 9, 1): (1, 0)}
        self.events = ev
        self.names = [b"r", b"N" * 300, b"r3", b"gone"]
        self.tile_ref = [0, 1, 1, 2, 3, 0, 2]
        self.blocks = np.array([(0, TW, 1), (TW, 2 * TW, 10 ** 10 - TW), (2 * TW, 3 * TW, 1), (3 * TW, 4 * TW, 10 ** 9 - 5),
                                (4 * TW, 4 * TW, 1), (5 * TW, 6 * TW, 99990), (6 * TW, 7 * TW, 9999990)], dtype=np.int64)
        self.counts = np.zeros((6, PAD_L), dtype=np.uint32)
        self.counts[:, 100] = (1, 2, 3, 4, 5, 6)
        self.counts[:, TW:2 * TW] = np.arange(TW, dtype=np.uint32)[None, :] % 11
        self.counts[:, 3 * TW] = 4294967295
        self.counts[:, 4 * TW - 1] = 4294967295
        self.wtile = np.repeat(np.arange(7, dtype=np.uint32), TW // 32)
        self.wtile[-2:] = 0xFFFFFFFF
        junk = [(7, 0, 9, 9), (PAD_L - 1, 3, 1, 0), (PAD_L + 40, 3, 1, 0)]
        rows = [(g, ln, n, d) for (g, ln), (n, d) in list(ev.items()) + list(self.skipped.items())] + junk
        rng = np.random.RandomState(7)
        self.n_slots = 8192
        slots = np.zeros((self.n_slots, 4), dtype=np.uint32)
        where = rng.permutation(self.n_slots)[:len(rows)]
        slots[where] = np.array(rows, dtype=np.uint64).astype(np.uint32)
        self.slots = slots
        self.n_rows = len(rows)

    def want(self, min_reads=1, blocks=None):
        blocks = self.blocks if blocks is None else blocks
        out = []
        for t, (a, b, p0) in enumerate(blocks.tolist()):
            txt = b""
            if 0 <= a <= b <= PAD_L and 0 <= p0 <= 10 ** 10 - (b - a):
                for (g, ln), (n, d) in sorted(self.events.items()):
                    if a <= g < b and n >= min_reads:
                        s = p0 + g - a
                        txt += self.names[self.tile_ref[t]] + b"\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
                            s, s + ln - 1, ln, n, d, int(self.counts[:, g].astype(np.int64).sum()))
            out.append(txt)
        return out


def run_format(sc, min_reads=1, blocks=None, offs=None, dst_len=None, shift=0, n_ent=None, tstart=None):
    """(lens, tn, dst bytes with 64 guard bytes behind, offs): s2c_dels_tiles, the prefix sum,
    s2c_dels_scatter, s2c_dels_len, the prefix sum, s2c_dels_write."""
    import torch
    from sam2consensus_amd import _lib
    lib = _lib.lib
    blocks = sc.blocks if blocks is None else blocks
    nt = len(blocks)
    slots, wtile = _u32(sc.slots), _u32(sc.wtile)
    before = slots.clone()
    tcount, cursor, tn = (torch.zeros(nt, dtype=torch.int32, device="cuda") for _ in range(3))
    ts = torch.zeros(nt + 1, dtype=torch.int64, device="cuda")
    _lib.check(lib.s2c_dels_tiles(_ptr(slots), sc.n_slots, _ptr(wtile), len(sc.wtile), nt, _ptr(tcount), _stream()))
    torch.cumsum(tcount, 0, dtype=torch.int64, out=ts[1:])
    if tstart is not None:
        ts = _dev_i64(tstart)
    ne = sc.n_rows if n_ent is None else n_ent
    guard = 4
    ent_all = torch.full((4 * (sc.n_rows + 2 * guard),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tmp_all = ent_all.clone()
    ent, tmp = ent_all[4 * guard:], tmp_all[4 * guard:]
    _lib.check(lib.s2c_dels_scatter(_ptr(slots), sc.n_slots, _ptr(wtile), len(sc.wtile), nt, _ptr(ts), _ptr(cursor), _ptr(ent), ne, _stream()))
    tiles = np.zeros((nt, _lib.S2C_TILE_WORDS), dtype=np.uint32)
    tiles[:, 2] = sc.tile_ref[:nt]
    names = np.frombuffer(b"".join(sc.names), dtype=np.uint8)
    tab = np.array([(sum(len(n) for n in sc.names[:k]), len(sc.names[k])) for k in range(len(sc.names))], dtype=np.int64)
    import torch as T
    names_d, tab_d, tiles_d, counts_d, b = T.from_numpy(names.copy()).cuda(), _dev_i64(tab), _u32(tiles), _u32(sc.counts), _dev_i64(blocks)
    lens = torch.full((nt,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.s2c_dels_len(_ptr(ent), _ptr(tmp), ne, _ptr(ts), _ptr(tiles_d), nt, _ptr(b), _ptr(names_d), len(names), _ptr(tab_d),
                                len(sc.names), _ptr(counts_d), PAD_L, min_reads, _ptr(tn), _ptr(lens), _stream()))
    lens = lens.cpu().numpy()
    if offs is None:
        offs = np.concatenate([[0], np.cumsum(lens)]) + shift
    total = int(offs[-1]) if dst_len is None else dst_len
    dst = torch.full((max(total, int(np.max(offs)), 0) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    _lib.check(lib.s2c_dels_write(_ptr(ent), ne, _ptr(ts), _ptr(tn), _ptr(tiles_d), nt, _ptr(b), _ptr(names_d), len(names), _ptr(tab_d),
                                  len(sc.names), _ptr(counts_d), PAD_L, _ptr(_dev_i64(offs)), _ptr(dst), total, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(slots, before)
    for whole in (ent_all, tmp_all):   # (nothing stored in front of or behind the entries)
        assert whole[:4 * guard].tolist() == [0x5A5A5A5A] * (4 * guard) and whole[4 * (guard + sc.n_rows):].tolist() == [0x5A5A5A5A] * (4 * guard)
    return lens, tn.cpu().numpy(), dst.cpu().numpy().tobytes(), offs


def check_format(sc, min_reads=1, shift=0, **kw):
    want = sc.want(min_reads, **{k: v for k, v in kw.items() if k == "blocks"})
    lens, tn, got, offs = run_format(sc, min_reads, shift=shift, **kw)
    assert lens.tolist() == [len(w) for w in want], [(t, int(lens[t]), len(want[t])) for t in range(len(want)) if lens[t] != len(want[t])]
    assert tn.tolist() == [w.count(b"\n") for w in want]
    total = int(offs[-1])
    assert got[:shift] == b"\xEE" * shift and got[total:] == b"\xEE" * 64
    for t, w in enumerate(want):
        assert got[offs[t]:offs[t + 1]] == w, (t, tt._first_diff(got[offs[t]:offs[t + 1]], w))
    return b"".join(want)


@pytest.mark.gpu
@pytest.mark.parametrize("min_reads", [1, 3, 2 ** 32 - 1])
def test_format_kernels_on_a_synthetic_table(min_reads):
    sc = DelScene()
    text = check_format(sc, min_reads)
    for shift in (1, 7, 15):
        assert check_format(sc, min_reads, shift=shift) == text
    want = sc.want(min_reads)
    assert want[2] == b"" and want[4] == b""
    if min_reads == 1:
        assert b"r\t999\t999\t1\t1\t0\t0\nr\t1000\t1000\t1\t1\t0\t0\nr\t2047\t2047\t1\t1\t0\t0\n" in want[0]
        assert want[5] == b"r\t99995\t99995\t1\t1\t0\t0\nr\t99999\t99999\t1\t1\t0\t0\nr\t100000\t100000\t1\t1\t0\t0\n"
        assert want[6] == b"r3\t9999999\t9999999\t1\t1\t0\t0\nr3\t10000000\t10000000\t1\t1\t0\t0\n"
        assert want[0].startswith(b"r\t1\t10\t10\t9\t4294967295\t0\nr\t2\t10\t9\t1\t0\t0\n")
        for k, v in enumerate(DIGITS):
            assert b"r\t%d\t%d\t%d\t%d\t%d\t0\n" % (3 * k + 2, 3 * k + v + 1, v, 1 + k, k) in want[0]
        assert b"r\t101\t102\t2\t5\t5\t21\nr\t101\t107\t7\t5\t0\t21\nr\t101\t4000000100\t4000000000\t9\t1\t21\n" in want[0]
        assert want[1].count(b"\n") == TW and len(want[1]) > 256 * 300 and want[1].endswith(b"\t9999999999\t10000000038\t40\t2048\t1\t6\n")
        assert want[3] == (b"r3\t999999995\t999999997\t3\t2\t1\t25769803770\nr3\t1000002042\t1000002050\t9\t4294967295\t4294967295\t25769803770\n")
    if min_reads == 2 ** 32 - 1:
        assert text == b"r\t55\t3350\t3296\t4294967295\t9\t0\nr3\t1000002042\t1000002050\t9\t4294967295\t4294967295\t25769803770\n"


@pytest.mark.gpu
def test_format_guards():
    """Blocks outside the bounds, a tile range past the entries, offs decreasing or past dst_len:
    no byte is written for them, and the guard bytes around dst and the entries stay."""
    sc = DelScene()
    good = sc.want()
    bad = sc.blocks.copy()
    bad[0] = (0, PAD_L + 1, 1)                        # b > padded_len
    bad[1] = (TW, 2 * TW, 10 ** 10 - TW + 1)          # a printed position of 11 digits
    bad[3] = (3 * TW, 3 * TW - 1, 1)                  # b < a
    lens, tn, got, _ = run_format(sc, blocks=bad, shift=3)
    assert lens.tolist()[:5] == [0] * 5 and tn.tolist()[:5] == [0] * 5 and got[:3] == b"\xEE" * 3
    assert got[3:-64] == b"".join(good[5:]) and got[-64:] == b"\xEE" * 64     # (the two blocks left as they were)
    cut = sc.blocks.copy()
    cut[0] = (64, 101, 65)                            # a block inside its tile: the slots outside it are skipped
    check_format(sc, blocks=cut)
    assert sc.want(blocks=cut)[0].count(b"\n") == 3       # (the three events at 100; the ladder lies below 64)
    # tile ranges that are no ranges: negative, decreasing, past the entries
    n = sc.n_rows
    lens, tn, got, _ = run_format(sc, tstart=[-1, 5, 3, n + 1, n + 2, n + 3, n + 2, n + 5])
    assert lens.tolist() == [0] * 7 and tn.tolist() == [0] * 7 and got == b"\xEE" * len(got)
    lens, tn, got, _ = run_format(sc, n_ent=10)      # fewer entries than the tiles hold: every range past them is refused
    assert lens.tolist() == [0] * 7 and tn.tolist() == [0] * 7 and got == b"\xEE" * len(got)
    # offs that do not match: a range 7 bytes short, one 5 bytes long, one that is none
    room = [len(good[0]) + 5, len(good[1]) - 9000, 0, len(good[3]) - 7, 0, len(good[5]), 0]
    offs = np.concatenate([[0], np.cumsum(room)]) + 100
    total = int(offs[-1])
    lens, tn, got, _ = run_format(sc, offs=offs, dst_len=total)
    assert got[:100] == b"\xEE" * 100 and got[total:] == b"\xEE" * 64
    assert got[offs[0]:offs[1]] == good[0] + b"\xEE" * 5 and got[offs[1]:offs[2]] == good[1][:-9000] and got[offs[3]:offs[4]] == good[3][:-7]
    assert got[offs[5]:offs[6]] == good[5] and offs[6] == offs[7]                          # (tile 6: a range of no byte)
    offs_bad = np.array([50, 40, -5, 10, total + 200, total + 300, total + 400, total + 350], dtype=np.int64)
    lens, tn, got, _ = run_format(sc, offs=offs_bad, dst_len=total)
    assert got == b"\xEE" * len(got)


IMAGE = 24 * 1024 - 16   # bytes of a step's lines that still leave through the LDS image


class SwitchScene(DelScene):
    """One tile whose 80 events are one step of k_dels_write: lines of 307 bytes (a name of 290
    characters, starts and ends of two digits, a coverage of three), IMAGE bytes in all: the last
    step that leaves through the LDS image.  With over = 1 the last event's reads have two digits:
    one byte more, the first step that goes out byte by byte."""

    def __init__(self, over):
        self.events = {(g, 1): (1, 0) for g in range(80)}
        if over:
            self.events[(79, 1)] = (10, 0)
        self.skipped = {}
        self.names = [b"N" * 290]
        self.tile_ref = [0]
        self.blocks = np.array([(0, TW, 10)], dtype=np.int64)
        self.counts = np.zeros((6, PAD_L), dtype=np.uint32)
        self.counts[:, :80] = 20
        self.wtile = np.full(PAD_L // 32, 0xFFFFFFFF, dtype=np.uint32)
        self.wtile[:TW // 32] = 0
        rows = [(g, ln, n, d) for (g, ln), (n, d) in self.events.items()]
        self.n_slots = 256
        self.slots = np.zeros((self.n_slots, 4), dtype=np.uint32)
        self.slots[np.random.RandomState(11).permutation(self.n_slots)[:len(rows)]] = np.array(rows, dtype=np.uint32)
        self.n_rows = len(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_format_at_the_image_switch(over):
    """A step of exactly the image's capacity and one of a byte more, dst shifted by 0 and by 15
    (the image then ends at its last byte): the same text either way, the guard bytes untouched."""
    sc = SwitchScene(over)
    want = sc.want()
    assert len(want) == 1 and want[0].count(b"\n") == 80 and len(want[0]) == IMAGE + over
    assert want[0].startswith(b"N" * 290 + b"\t10\t10\t1\t1\t0\t120\n")
    assert want[0].endswith(b"N\t89\t89\t1\t%d\t0\t120\n" % (10 if over else 1))
    text = check_format(sc)
    assert text == want[0] and check_format(sc, shift=15) == text


@pytest.mark.gpu
def test_collect_guards_and_the_overflow_word():
    """s2c_dels_collect on a real batch with tables of its own: two slots for four distinct events
    set the overflow word and store nothing outside the table; padded_len 20 clamps the events;
    a table of enough slots holds them all."""
    import torch
    from sam2consensus_amd import _lib
    from sam2consensus_amd.batch import parse_text
    from sam2consensus_amd.engine import DeviceBatch
    lib = _lib.lib
    hb = parse_text(_issue_sam())
    db = DeviceBatch(hb)
    i = hb.info
    Lp = int(i.padded_len)
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(lib.s2c_dels_count(_ptr(db.pc), _ptr(db.ops), int(i.n_pieces), int(i.n_ops), Lp, _ptr(total), _stream()))
    assert int(total.item()) == 7   # 3 + 1 + 2 + 1 events, four distinct

    def collect(ns, pl):
        buf = torch.full((4 * ns + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        body = buf[4:-4]
        body.zero_()
        over = torch.zeros(4, dtype=torch.int32, device="cuda")
        _lib.check(lib.s2c_dels_collect(_ptr(db.pc), _ptr(db.ops), _ptr(db.bq), _ptr(db.bx), int(i.n_pieces), int(i.n_ops), int(i.n_qwords),
                                        1, 150, pl, _ptr(body), ns, _ptr(over), _stream()))
        torch.cuda.synchronize()
        assert buf[:4].tolist() == [0x5A5A5A5A] * 4 and buf[-4:].tolist() == [0x5A5A5A5A] * 4 and over[1:].tolist() == [0, 0, 0]
        rows = body.cpu().numpy().view(np.uint32).reshape(ns, 4)
        return sorted(tuple(int(v) for v in r) for r in rows if r[1]), int(over[0])

    g2 = int(hb.ref_off[1])
    full = [(14, 3, 4, 1), (14, 4, 1, 0), (27, 160, 1, 1), (g2 + 7, 1, 1, 0)]
    assert collect(16, Lp) == (full, 0) and collect(4, Lp) == (full, 0)
    rows, over = collect(2, Lp)
    assert over == 1 and len(rows) == 2 and set(r[:2] for r in rows) <= set(r[:2] for r in full)
    assert collect(1, Lp)[1] == 1
    assert collect(16, 20) == ([(14, 3, 4, 1), (14, 4, 1, 0)], 0) and collect(16, 16) == ([(14, 2, 5, 1)], 0)   # clamped: 3D and 2D1I2D meet


# ---------------------------------------------------------------------------- GPU tier: end to end
CHUNK = 100
FIRSTS = list(range(0, len(CASES), CHUNK))


@functools.lru_cache(maxsize=None)
def _golden_model(idx):
    return _model_text(CASES[idx]["sam"], CASES[idx]["args"])


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRSTS)
def test_golden_cases_with_deletions(first):
    """run_text(..., --deletions) on every golden case, CHUNK to a test: the case's status; on ok
    the reference's FASTA files and the model's deletion table; every tenth case with all six
    tables beside it, and those tables as without the flag."""
    from sam2consensus_amd.cli import run_text
    six = ["--counts", "--variants", "--depth", "--lowcov", "--insertions", "--links", "--min-alt-reads", "1", "--min-alt-frac", "0.1"]
    for idx in range(first, min(first + CHUNK, len(CASES))):
        case = CASES[idx]
        status, files = run_text(case["sam"], list(case["args"]) + ["--deletions"])
        assert status == case["status"], case["name"]
        if status != "ok":
            assert files == {}, case["name"]
            continue
        assert {k: v for k, v in files.items() if k.endswith(".fasta")} == case["files"], case["name"]
        want = {o.parse_argv(["-i", "in.sam"] + list(case["args"])).prefix + ".deletions.tsv": _golden_model(idx)}
        assert {k: v for k, v in files.items() if not k.endswith(".fasta")} == want, case["name"]
        if idx % 10 == 0:
            _, base = run_text(case["sam"], list(case["args"]) + six)
            _, both = run_text(case["sam"], list(case["args"]) + six + ["--deletions"])
            assert list(both) == list(base) + list(want) and {k: v for k, v in both.items() if k not in want} == base, case["name"]
            assert {k: both[k] for k in want} == want, case["name"]


def _walk_events(hb):
    """{(g, len): [reads, dropped]} from a numpy walk of hb.pc / hb.ops: every piece that is not
    one M token, its D / N / P parts inside [ka, kb) merged when they touch."""
    from sam2consensus_amd import _lib
    active, maxdel = getattr(hb, "maxdel_active", True), getattr(hb, "maxdel", 150)
    pc = hb.pc.astype(np.int64)
    n = int(hb.info.n_pieces)
    fl = pc[:n, 3] >> 24
    events = {}
    for i in np.flatnonzero((fl & _lib.S2C_PF_SIMPLE) == 0).tolist():
        gpos, qh, o0, w3 = (int(v) for v in pc[i])
        oend, slen, f = int(pc[i + 1, 2]), w3 & 0xFFFFFF, w3 >> 24
        ka, kb = 0, 1 << 62
        if f & _lib.S2C_PF_RANGE:
            ka, kb = int(hb.ops[o0]), int(hb.ops[o0 + 1])
            o0 += 2
        if f & _lib.S2C_PF_INS:
            o0 += 3
        toks = [(int(w) & 15, int(w) >> 4) for w in hb.ops[o0:oend]]
        dashes, start, k, parts = 0, 0, 0, []
        for op, ln in toks:
            if op in bm.OP_BASES:
                take = max(0, min(ln, slen - start))
                if take and f & _lib.S2C_PF_X:
                    dashes += int((bm.plane_codes(hb, 16 * qh + start, take) == 5).sum())
                k += take
                start += ln
            elif op in bm.OP_DASH:
                s, e = max(k, ka), min(k + ln, kb)
                if e > s:
                    parts.append((gpos + s - ka, e - s))
                dashes += ln
                k += ln
            elif op in (1, 4):
                start += ln
        drop = bool(active and dashes > maxdel)
        merged = []
        for g, ln in parts:
            if merged and merged[-1][0] + merged[-1][1] == g:
                merged[-1][1] += ln
            else:
                merged.append([g, ln])
        for g, ln in merged:
            e = events.setdefault((g, ln), [0, 0])
            e[0] += 1
            e[1] += int(drop)
    return events


DEL_KINDS = [("c2", {"n_refs": 18, "long_del_frac": 0.2}), ("c5nd", {"ref_len": 400_000, "long_del_frac": 0.05}),
             ("c4", {"ref_len": 2000, "depth": 12000.0, "del_frac": 0.02, "del_max": 5, "long_del_frac": 0.1})]


@pytest.mark.gpu
@pytest.mark.parametrize("name,over", DEL_KINDS, ids=["c2", "c5", "c4"])
def test_every_tile_kind(name, over):
    """General tiles (c2), dense tiles (c5), deep tiles under 12,000 reads (c4), each with reads
    over -d (the generator's long_del_frac): the deletion table == the numpy walk of the pieces
    with the batch model's coverage, after the FASTA files, which equal the fused route's."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch(name, **over)
    if name == "c5nd":
        assert hb.info.n_dense > 0
    plain = consensus_batch(hb, [0.25, 0.75], b"x")
    both = consensus_batch(hb, [0.25, 0.75], b"x", deletions=1)
    assert plain and list(both) == list(plain) + [b"x.deletions.tsv"]
    for k, v in plain.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
    events = _walk_events(hb)
    cov = bm.model_counts(hb).sum(axis=0)
    off = np.asarray(hb.ref_off, dtype=np.int64)
    per_ref, covs = {nm: {} for nm in hb.names}, {}
    for (g, ln), v in events.items():
        r = int(np.searchsorted(off, g, side="right") - 1)
        per_ref[hb.names[r]][(g - int(off[r]), ln)] = v
    for r, nm in enumerate(hb.names):
        covs[nm] = cov[int(off[r]):int(off[r]) + int(hb.ref_len[r])]
    want = DEL_HEADER + table.format_deletions(per_ref, covs)
    got = both[b"x.deletions.tsv"]
    assert got == want, tt._first_diff(got, want)
    assert len(events) > 100 and any(v[1] > 0 for v in events.values()), "the configuration must hold events, some of dropped reads"
    assert consensus_batch(hb, [0.75], b"x", min_depth=7, fill=b"N", nchar=60, deletions=1)[b"x.deletions.tsv"] == got   # (-c, -m, -f, -n change nothing)
    three = consensus_batch(hb, [0.25], b"x", deletions=3)[b"x.deletions.tsv"]
    assert three == DEL_HEADER + table.format_deletions(per_ref, covs, 3) and three != got


@pytest.mark.gpu
def test_workspace_reuse():
    """run_with_tables(deletions=...) twice on one workspace: the same bytes and FASTA results;
    beside other tables those are unchanged; deletions_table raises before the counts are filled."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.engine import DeviceBatch, Workspace

    def fetched(ws):
        stats, offs, out = ws.fetch()
        return stats.tobytes(), offs.tobytes(), bytes(out)

    hb = configs.synth_batch("c2", n_refs=6)
    ws0 = Workspace(DeviceBatch(hb), [0.25])
    ws0.run()
    base = fetched(ws0)
    ws = Workspace(DeviceBatch(hb, dense_layers=True), [0.25], keep_counts=True)
    with pytest.raises(ValueError):
        ws.deletions_table()
    runs = []
    for _ in range(2):
        res = ws.run_with_tables({}, deletions=1)
        assert set(res) == {"deletions"}
        offs, text = res["deletions"]
        assert len(offs) == hb.info.n_tiles + 1 and int(offs[-1]) == text.numel()
        runs.append((offs.tobytes(), text.cpu().numpy().tobytes(), fetched(ws)))
    assert runs[0] == runs[1] and runs[0][2] == base and runs[0][1].count(b"\n") > 100
    alone = ws.run_with_tables({"counts": (), "links": (1, 8, 0.0, 1)})
    beside = ws.run_with_tables({"counts": (), "links": (1, 8, 0.0, 1)}, deletions=True)
    assert list(beside) == ["counts", "links", "deletions"] and fetched(ws) == base
    for k in alone:
        assert beside[k][1].cpu().numpy().tobytes() == alone[k][1].cpu().numpy().tobytes()
    assert beside["deletions"][1].cpu().numpy().tobytes() == runs[0][1]
    two = ws.run_with_tables({}, deletions=2)["deletions"][1].cpu().numpy().tobytes()
    assert 0 < two.count(b"\n") < runs[0][1].count(b"\n")
    with pytest.raises(ValueError):
        ws.run_with_tables({}, deletions=0)
    assert table.deletions_file(hb, b"x", offs, runs[0][1]) == {b"x.deletions.tsv": DEL_HEADER + runs[0][1]}


@pytest.mark.gpu
def test_cli_process(tmp_path):
    """sam2consensus.py on a C1-sized file with --deletions beside --counts and --links: one
    c1.deletions.tsv equal to the model's, announced last, after the link tables' lines and
    before Done.; everything else as without the flag."""
    import subprocess
    import sys
    from sam2consensus_amd import configs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sam = str(tmp_path / "c1.sam")
    configs.synth_write("c1", sam, depth=100.0, del_frac=0.2, del_max=2, long_del_frac=0.1)
    want = _model_text(open(sam).read(), ["-c", "0.25", "-p", "c1"], 2)
    assert want.count("\n") > 10 and all(int(ln.split("\t")[4]) >= 2 for ln in want.split("\n")[1:-1])
    every = _model_text(open(sam).read(), ["-c", "0.25", "-p", "c1"])
    assert every.count("\n") > want.count("\n") and any(ln.split("\t")[5] != "0" for ln in every.split("\n")[1:-1])
    outs = {}
    for tag, extra in (("base", ["--links", "--counts"]), ("every", ["--deletions", "--links", "--counts", "--min-del-reads", "2"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(root, "sam2consensus.py"), "-i", sam, "-o", str(out), "-c", "0.25"] +
                           extra, capture_output=True, text=True, timeout=240, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (r.stdout.replace(str(out), "OUT").split("\n"), {fn: open(os.path.join(out, fn), "rb").read() for fn in os.listdir(out)})
    head, base = outs["base"]
    so, files = outs["every"]
    k = so.index("Done.")
    assert so[k - 1] == "Deletion table saved in: OUT/c1.deletions.tsv" and so[k - 2].startswith("Link table saved for ")
    assert so[:k - 1] + so[k:] == head and not any("Deletion" in ln for ln in head)
    assert {fn: v for fn, v in files.items() if fn != "c1.deletions.tsv"} == base and len(files) == len(base) + 1
    assert files["c1.deletions.tsv"].decode() == want
