"""--links: allele pairs across neighbouring mixed sites (sam2consensus_amd/table.py, csrc/s2c_links.hip).

Without a GPU: a literal file for a hand-written SAM, the order of the pairs and the longest
line, the model against a restatement on every golden case (observations per read from the
oracle's parsecigar and the :210-218 loop, summing to the oracle's counts), the flags and their
refused combinations, the bindings.  On the GPU: the count kernel through run_text on
hand-written SAM texts (mask word and tile edges, S / I / D between the sites, '-' from D and
from SEQ, the maxdel rule, the POS 0 wrap, a long N skip, a short SEQ, 10,000 contended adds,
two references, --min-link-reads), the format kernels alone on a synthetic mask, rank and pairs
(the digit ladder, 1 and 36 pairs, ties, empty and full blocks, a pair into a later block,
shifted dst; the guards), the golden cases end to end, every tile kind against the batch model,
a reused workspace, all six tables at once, and the CLI process on a C1-sized file.  Every
comparison is exact."""
import functools
import os

import numpy as np
import pytest

import batch_model as bm
from devmem import _ptr, _stream
import s2c_oracle as o
import test_table as tt

from sam2consensus_amd import table

CASES = tt.CASES
LINKS_HEADER = b"pos1\tpos2\treads\thaps\tpairs\n"
SYM = "-ACGNT"
RULE = (2, 0.05)              # --min-alt-reads, --min-alt-frac: the defaults
GOLD_RULE = (1, 0.1)          # the golden cases' (their coverage is low)
GOLD_ARGS = ["--links", "--min-alt-reads", "1", "--min-alt-frac", "0.1"]


# ---------------------------------------------------------------------------- expectations
def _observations(sam_text, args):
    """(refs, counts, {ref: fragments}, opt) of a SAM text: per read the oracle's parsecigar and
    the loop of :210-218 restated — seqout char k lands on index POS-1+k, a negative index on
    the reference's end, a '-' of a read over -d nowhere.  A read is one fragment, or two around
    the wrap: the chars at negative indices and the others."""
    opt = o.parse_argv(["-i", "in.sam"] + list(args))
    lines = o._lines(sam_text)
    refs = o.read_header(lines)
    counts, _ = o.pileup(lines, refs, opt)
    frags = {r: [] for r in refs}
    for line in lines:
        if line[0] == "@":
            continue
        f = line.split("\t")
        if f[5] == "*":
            continue
        rname = o.py2_split(f[2])[0]
        pos = o.py2_int(f[3]) - 1
        seqout, _ = o.parsecigar(f[5], f[9], pos)
        ln = refs[rname]
        drop = opt.maxdel_active and seqout.count("-") > opt.maxdel
        wrapped, straight = [], []
        for ch in seqout:
            if not (drop and ch == "-"):
                (wrapped if pos < 0 else straight).append((pos + ln if pos < 0 else pos, ch))
            pos += 1
        frags[rname] += [wrapped, straight]
    return refs, counts, frags, opt


def _sites(counts_ref, min_cov, rule):
    return np.flatnonzero(table.site_mask(tt._c6(counts_ref), min_cov, *rule)).tolist()


def _model_files(sam_text, args, rule=RULE, min_reads=1):
    """({file name: content}, [n[6][6] of every pair]) through the model: one table per reference
    with Σcoverage > 0."""
    refs, counts, frags, opt = _observations(sam_text, args)
    files, every = {}, []
    for r in refs:
        if sum(sum(c) for c in counts[r]) == 0:
            continue
        sites = _sites(counts[r], max(opt.min_depth, 1), rule)
        pairs = table.link_pairs(frags[r], sites)
        every += list(pairs.values())
        files[r + "__" + opt.prefix + ".links.tsv"] = (LINKS_HEADER + table.format_links(pairs, sites, 1, min_reads)).decode()
    return files, every


@functools.lru_cache(maxsize=None)
def _golden_model(idx):
    return _model_files(CASES[idx]["sam"], CASES[idx]["args"], GOLD_RULE)


def _restated(frags, sites, min_reads=1):
    """The definition restated: for neighbours p1 < p2 the fragments that observe both, as a
    dict "XY" → n, printed through sorted() with an explicit key."""
    lines = []
    seen = [dict(obs) for obs in frags]
    for p1, p2 in zip(sites, sites[1:]):
        n = {}
        for d in seen:
            if p1 in d and p2 in d:
                n[d[p1] + d[p2]] = n.get(d[p1] + d[p2], 0) + 1
        if n and sum(n.values()) >= min_reads:
            order = sorted(n, key=lambda xy: (-n[xy], SYM.index(xy[0]), SYM.index(xy[1])))
            lines.append("\t".join([str(p1 + 1), str(p2 + 1), str(sum(n.values())), str(len(n)),
                                    ",".join(xy + ":" + str(n[xy]) for xy in order)]) + "\n")
    return "".join(lines).encode()


def _seq(start, n, subs, bg="A"):
    """SEQ of n chars for a read whose first char lands on 1-based position start: bg, with
    subs {1-based position: char}."""
    s = [bg] * n
    for p, ch in subs.items():
        s[p - start] = ch
    return "".join(s)


def _read(name, ref, pos, cigar, seq):
    return "%s\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (name, ref, pos, cigar, seq)


def _haps(ref, pos, n, haps, tag="r"):
    """Reads of n M from 1-based pos: (copies, subs) per haplotype."""
    out = ""
    for h, (copies, subs) in enumerate(haps):
        for k in range(copies):
            out += _read("%s%d_%d" % (tag, h, k), ref, pos, "%dM" % n, _seq(pos, n, subs))
    return out


# ---------------------------------------------------------------------------- CPU tier
def _issue_sam():
    sam = "@SQ\tSN:g1\tLN:400\n"
    sam += _haps("g1", 110, 61, [(12, {120: "A", 161: "C"}), (9, {120: "G", 161: "T"})], "s")
    sam += _haps("g1", 155, 191, [(4, {161: "C", 340: "A"}), (2, {161: "T", 340: "G"})], "l")
    sam += _read("d0", "g1", 155, "185M1D5M", _seq(155, 190, {161: "T"}))
    return sam


ISSUE_TABLE = ("pos1\tpos2\treads\thaps\tpairs\n"
               "120\t161\t21\t2\tAC:12,GT:9\n"
               "161\t340\t7\t3\tCA:4,TG:2,T-:1\n")


def test_constants():
    assert (table.LINKS_HEADER, table.LINKS_SUFFIX) == (LINKS_HEADER, b".links.tsv")


def test_hand_written_literal():
    """The issue's example: two haplotypes over 120 and 161, seven longer reads over 161 and
    340, one of them with a deletion at 340."""
    files, every = _model_files(_issue_sam(), [])
    assert files == {"g1__in.links.tsv": ISSUE_TABLE}
    assert len(every) == 2
    assert _model_files(_issue_sam(), [], min_reads=8)[0] == {"g1__in.links.tsv": ISSUE_TABLE[:ISSUE_TABLE.index("161\t340")]}
    assert _model_files(_issue_sam(), [], min_reads=22)[0] == {"g1__in.links.tsv": LINKS_HEADER.decode()}


def test_order_and_longest_line():
    """Equal counts are ordered by (s1, s2) in -ACGNT order.  All 36 pairs at 4294967295 on the
    last two printable positions give the longest line: 542 bytes — 10 + 1 + 10 + 1 + 12 + 1 + 2 +
    1 + 36·13 + 35 + 1, the reads field being Σ n = 154618822620, twelve digits (the issue counted
    ten for it and so 540; with every count at ten digits the sum cannot have fewer than eleven)."""
    n = [[0] * 6 for _ in range(6)]
    for a, b, v in ((5, 5, 2), (0, 1, 2), (1, 0, 2), (0, 0, 2), (4, 5, 7), (1, 5, 2)):
        n[a][b] = v
    assert table.format_links({0: n}, [3, 9]) == b"4\t10\t17\t6\tNT:7,--:2,-A:2,A-:2,AT:2,TT:2\n"
    assert table.format_links({0: n}, [3, 9], 1, 17) != b"" and table.format_links({0: n}, [3, 9], 1, 18) == b""
    full = [[4294967295] * 6 for _ in range(6)]
    line = table.format_links({0: full}, [0, 1], 9999999998)
    assert len(line) == 542 and line.startswith(b"9999999998\t9999999999\t154618822620\t36\t--:4294967295,-A:4294967295,")
    assert line.endswith(b",TT:4294967295\n") and line.count(b",") == 35
    with pytest.raises(ValueError):
        table.format_links({0: n}, [3, 9], 1, 0)
    # only neighbours pair, and only through consecutive observations
    pairs = table.link_pairs([[(1, "A"), (5, "C"), (9, "G")], [(1, "A"), (9, "T")], [(5, 2), (9, 5)]], [1, 5, 9])
    assert sorted(pairs) == [0, 1] and pairs[0][1][2] == 1 and pairs[1][2][3] == 1 and pairs[1][2][5] == 1
    assert sum(map(sum, pairs[0])) == 1 and sum(map(sum, pairs[1])) == 2


def test_model_against_the_restatement_on_every_ok_case():
    lines = multi = dash = cases = wrapped = 0
    for idx, case in enumerate(CASES):
        if case["status"] != "ok":
            continue
        refs, counts, frags, opt = _observations(case["sam"], case["args"])
        for r, ln in refs.items():
            summed = [[0] * 6 for _ in range(ln)]
            for obs in frags[r]:
                assert [p for p, _ in obs] == sorted({p for p, _ in obs}), (case["name"], r)   # rising inside a fragment
                for p, ch in obs:
                    summed[p][SYM.index(ch)] += 1
            assert summed == [list(c) for c in counts[r]], (case["name"], r)
            wrapped += sum(1 for k in range(0, len(frags[r]), 2) if frags[r][k])
            sites = _sites(counts[r], max(opt.min_depth, 1), GOLD_RULE)
            pairs = table.link_pairs(frags[r], sites)
            for mr in (1, 2):
                assert table.format_links(pairs, sites, 1, mr) == _restated(frags[r], sites, mr), (case["name"], r)
        files, every = _golden_model(idx)
        cases += bool(every)
        for n in every:
            lines += 1
            multi += sum(v != 0 for row in n for v in row) >= 2
            dash += any(n[a][b] for a in range(6) for b in range(6) if a == 0 or b == 0)
    assert lines >= 100 and multi >= 10 and dash >= 1 and cases >= 20 and wrapped >= 1, (lines, multi, dash, cases, wrapped)


def test_parser_has_the_flags(capsys):
    from sam2consensus_amd.cli import build_parser, links_of, variants_of
    p = build_parser()
    a = p.parse_args(["-i", "x.sam"])
    assert a.links is False and a.min_link_reads is None and links_of(p, a) is None and variants_of(p, a) is None
    assert links_of(p, p.parse_args(["-i", "x.sam", "--links"])) == (2, 0.05, 1)
    a = p.parse_args(["-i", "x.sam", "--links", "--min-link-reads", "3", "--min-alt-reads", "4", "--min-alt-frac", "0.2"])
    assert links_of(p, a) == (4, 0.2, 3) and variants_of(p, a) is None     # (--links alone writes no variant table)
    a = p.parse_args(["-i", "x.sam", "--links", "--variants", "--min-alt-reads", "4"])
    assert links_of(p, a) == (4, 0.05, 1) and variants_of(p, a) == (4, 0.05)
    a = p.parse_args(["-i", "x.sam", "--links", "--insertions", "--counts", "--depth", "--variants", "--lowcov"])
    assert a.links and a.insertions and a.counts and a.depth and a.variants and a.lowcov
    for argv, word in ((["--min-link-reads", "2"], "--min-link-reads needs --links"), (["--links", "--min-link-reads", "0"], "--min-link-reads"),
                       (["--links", "--min-link-reads", str(2 ** 32)], "--min-link-reads"), (["--links", "--min-alt-reads", "0"], "--min-alt-reads")):
        with pytest.raises(SystemExit) as e:
            links_of(p, p.parse_args(["-i", "x.sam"] + argv))
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert links_of(p, p.parse_args(["-i", "x.sam", "--links", "--min-link-reads", str(2 ** 32 - 1)]))[2] == 2 ** 32 - 1
    for opt in (["--min-alt-reads", "2"], ["--min-alt-frac", "0.1"]):   # with neither flag: today's message
        with pytest.raises(SystemExit) as e:
            variants_of(p, p.parse_args(["-i", "x.sam"] + opt))
        assert e.value.code == 2 and opt[0] + " needs --variants" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["-i", "x.sam", "--links", "--min-link-reads", "x"])
    h = p.format_help()
    assert "--links" in h and "--min-link-reads" in h and "REF__PREFIX.links.tsv" in h and "With --variants or --links" in h


@pytest.mark.parametrize("env,extra,word", [({"WORLD_SIZE": "2"}, ["--links"], "--links is not available with more than one process"),
                                            ({"S2C_STREAM": "1M"}, ["--links"], "--links is not available with streamed batches"),
                                            ({}, ["--links", "--min-link-reads", "0"], "--min-link-reads"),
                                            ({}, ["--min-link-reads", "2"], "--min-link-reads needs --links"),
                                            ({}, ["--min-alt-reads", "2"], "--min-alt-reads needs --variants")],
                         ids=["world2", "stream", "min0", "alone", "alt-alone"])
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


def test_links_symbols_declared_and_bound():
    from sam2consensus_amd import _lib
    lib = _lib.lib
    names = ["s2c_links_pop", "s2c_links_count", "s2c_links_len", "s2c_links_write"]
    assert set(names) <= set(_lib.EXPORTS) and lib.s2c_abi_version() == 14
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2c.h")).read()
    assert all("int " + n + "(" in header for n in names) and "k_links_*" in header
    assert [len(getattr(lib, f).argtypes) for f in names] == [4, 14, 11, 13]
    OK, ARG = _lib.S2C_OK, _lib.S2C_ERR_ARG   # (argument errors need no device)
    pop = lambda pl=0: lib.s2c_links_pop(None, pl, None, None)  # noqa: E731
    cnt = lambda npc=0, nq=0, pl=64, ns=1: lib.s2c_links_count(None, None, None, None, npc, nq, 1, 150, None, None, pl, ns, None, None)  # noqa: E731
    ln = lambda pl=64, ns=0, n=0, mr=1: lib.s2c_links_len(None, None, pl, None, ns, None, None, n, mr, None, None)  # noqa: E731
    wr = lambda pl=64, ns=0, n=0, mr=1, dl=0: lib.s2c_links_write(None, None, pl, None, ns, None, None, None, n, mr, None, dl, None)  # noqa: E731
    assert pop() == OK and pop(-1) == ARG and pop(64) == ARG
    assert cnt() == OK and cnt(npc=-1) == ARG and cnt(nq=-1) == ARG and cnt(pl=-1) == ARG and cnt(ns=2 ** 32) == ARG and cnt(npc=1) == ARG
    assert ln() == OK and ln(pl=-1) == ARG and ln(ns=-1) == ARG and ln(n=-1) == ARG and ln(mr=0) == ARG and ln(mr=2 ** 32) == ARG and ln(n=1) == ARG
    assert wr() == OK and wr(pl=-1) == ARG and wr(ns=2 ** 32) == ARG and wr(mr=0) == ARG and wr(dl=-1) == ARG and wr(n=1) == ARG


# ---------------------------------------------------------------------------- GPU tier: the count kernel through run_text
def _check_sam(sam, base=(), extra=(), rule=RULE, min_reads=1):
    """run_text(sam, base + --links + extra) == the model at `base`: the link files' contents."""
    from sam2consensus_amd.cli import run_text
    status, files = run_text(sam, list(base) + ["--links"] + list(extra))
    assert status == "ok"
    want, _ = _model_files(sam, base, rule, min_reads)
    got = {k: v for k, v in files.items() if not k.endswith(".fasta")}
    assert got == want, (got, want)
    return got


TWO_SITES = "@SQ\tSN:g1\tLN:100\n" + _haps("g1", 1, 30, [(3, {11: "C", 21: "G"}), (2, {11: "T", 21: "A"})])


def _body(*lines):
    return LINKS_HEADER.decode() + "".join(ln + "\n" for ln in lines)


@pytest.mark.gpu
def test_two_sites_in_one_mask_word_and_min_link_reads():
    assert _check_sam(TWO_SITES) == {"g1__in.links.tsv": _body("11\t21\t5\t2\tCG:3,TA:2")}
    assert _check_sam(TWO_SITES, extra=["--min-link-reads", "5"], min_reads=5) == {"g1__in.links.tsv": _body("11\t21\t5\t2\tCG:3,TA:2")}
    assert _check_sam(TWO_SITES, extra=["--min-link-reads", "6"], min_reads=6) == {"g1__in.links.tsv": _body()}
    # the rule of --variants: --min-alt-reads 3 leaves no site
    assert _check_sam(TWO_SITES, extra=["--min-alt-reads", "3"], rule=(3, 0.05)) == {"g1__in.links.tsv": _body()}


@pytest.mark.gpu
def test_sites_at_word_and_tile_edges():
    """Global bits 63 | 64 (two mask words) and 2047 | 2048 (two tiles); nobody spans 65 → 2048."""
    sam = "@SQ\tSN:g1\tLN:2200\n"
    sam += _haps("g1", 60, 10, [(3, {64: "C", 65: "G"}), (2, {64: "T", 65: "C"})], "a")
    sam += _haps("g1", 2040, 20, [(4, {2048: "G", 2049: "T"}), (3, {2048: "C", 2049: "G"})], "b")
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("64\t65\t5\t2\tCG:3,TC:2", "2048\t2049\t7\t2\tGT:4,CG:3")}


@pytest.mark.gpu
def test_second_site_two_tiles_on():
    """Tiles of 64 positions (the parser's tile width): the first site in tile 0, its partner in
    tile 2, the tile between without a site."""
    from sam2consensus_amd import _lib
    from sam2consensus_amd.batch import Parser
    from sam2consensus_amd.cli import consensus_batch
    sam = "@SQ\tSN:g1\tLN:400\n" + _haps("g1", 1, 160, [(3, {11: "C", 151: "G"}), (2, {11: "T", 151: "A"})])
    p = Parser(True, 150)
    try:
        _lib.check(_lib.lib.s2c_parser_set_tile_width(p._p, 64))
        p.feed(sam.encode())
        hb = p.finish()
    finally:
        p.close()
    assert hb.info.n_tiles >= 7 and [int(v) for v in hb.tiles[2, :2]] == [128, 192]
    files = consensus_batch(hb, [0.25], b"in", links=RULE + (1,))
    want, _ = _model_files(sam, [])
    assert {k.decode(): v.decode() for k, v in files.items() if not k.endswith(b".fasta")} == want
    assert want == {"g1__in.links.tsv": _body("11\t151\t5\t2\tCG:3,TA:2")}


@pytest.mark.gpu
def test_soft_clip_insertion_and_deletion_between_the_sites():
    sam = "@SQ\tSN:g1\tLN:100\n"
    for k, (x, y) in enumerate([("C", "G")] * 3 + [("T", "A")] * 2):
        seq = "TTT" + _seq(1, 10, {5: x}) + "GG" + "A" * 10 + _seq(24, 10, {30: y})
        sam += _read("r%d" % k, "g1", 1, "3S10M2I10M3D10M", seq)
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("5\t30\t5\t2\tCG:3,TA:2")}


def _deletion_sam():
    """Three reads C / G / T at 5 / 15 / 25, two with A at 15, and two whose 1D covers 15 and
    whose 151D further on takes them over the default -d."""
    sam = "@SQ\tSN:g1\tLN:600\n"
    sam += _haps("g1", 1, 40, [(3, {5: "C", 15: "G", 25: "T"}), (2, {5: "C", 15: "A", 25: "T"})])
    for k in range(2):
        sam += _read("d%d" % k, "g1", 1, "14M1D25M151D10M", _seq(1, 14, {5: "T"}) + _seq(16, 25, {25: "C"}) + "A" * 10)
    return sam


@pytest.mark.gpu
def test_deletion_over_a_site():
    """A D over a site is the symbol '-'."""
    sam = "@SQ\tSN:g1\tLN:100\n" + _haps("g1", 1, 30, [(3, {5: "C", 15: "G", 25: "T"})])
    for k in range(2):
        sam += _read("d%d" % k, "g1", 1, "14M1D15M", _seq(1, 14, {5: "T"}) + _seq(16, 15, {25: "C"}))
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("5\t15\t5\t2\tCG:3,T-:2", "15\t25\t5\t2\tGT:3,-C:2")}


@pytest.mark.gpu
def test_dropped_deletion_links_nothing_and_dash_d_keeps_it():
    """Over the default -d the two reads' '-' at 15 is not counted: they observe 5 and 25 but
    link nothing across 15.  With -d 5 (Python 2: a string, never exceeded) every dash counts."""
    got = _check_sam(_deletion_sam())
    assert got == {"g1__in.links.tsv": _body("5\t15\t5\t2\tCG:3,CA:2", "15\t25\t5\t2\tGT:3,AT:2")}
    kept = _check_sam(_deletion_sam(), base=["-d", "5"])
    assert kept == {"g1__in.links.tsv": _body("5\t15\t7\t3\tCG:3,CA:2,T-:2", "15\t25\t7\t3\tGT:3,-C:2,AT:2")}


@pytest.mark.gpu
def test_n_and_dash_in_seq():
    sam = "@SQ\tSN:g1\tLN:100\n" + _haps("g1", 1, 20, [(3, {5: "C", 10: "G"}), (2, {5: "N", 10: "-"})])
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("5\t10\t5\t2\tCG:3,N-:2")}


@pytest.mark.gpu
def test_pos_0_read_is_two_fragments():
    """POS 0: the first char lands on the reference's last position (:212's index -1), the rest
    from position 1 on.  The two parts link 1 → 6 but nothing to 50."""
    sam = "@SQ\tSN:g1\tLN:50\n"
    sam += _haps("g1", 1, 10, [(3, {1: "C", 6: "G"})], "a")
    sam += _haps("g1", 41, 10, [(3, {50: "C"})], "b")
    for k in range(2):
        sam += _read("w%d" % k, "g1", 0, "10M", "G" + _seq(1, 9, {1: "T", 6: "A"}))
    refs, counts, frags, _ = _observations(sam, [])
    assert counts["g1"][49][SYM.index("G")] == 2 and sum(1 for f in frags["g1"][::2] if f) == 2
    assert _sites(counts["g1"], 1, RULE) == [0, 5, 49]
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("1\t6\t5\t2\tCG:3,TA:2")}


@pytest.mark.gpu
def test_long_skip_with_sites_on_both_sides():
    """A 3,000-position N skip (a long piece): its dropped '-' link the two sides when no site
    lies under it, and nothing across a site under it; with -d 5 they are observations."""
    from sam2consensus_amd.batch import parse_text
    sam = "@SQ\tSN:g1\tLN:3200\n"
    for k, (x, y) in enumerate([("C", "G")] * 3 + [("T", "A")] * 2):
        sam += _read("n%d" % k, "g1", 1, "10M3000N10M", _seq(1, 10, {5: x}) + _seq(3011, 10, {3015: y}))
    hb = parse_text(sam)
    assert hb.info.n_long > 0
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("5\t3015\t5\t2\tCG:3,TA:2")}
    under = sam + _haps("g1", 1495, 10, [(3, {1500: "C"}), (2, {1500: "T"})], "u")
    assert _check_sam(under) == {"g1__in.links.tsv": _body()}
    kept = _check_sam(under, base=["-d", "5"])["g1__in.links.tsv"]
    assert "5\t1495\t5\t2\tC-:3,T-:2\n" in kept and "1504\t3015\t5\t2\t-G:3,-A:2\n" in kept and "1499\t1500\t10\t3\t--:5,AC:3,AT:2\n" in kept


@pytest.mark.gpu
def test_seq_shorter_than_the_cigar():
    """20M with ten bases of SEQ: the observations end with SEQ."""
    sam = "@SQ\tSN:g1\tLN:100\n" + _haps("g1", 1, 20, [(3, {5: "C", 15: "G"}), (2, {5: "T", 15: "A"})])
    for k in range(2):
        sam += _read("t%d" % k, "g1", 1, "20M", _seq(1, 10, {5: "T"}))
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("5\t15\t5\t2\tCG:3,TA:2")}


@pytest.mark.gpu
def test_ten_thousand_contended_adds_are_exact():
    sam = "@SQ\tSN:g1\tLN:100\n" + _haps("g1", 1, 30, [(5000, {11: "C", 21: "G"}), (5000, {11: "T", 21: "A"})])
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("11\t21\t10000\t2\tCG:5000,TA:5000")}


@pytest.mark.gpu
def test_no_line_crosses_two_references():
    """Sites at the last position of g1 and the first of g2 are neighbours in the mask."""
    sam = "@SQ\tSN:g1\tLN:70\n@SQ\tSN:g2\tLN:70\n"
    sam += _haps("g1", 61, 10, [(3, {65: "G", 70: "C"}), (2, {65: "A", 70: "T"})], "a")
    sam += _haps("g2", 1, 10, [(3, {1: "G", 6: "C"}), (2, {1: "A", 6: "T"})], "b")
    assert _check_sam(sam) == {"g1__in.links.tsv": _body("65\t70\t5\t2\tGC:3,AT:2"), "g2__in.links.tsv": _body("1\t6\t5\t2\tGC:3,AT:2")}
    one = "@SQ\tSN:g1\tLN:70\n@SQ\tSN:g2\tLN:70\n"
    one += _haps("g1", 61, 10, [(3, {70: "C"}), (2, {70: "T"})], "a") + _haps("g2", 1, 10, [(3, {1: "G"}), (2, {1: "A"})], "b")
    assert _check_sam(one) == {"g1__in.links.tsv": _body(), "g2__in.links.tsv": _body()}


# ---------------------------------------------------------------------------- GPU tier: the format kernels alone
DIGITS = [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [4294967295]
PAD_L = 2304 + 128 + 64 + 384
WIDE = 2496                 # reference C: 300 neighbouring sites of eight ten-digit pairs each


class LinkScene:
    """A hand-built mask, rank and pairs.  Reference A = [0, 2304): every position of [64, 128)
    a site (a block of sites only), none in [128, 192), the digit ladder from 200, all 36 pairs
    at 300, ties at 400, a site at 2000 whose partner 2250 lies in a later block; reference
    B = [2304, 2432) printed up to 9999999999 with the longest line on its last two positions and
    a first site whose predecessor is A's last one; reference C = [2496, 2880) with 300 sites side
    by side whose lines take about 150 bytes each, so that a step of 256 of them is more than the
    write kernel's LDS image holds and goes out byte by byte."""

    def __init__(self):
        rows = {}
        for k, g in enumerate(range(64, 128)):
            rows[g] = {(k % 6, (k // 6) % 6): k + 1}
        rows[127] = {(1, 2): 5, (3, 5): 5}                       # → 200, past the empty block
        for k, v in enumerate(DIGITS):
            rows[200 + 2 * k] = {(k % 6, 5 - k % 6): v}           # one pair each: 9, 10, ... 4294967295
        rows[300] = {(a, b): 4294967295 for a in range(6) for b in range(6)}
        rows[301] = {}                                           # reads 0: not listed
        rows[400] = {(5, 5): 3, (0, 0): 3, (2, 4): 3, (2, 1): 3, (4, 0): 9, (1, 1): 1, (0, 5): 1}
        rows[401] = {(1, 3): 1}
        rows[2000] = {(1, 1): 12, (3, 5): 9}                     # → 2250
        rows[2250] = {(2, 2): 4}                                 # → 2304 + 5: the next reference
        rows[2304 + 5] = {(0, 4): 2, (4, 0): 2}
        rows[2304 + 126] = {(a, b): 4294967295 for a in range(6) for b in range(6)}
        rows[2304 + 127] = {(1, 1): 7}                           # the last site: no partner
        for k in range(300):
            rows[WIDE + k] = {(j % 6, (k + j + 3 * (j // 6)) % 6): 4294967295 - 8 * k - j for j in range(8)}
        self.sites = sorted(rows)
        self.n6 = []
        for g in self.sites:
            n = [[0] * 6 for _ in range(6)]
            for (a, b), v in rows[g].items():
                n[a][b] = v
            self.n6.append(n)
        self.mask = np.zeros(PAD_L // 64, dtype=np.uint64)
        for g in self.sites:
            self.mask[g >> 6] |= np.uint64(1) << np.uint64(g & 63)
        pop = np.array([bin(int(w)).count("1") for w in self.mask], dtype=np.uint32)
        self.rank = np.concatenate([[0], np.cumsum(pop)]).astype(np.uint32)
        self.pairs = np.array(self.n6, dtype=np.uint32).reshape(-1, 36)
        self.blocks = np.array([(0, 64, 1), (64, 128, 65), (128, 192, 129), (192, 2240, 193), (2240, 2304, 2241),
                                (2304, 2432, 10 ** 10 - 128), (2432, 2432, 1), (WIDE, WIDE + 384, 1)], dtype=np.int64)
        self.refs = np.array([(0, 2304)] * 5 + [(2304, 2432)] + [(2432, 2496)] + [(WIDE, WIDE + 384)], dtype=np.int64)

    def want(self, min_reads=1, blocks=None, refs=None, n_sites=None):
        blocks = self.blocks if blocks is None else blocks
        refs = self.refs if refs is None else refs
        ns = len(self.sites) if n_sites is None else n_sites
        out = []
        for (a, b, p0), (s, e) in zip(blocks.tolist(), refs.tolist()):
            txt = b""
            if 0 <= s <= a <= b <= e <= PAD_L and 0 <= p0 <= 10 ** 10 - (e - a):
                pr = {k: self.n6[k] for k, g in enumerate(self.sites)
                      if a <= g < b and k < ns and k + 1 < len(self.sites) and self.sites[k + 1] < e}
                txt = table.format_links(pr, [g - a for g in self.sites], p0, min_reads)
            out.append(txt)
        return out


def _dev_u32(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    if a.size < 4:
        a = np.concatenate([a, np.zeros(4 - a.size, dtype=np.uint32)])
    return torch.from_numpy(a.view(np.int32)).cuda()


def run_format(sc, min_reads=1, blocks=None, refs=None, offs=None, dst_len=None, shift=0, n_sites=None):
    """(lens, dst bytes with 64 guard bytes behind, offs): s2c_links_len, the prefix sum,
    s2c_links_write; mask, rank and pairs are bit-identical after both calls."""
    import torch
    from sam2consensus_amd import _lib
    lib = _lib.lib
    blocks = sc.blocks if blocks is None else blocks
    refs = sc.refs if refs is None else refs
    ns = len(sc.sites) if n_sites is None else n_sites
    nb = len(blocks)
    mask = torch.from_numpy(sc.mask.view(np.int64)).cuda()
    rank, pairs = _dev_u32(sc.rank), _dev_u32(sc.pairs)
    before = [t.clone() for t in (mask, rank, pairs)]
    b, r = tt._dev_i64(blocks), tt._dev_i64(refs)
    lens = torch.full((nb,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.s2c_links_len(_ptr(mask), _ptr(rank), PAD_L, _ptr(pairs), ns, _ptr(b), _ptr(r), nb, min_reads, _ptr(lens), _stream()))
    lens = lens.cpu().numpy()
    if offs is None:
        offs = np.concatenate([[0], np.cumsum(lens)]) + shift
    total = int(offs[-1]) if dst_len is None else dst_len
    dst = torch.full((max(total, int(np.max(offs)), 0) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    f = tt._dev_i64(offs)
    _lib.check(lib.s2c_links_write(_ptr(mask), _ptr(rank), PAD_L, _ptr(pairs), ns, _ptr(b), _ptr(r), _ptr(f), nb, min_reads,
                                   _ptr(dst), total, _stream()))
    torch.cuda.synchronize()
    for t, t0 in zip((mask, rank, pairs), before):
        assert torch.equal(t, t0)
    return lens, dst.cpu().numpy().tobytes(), offs


def check_format(sc, min_reads=1, shift=0, **kw):
    want = sc.want(min_reads, **{k: v for k, v in kw.items() if k in ("blocks", "refs", "n_sites")})
    lens, got, offs = run_format(sc, min_reads, shift=shift, **kw)
    assert lens.tolist() == [len(w) for w in want], [(t, int(lens[t]), len(want[t])) for t in range(len(want)) if lens[t] != len(want[t])]
    total = int(offs[-1])
    assert got[:shift] == b"\xEE" * shift and got[total:] == b"\xEE" * 64
    for t, w in enumerate(want):
        assert got[offs[t]:offs[t + 1]] == w, (t, tt._first_diff(got[offs[t]:offs[t + 1]], w))
    return b"".join(want)


@pytest.mark.gpu
@pytest.mark.parametrize("min_reads", [1, 4, 2 ** 32 - 1])
def test_format_kernels_on_a_synthetic_scene(min_reads):
    sc = LinkScene()
    text = check_format(sc, min_reads)
    for shift in (1, 7, 15):
        assert check_format(sc, min_reads, shift=shift) == text
    want = sc.want(min_reads)
    assert want[0] == b"" and want[2] == b"" and want[6] == b""            # no site; a block of no site; an empty block
    wide = want[7].split(b"\n")[:-1]
    assert len(wide) == 299 and sum(len(ln) + 1 for ln in wide[:256]) > 32768 and all(ln.split(b"\t")[3] == b"8" for ln in wide)
    if min_reads == 1:
        assert want[1].count(b"\n") == 64 and want[1].startswith(b"65\t66\t1\t1\t--:1\n66\t67\t2\t1\tA-:2\n")
        assert want[1].endswith(b"128\t201\t10\t2\tAC:5,GT:5\n")            # over the empty block, ties by (s1, s2)
        for k, v in enumerate(DIGITS):
            assert b"\t%d\t1\t%s%s:%d\n" % (v, SYM[k % 6].encode(), SYM[5 - k % 6].encode(), v) in want[3]
        assert b"301\t302\t154618822620\t36\t--:4294967295,-A:4294967295," in want[3] and b"\n302\t401\t" not in want[3]
        assert b"401\t402\t23\t7\tN-:9,--:3,CA:3,CN:3,TT:3,-T:1,AA:1\n402\t2001\t1\t1\tAG:1\n" in want[3]
        assert want[3].endswith(b"2001\t2251\t21\t2\tAA:12,GT:9\n")         # the partner lies in the next block
        assert want[4] == b""                                               # 2250's partner is another reference's
        assert want[5].startswith(b"9999999877\t9999999998\t4\t2\t-N:2,N-:2\n9999999998\t9999999999\t154618822620\t36\t")
        assert len(want[5].split(b"\n")[1]) + 1 == 542 and want[5].count(b"\n") == 2
    if min_reads == 4:
        assert want[1].startswith(b"68\t69\t4\t1\tG-:4\n") and b"\n402\t" not in want[3] and b"\n401\t402\t23\t" in want[3]
    if min_reads == 2 ** 32 - 1:
        assert text.count(b"\n") == 3 + 299 and b"\t4294967295\t1\t-T:4294967295\n" in text


@pytest.mark.gpu
def test_format_guards():
    """Blocks outside the bounds, offs decreasing or past dst_len, ranks at or past n_sites: no
    byte is written, and the guard bytes around dst stay."""
    sc = LinkScene()
    good = sc.want()
    bad = sc.blocks.copy()
    bad[1] = (64, PAD_L + 1, 65)                      # b > padded_len (and > e)
    bad[3] = (192, 191, 193)                          # b < a
    bad[5] = (2304, 2432, 10 ** 10 - 127)             # a printed position of 11 digits
    bad_refs = sc.refs.copy()
    bad_refs[4] = (2241, 2304)                        # s > a
    bad_refs[7] = (WIDE, WIDE + 383)                  # e < b
    lens, got, offs = run_format(sc, blocks=bad, refs=bad_refs, shift=3)
    assert lens.tolist() == [0] * 8 and got == b"\xEE" * len(got)
    cut_refs = sc.refs.copy()
    cut_refs[3] = (0, 2250)                           # e at the partner: 2000 → 2250 is not listed
    check_format(sc, refs=cut_refs)
    assert sc.want(refs=cut_refs)[3] == good[3][:-len(b"2001\t2251\t21\t2\tAA:12,GT:9\n")]
    # ranks at or past n_sites are not listed (and their rows not read)
    for ns in (0, 1, 70, len(sc.sites) - 1):
        check_format(sc, n_sites=ns)
    assert sc.want(n_sites=0) == [b""] * 8 and sc.want(n_sites=1)[1] == b"65\t66\t1\t1\t--:1\n"
    # offs that do not match: a range 7 bytes short, one 5 bytes long, one that is none
    room = [0, len(good[1]) + 5, 0, len(good[3]) - 7, 0, len(good[5]), 0, len(good[7]) - 9000]
    offs = np.concatenate([[0], np.cumsum(room)]) + 100
    total = int(offs[-1])
    lens, got, _ = run_format(sc, offs=offs, dst_len=total)
    assert got[:100] == b"\xEE" * 100 and got[total:] == b"\xEE" * 64
    assert got[offs[1]:offs[2]] == good[1] + b"\xEE" * 5 and got[offs[3]:offs[4]] == good[3][:-7] and got[offs[5]:offs[6]] == good[5]
    assert got[offs[7]:offs[8]] == good[7][:-9000]       # (cut inside the lines that are stored byte by byte, and in the image's)
    offs_bad = np.array([50, 40, -5, 10, total + 200, total + 300, total + 400, total + 500, total + 600], dtype=np.int64)
    lens, got, _ = run_format(sc, offs=offs_bad, dst_len=total)
    assert got == b"\xEE" * len(got)


@pytest.mark.gpu
def test_count_guards():
    """s2c_links_count on a real batch with a rank table of its own: with n_sites below the true
    number the pairs past it get no add, and the words around pairs stay."""
    import torch
    from sam2consensus_amd import _lib
    from sam2consensus_amd.batch import parse_text
    from sam2consensus_amd.engine import DeviceBatch
    lib = _lib.lib
    sam = "@SQ\tSN:g1\tLN:100\n" + _haps("g1", 1, 40, [(3, {5: "C", 15: "G", 25: "T", 35: "C"}), (2, {5: "T", 15: "A", 25: "C", 35: "G"})])
    hb = parse_text(sam)
    db = DeviceBatch(hb)
    i = hb.info
    Lp = int(i.padded_len)
    mask = np.zeros((Lp + 63) // 64, dtype=np.uint64)
    for g in (4, 14, 24, 34):
        mask[g >> 6] |= np.uint64(1) << np.uint64(g & 63)
    rank = np.concatenate([[0], np.cumsum([bin(int(w)).count("1") for w in mask])]).astype(np.uint32)
    mask_d, rank_d = torch.from_numpy(mask.view(np.int64)).cuda(), _dev_u32(rank)
    full = None
    for ns in (4, 2, 1):
        pairs = torch.zeros(36 * 4 + 8, dtype=torch.int32, device="cuda")
        pairs[:4] = 0x5A5A5A5A
        pairs[-4:] = 0x5A5A5A5A
        body = pairs[4:-4]
        assert body.data_ptr() % 16 == 0
        for Lpad in (Lp, 20):    # (padded_len 20: the runs are clamped, sites 24 and 34 are not reached)
            body.zero_()
            _lib.check(lib.s2c_links_count(_ptr(db.pc), _ptr(db.ops), _ptr(db.bq), _ptr(db.bx), int(i.n_pieces), int(i.n_qwords), 1, 150,
                                           _ptr(mask_d), _ptr(rank_d), Lpad, ns, _ptr(body), _stream()))
            torch.cuda.synchronize()
            got = body.cpu().numpy().reshape(4, 6, 6)
            assert pairs[:4].tolist() == [0x5A5A5A5A] * 4 and pairs[-4:].tolist() == [0x5A5A5A5A] * 4
            if Lpad == Lp and ns == 4:
                full = got.copy()
                assert full[0, 2, 3] == 3 and full[0, 5, 1] == 2 and full[1, 3, 5] == 3 and full[2, 5, 2] == 3 and full.sum() == 15
                assert full[3].sum() == 0
            elif Lpad == Lp:
                assert (got[:ns - 1] == full[:ns - 1]).all() and got[ns - 1:].sum() == 0
            else:
                assert (got[0] == full[0]).all() == (ns >= 2) and got[1:].sum() == 0 and (ns >= 2 or got.sum() == 0)


# ---------------------------------------------------------------------------- GPU tier: end to end
CHUNK = 100   # golden cases per test: a run takes milliseconds, most of a test of one would be its set-up
FIRSTS = list(range(0, len(CASES), CHUNK))


@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRSTS)
def test_golden_cases_with_links(first):
    """run_text(..., --links) on every golden case, CHUNK to a test: the case's status; on ok the
    reference's FASTA files and a link table per reference with Σcoverage > 0, equal to the
    model's; with --counts and --variants beside it, those tables as without --links."""
    from sam2consensus_amd.cli import run_text
    for idx in range(first, min(first + CHUNK, len(CASES))):
        case = CASES[idx]
        status, files = run_text(case["sam"], list(case["args"]) + GOLD_ARGS)
        assert status == case["status"], case["name"]
        if status != "ok":
            assert files == {}, case["name"]
            continue
        assert {k: v for k, v in files.items() if k.endswith(".fasta")} == case["files"], case["name"]
        assert {k: v for k, v in files.items() if not k.endswith(".fasta")} == _golden_model(idx)[0], case["name"]
        if idx % 10 == 0:
            others = ["--counts", "--variants", "--min-alt-reads", "1", "--min-alt-frac", "0.1"]
            _, base = run_text(case["sam"], list(case["args"]) + others)
            _, both = run_text(case["sam"], list(case["args"]) + others + ["--links"])
            assert {k: v for k, v in both.items() if not k.endswith(".links.tsv")} == base, case["name"]
            assert {k: v for k, v in both.items() if k.endswith(".links.tsv")} == _golden_model(idx)[0], case["name"]


@functools.lru_cache(maxsize=4)
def _model_pairs(hb, rule):
    """(sites, pairs[n_sites][6][6]) from batch_model's piece walk: every run record against the
    sites of the model's counts, a piece's observations in the order of its op slots."""
    runs, _ = bm.model_reads(hb)
    sites = np.flatnonzero(table.site_mask(bm.model_counts(hb, runs), 1, *rule))
    r = runs.astype(np.int64)
    kind, ln = r[:, 1] >> bm.RUN_KSHIFT, r[:, 1] & ((1 << bm.RUN_KSHIFT) - 1)
    lo, hi = np.searchsorted(sites, r[:, 0]), np.searchsorted(sites, r[:, 0] + ln)
    slots = np.flatnonzero((hi > lo) & ((kind & 3) != 0))
    cnt = hi[slots] - lo[slots]
    j = np.repeat(slots, cnt)                                   # an observation's op slot
    k = np.repeat(lo[slots], cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)   # its site's rank
    piece = np.searchsorted(hb.pc[:hb.info.n_pieces + 1, 2].astype(np.int64), j, side="right") - 1
    bases = (kind[j] & 3) == bm.RUN_BASES
    q = np.where(bases, (r[j, 2] | (r[j, 3] << 32)) + sites[k] - r[j, 0], 0)
    w, sh = q >> 5, (q & 31).astype(np.uint32)
    code = ((hb.bx[w] >> sh) & 1).astype(np.int64) << 2 | ((hb.bq[w, 1] >> sh) & 1) << 1 | ((hb.bq[w, 0] >> sh) & 1)
    sym = np.where(bases, bm.CODE_SYM[code], 0)
    keep = ~(bases & (sym == 0) & ((kind[j] & bm.RUN_DROP) != 0))   # a dropped '-' of SEQ is no observation
    piece, k, sym = piece[keep], k[keep], sym[keep]
    link = (piece[1:] == piece[:-1]) & (k[1:] == k[:-1] + 1)
    pairs = np.zeros((len(sites), 6, 6), dtype=np.int64)
    np.add.at(pairs, (k[:-1][link], sym[:-1][link], sym[1:][link]), 1)
    return sites, pairs


def _model_links(hb, prefix, rule, min_reads=1):
    """{file: bytes} of the batch model's pairs; and the largest reads of a pair."""
    sites, pairs = _model_pairs(hb, rule)
    off = np.asarray(hb.ref_off, dtype=np.int64)
    out = {}
    for ref in range(hb.info.n_refs):
        if hb.ref_reads[ref] > 0:
            a, e = int(off[ref]), int(off[ref]) + int(hb.ref_len[ref])
            k0, k1 = np.searchsorted(sites, [a, e])
            pr = {k - k0: pairs[k].tolist() for k in range(k0, k1 - 1) if pairs[k].any()}
            out[hb.names[ref].encode() + b"__" + prefix + b".links.tsv"] = LINKS_HEADER + table.format_links(
                pr, (sites[k0:k1] - a).tolist(), 1, min_reads)
    return out, int(pairs.sum(axis=(1, 2)).max()) if len(sites) else 0


# (the rules: a site needs this many minority reads — c2 is 500 reads deep, c4 12,000, their
# minorities random substitutions of 1 %; c5 is 30 deep: the defaults)
LINK_KINDS = [("c2", {"n_refs": 18}, (8, 0.0)), ("c5", {"ref_len": 400_000}, (2, 0.05)),
              ("c4", {"ref_len": 2000, "depth": 12000.0}, (140, 0.0))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,over,rule", LINK_KINDS, ids=["c2", "c5", "c4"])
def test_every_tile_kind(name, over, rule):
    """General tiles (c2), dense tiles (c5), deep tiles under 12,000 reads (c4): the link tables
    == the batch model's piece walk against its own sites, after the FASTA files, which equal the
    fused route's."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch(name, **over)
    if name == "c5":
        assert hb.info.n_dense > 0
    plain = consensus_batch(hb, [0.25, 0.75], b"x")
    both = consensus_batch(hb, [0.25, 0.75], b"x", links=rule + (1,))
    nf = len(plain)
    assert plain and list(both)[:nf] == list(plain)
    for k, v in plain.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
    want, most = _model_links(hb, b"x", rule)
    assert list(both)[nf:] == list(want)
    for k, v in want.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
    assert sum(v.count(b"\n") - 1 for v in want.values()) > 0, "the configuration must hold pairs"
    if name == "c4":
        assert most > 1000, "the deep configuration must hold pairs with reads > 1000"


@pytest.mark.gpu
def test_workspace_reuse():
    """run_with_tables(links=...) twice on one workspace: the same bytes and FASTA results; the
    link tables beside the site tables of the same rule are what each gives alone; a plain run()
    on a fresh workspace is unchanged; links_table raises before anything filled the counts."""
    import torch
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
        ws.links_table()
    runs = []
    for _ in range(2):
        res = ws.run_with_tables({"links": (1, 8, 0.0, 1)})
        assert set(res) == {"links"}
        offs, text = res["links"]
        runs.append((offs.tobytes(), text.cpu().numpy().tobytes(), fetched(ws)))
    assert runs[0] == runs[1] and runs[0][2] == base
    want, _ = _model_links(hb, b"x", (8, 0.0))
    assert table.table_files(hb, b"x", offs, runs[0][1], table.LINKS_HEADER, table.LINKS_SUFFIX) == want
    alone = ws.run_with_tables({"variants": (1, 8, 0.0)})
    sites_text = alone["variants"][1].cpu().numpy().tobytes()
    six = ws.run_with_tables({"links": (1, 8, 0.0, 2), "insertions": (1,), "lowcov": (1,), "depth": (1,), "variants": (1, 8, 0.0),
                              "counts": ()})   # (the request's own order does not matter)
    assert list(six) == ["counts", "variants", "depth", "lowcov", "insertions", "links"] and fetched(ws) == base
    assert six["variants"][1].cpu().numpy().tobytes() == sites_text
    assert table.table_files(hb, b"x", six["links"][0], six["links"][1].cpu().numpy().tobytes(), table.LINKS_HEADER,
                             table.LINKS_SUFFIX) == _model_links(hb, b"x", (8, 0.0), 2)[0]
    other = ws.run_with_tables({"variants": (1, 8, 0.0), "links": (1, 12, 0.0, 1)})   # (two rules: two masks)
    assert list(other) == ["variants", "links"] and other["variants"][1].cpu().numpy().tobytes() == sites_text
    assert table.table_files(hb, b"x", other["links"][0], other["links"][1].cpu().numpy().tobytes(), table.LINKS_HEADER,
                             table.LINKS_SUFFIX) == _model_links(hb, b"x", (12, 0.0))[0]
    two = ws.run_with_tables({"counts": ()})
    assert set(two) == {"counts"} and fetched(ws) == base
    ws.accumulate(keep_tables=True)   # (onto the counts the vote left zero)
    with pytest.raises(ValueError):
        ws.links_table(1, 8, 0.0, 0)
    again = ws.links_table(1, 8, 0.0, 1)
    assert again[1].cpu().numpy().tobytes() == runs[0][1]
    ws.vote_all()
    ws1 = Workspace(DeviceBatch(hb), [0.25])
    ws1.run()
    assert fetched(ws1) == base
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_all_six_tables_equal_the_separate_runs():
    """--counts --variants --depth --lowcov --insertions --links in one run: every file what the
    run with its flag alone gives; the link tables come last, after the insertion tables."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch("c2", n_refs=3)
    kw = dict(min_depth=30)
    plain = consensus_batch(hb, [0.25], b"x", **kw)
    alone = [consensus_batch(hb, [0.25], b"x", counts=True, **kw), consensus_batch(hb, [0.25], b"x", variants=(1, 0.0), **kw),
             consensus_batch(hb, [0.25], b"x", depth=True, **kw), consensus_batch(hb, [0.25], b"x", lowcov=True, **kw),
             consensus_batch(hb, [0.25], b"x", insertions=1, **kw), consensus_batch(hb, [0.25], b"x", links=(1, 0.0, 1), **kw)]
    every = consensus_batch(hb, [0.25], b"x", counts=True, variants=(1, 0.0), depth=True, lowcov=True, insertions=1,
                            links=(1, 0.0, 1), **kw)
    order = list(plain)
    for files in alone:
        assert list(files)[:len(plain)] == list(plain) and len(files) > len(plain)
        order += list(files)[len(plain):]
    summary = order.pop(order.index(b"x.depth_summary.tsv"))
    tail = [k for k in order if k.endswith(b".insertions.tsv")] + [k for k in order if k.endswith(b".links.tsv")]
    assert len(tail) == 6
    assert list(every) == [k for k in order if k not in tail] + [summary] + tail
    for files in alone:
        for k, v in files.items():
            assert every[k] == v, (k, tt._first_diff(every[k], v))
    links = {k: v for k, v in every.items() if k.endswith(b".links.tsv")}
    assert all(v.count(b"\n") > 1 for v in links.values())
    assert consensus_batch(hb, [0.75], b"x", min_depth=30, fill=b"N", nchar=60, links=(1, 0.0, 1))[tail[-1]] == every[tail[-1]]   # (-c, -f, -n change nothing)
    assert consensus_batch(hb, [0.25], b"x", min_depth=1, links=(1, 0.0, 1))[tail[-1]] != every[tail[-1]]                        # (-m does: the sites)


@pytest.mark.gpu
def test_cli_process(tmp_path):
    """sam2consensus.py on a C1-sized file with --links beside --counts and --insertions: one
    .links.tsv per FASTA file, equal to the model's; the stdout lines in order, the link tables'
    last, after the insertion tables' and before Done.; everything else as without the flag."""
    import subprocess
    import sys
    from sam2consensus_amd import configs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sam = str(tmp_path / "c1.sam")
    configs.synth_write("c1", sam, depth=30.0, ins_frac=0.2, ins_max=6)
    want, every = _model_files(open(sam).read(), ["-c", "0.25", "-p", "c1"], (2, 0.0), 2)
    assert len(want) == 10 and sum(v.count("\n") - 1 for v in want.values()) > 10
    outs = {}
    for tag, extra in (("base", ["--insertions", "--counts"]),
                       ("every", ["--insertions", "--links", "--counts", "--min-alt-frac", "0", "--min-link-reads", "2"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(root, "sam2consensus.py"), "-i", sam, "-o", str(out), "-c", "0.25"] +
                           extra, capture_output=True, text=True, timeout=240, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (r.stdout.replace(str(out), "OUT").split("\n"), {fn: open(os.path.join(out, fn), "rb").read() for fn in os.listdir(out)})
    head, base = outs["base"]
    so, files = outs["every"]
    names = sorted(k[:-len("__c1.fasta")] for k in base if k.endswith(".fasta"))
    assert len(names) == 10 and not any("Link" in ln for ln in head)
    k = so.index("Done.")
    link_lines = so[k - 10:k]
    assert sorted(link_lines) == sorted("Link table saved for %s in: OUT/%s__c1.links.tsv" % (n, n) for n in names)
    assert so[k - 11].startswith("Insertion table saved for ")
    assert so[:k - 10] + so[k:] == head
    assert {fn: v for fn, v in files.items() if not fn.endswith(".links.tsv")} == base and len(files) == len(base) + 10
    assert {fn: v.decode() for fn, v in files.items() if fn.endswith(".links.tsv")} == want


@pytest.mark.gpu
def test_cli_process_all_six_flags(tmp_path, capsys):
    """sam2consensus.py with all six table flags in one process on the C1-sized file of
    test_cli_process: after the consensus lines and before Done. the stdout lines are the count,
    variant, depth and low-coverage tables' (ten each, in reference order), the one depth summary
    line, then the insertion and the link tables'; the folder holds the 10 FASTA files, 60 tables
    and the summary; every table file is what the run with its flag alone writes."""
    import subprocess
    import sys
    from sam2consensus_amd import configs
    from sam2consensus_amd.batch import parse_file
    from sam2consensus_amd.cli import main
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sam = str(tmp_path / "c1.sam")
    configs.synth_write("c1", sam, depth=30.0, ins_frac=0.2, ins_max=6)
    hb = parse_file(sam)
    names = list(hb.names)
    hb.free()
    assert len(names) == 10
    flags = ["--counts", "--variants", "--depth", "--lowcov", "--insertions", "--links"]
    out = tmp_path / "every"
    r = subprocess.run([sys.executable, os.path.join(root, "sam2consensus.py"), "-i", sam, "-o", str(out), "-c", "0.25"] +
                       flags + ["--min-alt-frac", "0"], capture_output=True, text=True, timeout=240, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    so = r.stdout.replace(str(out), "OUT").split("\n")
    groups = [("Count table", "counts.tsv"), ("Variant table", "variants.tsv"), ("Depth table", "depth.tsv"),
              ("Low-coverage table", "lowcov.tsv"), None, ("Insertion table", "insertions.tsv"), ("Link table", "links.tsv")]
    want = ["Consensus sequence at 25%% saved for %s in: OUT/%s__c1.fasta" % (n, n) for n in names]
    for g in groups:
        want += ["Depth summary saved in: OUT/c1.depth_summary.tsv"] if g is None else \
            ["%s saved for %s in: OUT/%s__c1.%s" % (g[0], n, n, g[1]) for n in names]
    first = so.index(want[0])
    assert so[first:] == want + ["Done.", "", ""]
    files = {fn: open(os.path.join(out, fn), "rb").read() for fn in os.listdir(out)}
    assert sorted(files) == sorted(["%s__c1.%s" % (n, g[1]) for g in groups if g for n in names] +
                                   [n + "__c1.fasta" for n in names] + ["c1.depth_summary.tsv"])
    assert len(files) == 71
    seen = set()
    for flag in flags:
        alone = tmp_path / flag[2:]
        rule = ["--min-alt-frac", "0"] if flag in ("--variants", "--links") else []
        assert main(["-i", sam, "-o", str(alone), "-c", "0.25", flag] + rule) == 0
        tables = [fn for fn in os.listdir(alone) if not fn.endswith(".fasta")]
        assert len(tables) == (11 if flag == "--depth" else 10)
        for fn in tables:
            assert files[fn] == open(os.path.join(alone, fn), "rb").read(), fn
        seen.update(tables)
    capsys.readouterr()
    assert len(seen) == 61
    assert sum(v.count(b"\n") - 1 for fn, v in files.items() if fn.endswith(".links.tsv")) > 10
