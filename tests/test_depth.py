"""--depth and --lowcov: the runs of equal coverage (sam2consensus_amd/table.py, csrc/s2c_runs.hip).

Without a GPU: the line formats literally, the models against a restatement with
itertools.groupby on every golden case, the numeric edges, the flags and their refused
combinations, the bindings.  On the GPU: the three kernels alone on synthetic counts (runs
across mask words, walk steps, blocks and many blocks, a 40,000-position run, runs that end at
their reference's end, 255 to 2,048 starts in a block, references of one position and with
equal or different coverage at their seam, the digit ladder; the same counts cut into blocks
four ways; the guards), the golden cases end to end, every tile kind against the batch model,
a reused workspace, all four tables at once, and the CLI process on C1."""
import hashlib
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import golden_io
import s2c_oracle as o
import test_table as tt
from devmem import _ptr, _stream

from sam2consensus_amd import table

CASES = tt.CASES
KAT = len(golden_io.load("kat"))
DEPTH_HEADER = b"start\tend\tcov\n"
LOWCOV_HEADER = b"start\tend\n"
SUMMARY_HEADER = b"ref\tlen\tcovered\tpassed\tsumcov\tmincov\tmaxcov\truns\n"
EMPTY = (0, 0, 0, 0, 2 ** 63 - 1, -1)


def _min_cov(case):
    return max(o.parse_argv(["-i", "in.sam"] + list(case["args"])).min_depth, 1)


def _summary_line(name, c, min_cov):
    runs, covered, passed, sumcov, mn, mx = table.depth_stats(c, min_cov)
    return "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, c.shape[1], covered, passed, sumcov, mn, mx, runs)


def _oracle_runs(idx):
    """{file name: content} the oracle's counts give: a depth and a low-coverage table per
    reference with Σcoverage > 0, and the summary."""
    refs, counts, prefix = tt._oracle(idx)
    mc = _min_cov(CASES[idx])
    out, summary = {}, SUMMARY_HEADER.decode()
    for r in refs:
        if sum(sum(c) for c in counts[r]) > 0:
            c = tt._c6(counts[r])
            out[r + "__" + prefix + ".depth.tsv"] = (DEPTH_HEADER + table.format_depth(c)).decode("latin-1")
            out[r + "__" + prefix + ".lowcov.tsv"] = (LOWCOV_HEADER + table.format_lowcov(c, 1, mc)).decode("latin-1")
            summary += _summary_line(r, c, mc)
    out[prefix + ".depth_summary.tsv"] = summary
    return out


# ---------------------------------------------------------------------------- CPU tier
def test_constants():
    assert (table.DEPTH_HEADER, table.DEPTH_SUFFIX) == (DEPTH_HEADER, b".depth.tsv")
    assert (table.LOWCOV_HEADER, table.LOWCOV_SUFFIX) == (LOWCOV_HEADER, b".lowcov.tsv")
    assert (table.SUMMARY_HEADER, table.SUMMARY_SUFFIX) == (SUMMARY_HEADER, b".depth_summary.tsv")
    assert table.EMPTY_STATS == EMPTY


def test_tiny_literal():
    """The `tiny` case (coverage 1 2 2 2 2 1 0 0 0 0): both files and the summary line."""
    idx = next(k for k, c in enumerate(CASES) if c["name"] == "tiny")
    refs, counts, _ = tt._oracle(idx)
    c = tt._c6(counts["g1"])
    assert table.coverage(c) == [1, 2, 2, 2, 2, 1, 0, 0, 0, 0]
    assert table.depth_runs(table.coverage(c)) == [(0, 1, 1), (1, 5, 2), (5, 6, 1), (6, 10, 0)]
    assert table.format_depth(c) == b"1\t1\t1\n2\t5\t2\n6\t6\t1\n7\t10\t0\n"
    assert table.format_depth(c, 95) == b"95\t95\t1\n96\t99\t2\n100\t100\t1\n101\t104\t0\n"
    assert table.format_lowcov(c) == b"7\t10\n" == table.format_lowcov(c, 1, 1)
    assert table.format_lowcov(c, 1, 2) == b"1\t1\n6\t10\n"
    assert table.format_lowcov(c, 1, 3) == b"1\t10\n"
    assert table.depth_stats(c, 1) == (4, 6, 6, 10, 0, 2) and table.depth_stats(c, 2) == (4, 6, 4, 10, 0, 2)
    # the summary: the tiles' statistics summed per reference (here the reference cut 4 + 6,
    # a second reference without reads between, a third of one tile)
    hb = SimpleNamespace(info=SimpleNamespace(n_refs=3), names=["g1", "none", "g3"], ref_reads=[2, 0, 1],
                         ref_first_block=[0, 2, 3], ref_nblocks=[2, 1, 1], ref_len=[10, 7, 3])
    stats = np.array([table.depth_stats(c[:, :4], 1), (2, 2, 2, 3, 0, 2), EMPTY, (1, 3, 0, 6, 2, 2)], dtype=np.int64)
    assert stats[0].tolist() == [2, 4, 4, 7, 1, 2]
    assert table.summary_file(hb, "px", stats) == {
        b"px.depth_summary.tsv": SUMMARY_HEADER + b"g1\t10\t6\t6\t10\t0\t2\t4\n" + b"g3\t3\t3\t0\t6\t2\t2\t1\n"}
    assert _summary_line("g1", c, 1) == "g1\t10\t6\t6\t10\t0\t2\t4\n"


def test_numeric_edges():
    big = np.full((6, 1), 4294967295, dtype=np.uint32)
    line = table.format_depth(big, 9999999999)
    assert line == b"9999999999\t9999999999\t25769803770\n" and len(line) == 34
    assert table.format_lowcov(np.zeros((6, 2), dtype=np.uint32), 9999999998) == b"9999999998\t9999999999\n"
    assert table.depth_stats(big, 1) == (1, 1, 1, 25769803770, 25769803770, 25769803770)
    empty = np.zeros((6, 0), dtype=np.uint32)
    assert table.format_depth(empty) == b"" == table.format_lowcov(empty)
    assert table.depth_runs([]) == [] and table.depth_stats(empty, 1) == EMPTY
    for f in (table.format_depth, table.format_lowcov, lambda c: table.depth_stats(c, 1)):
        with pytest.raises(ValueError):
            f(np.zeros((5, 3)))


def test_models_against_groupby_on_every_ok_case():
    """Every line of both tables and every statistic against itertools.groupby over the oracle's
    coverage lists; the runs partition [1, LN]."""
    n_runs = n_low = multi = 0
    for idx, case in enumerate(CASES):
        if case["status"] != "ok":
            continue
        refs, counts, _ = tt._oracle(idx)
        mc = _min_cov(case)
        for r, ln in refs.items():
            cov = [sum(int(v) for v in n) for n in counts[r]]
            assert len(cov) == ln
            c = tt._c6(counts[r]) if ln else np.zeros((6, 0), dtype=np.int64)
            want, low, p = [], [], 1
            for v, grp in itertools.groupby(cov):
                k = len(list(grp))
                want.append("%d\t%d\t%d" % (p, p + k - 1, v))
                p += k
            assert p == ln + 1
            p = 1
            for v, grp in itertools.groupby(x < mc for x in cov):
                k = len(list(grp))
                if v:
                    low.append("%d\t%d" % (p, p + k - 1))
                p += k
            got = table.format_depth(c).decode().split("\n")
            assert got.pop() == "" and got == want, (case["name"], r)
            got = table.format_lowcov(c, 1, mc).decode().split("\n")
            assert got.pop() == "" and got == low, (case["name"], r)
            if ln:
                assert table.depth_stats(c, mc) == (len(want), sum(x >= 1 for x in cov), sum(x >= mc for x in cov),
                                                    sum(cov), min(cov), max(cov)), (case["name"], r)
            n_runs += len(want)
            n_low += len(low)
            multi += len(want) > 1
    assert n_runs > 1000 and n_low > 100 and multi > 100


def test_parser_has_the_flags():
    from sam2consensus_amd.cli import build_parser, variants_of
    p = build_parser()
    a = p.parse_args(["-i", "x.sam"])
    assert a.depth is False and a.lowcov is False
    a = p.parse_args(["-i", "x.sam", "--depth"])
    assert a.depth is True and a.lowcov is False
    a = p.parse_args(["-i", "x.sam", "--lowcov"])
    assert a.depth is False and a.lowcov is True
    a = p.parse_args(["-i", "x.sam", "--lowcov", "--counts", "--depth", "--variants"])
    assert a.depth and a.lowcov and a.counts and variants_of(p, a) == (2, 0.05)


@pytest.mark.parametrize("env", [{"WORLD_SIZE": "2"}, {"S2C_STREAM": "1M"}], ids=["world2", "stream"])
@pytest.mark.parametrize("flag", ["--depth", "--lowcov"])
def test_refused_combinations(flag, env, tmp_path, monkeypatch, capsys):
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
        main(["-i", str(sam), "-o", str(tmp_path / "out"), flag])
    assert e.value.code == 2
    assert flag in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == ["in.sam"]


def test_runs_symbols_declared_and_bound():
    from sam2consensus_amd import _lib
    lib = _lib.lib
    assert {"s2c_runs_mark", "s2c_runs_len", "s2c_runs_write"} <= set(_lib.EXPORTS)
    assert lib.s2c_abi_version() == 14
    assert [len(getattr(lib, f).argtypes) for f in ("s2c_runs_mark", "s2c_runs_len", "s2c_runs_write")] == [5, 11, 11]
    # (argument errors need no device)
    OK, ARG = _lib.S2C_OK, _lib.S2C_ERR_ARG
    assert lib.s2c_runs_mark(None, -1, 0, None, None) == ARG
    assert lib.s2c_runs_mark(None, 0, -1, None, None) == ARG
    assert lib.s2c_runs_mark(None, 0, 0, None, None) == OK and lib.s2c_runs_mark(None, 0, 3, None, None) == OK
    assert lib.s2c_runs_mark(None, 64, 0, None, None) == ARG
    assert lib.s2c_runs_len(None, 16, None, None, None, -1, 0, 1, None, None, None) == ARG
    assert lib.s2c_runs_len(None, -16, None, None, None, 0, 0, 1, None, None, None) == ARG
    assert lib.s2c_runs_len(None, 16, None, None, None, 0, -1, 1, None, None, None) == ARG
    assert lib.s2c_runs_len(None, 16, None, None, None, 0, 0, -1, None, None, None) == ARG
    assert lib.s2c_runs_len(None, 16, None, None, None, 0, 0, 1, None, None, None) == OK
    assert lib.s2c_runs_len(None, 16, None, None, None, 1, 0, 1, None, None, None) == ARG
    assert lib.s2c_runs_write(None, 16, None, None, None, None, 1, 0, None, -1, None) == ARG
    assert lib.s2c_runs_write(None, 16, None, None, None, None, -1, 0, None, 0, None) == ARG
    assert lib.s2c_runs_write(None, 16, None, None, None, None, 0, -1, None, 0, None) == ARG
    assert lib.s2c_runs_write(None, 16, None, None, None, None, 0, 0, None, 0, None) == OK
    assert lib.s2c_runs_write(None, 16, None, None, None, None, 1, 0, None, 0, None) == ARG


# ---------------------------------------------------------------------------- GPU tier: the kernels
def _counts_of(cov):
    """counts[6][P] u32 with column sums cov (each < 2^32): the symbols holding them change
    from position to position, so equal coverage next to each other has different counts."""
    cov = np.asarray(cov, dtype=np.uint64)
    j = np.arange(len(cov))
    c = np.zeros((6, len(cov)), dtype=np.uint64)
    np.add.at(c, (j % 6, j), cov - cov // 2)
    np.add.at(c, ((j // 6) % 6, j), cov // 2)
    assert (c.sum(axis=0) == cov).all() and c.max() < 2 ** 32
    return c.astype(np.uint32)


# The shapes scene.  References (global ranges; each starts at a multiple of 64):
#   R1 [0, 3000)       a run over position 64, one over the walk step at 256, uncovered between
#                      and to its end: the last run ends at e with 8 positions of padding behind
#   R2 [3008, 3009)    one position, uncovered as R1's end and the padding: its start is forced
#   R3 [3072, 5120)    coverage 4, 5, 4, 5, …: 2,048 starts; its first differs from the padding
#   R4 [5120, 5720)    begins with R3's last coverage (5) and no padding between: forced start
#   R5 [5760, 45860)   10 covered, 40,000 uncovered, 90 covered: the end of a run looked up over
#                      about 600 mask words, more than one step of the workgroup
P2 = 45888
REFS2 = [(0, 3000), (3008, 3009), (3072, 5120), (5120, 5720), (5760, 45860)]


def _scene_cov():
    cov = np.zeros(P2, dtype=np.uint64)
    cov[10:100] = 5
    cov[200:300] = 7
    cov[300:310] = 12345
    cov[3072:5120] = 4 + (np.arange(2048) & 1)
    cov[5120:5400] = 5
    cov[5400:5720] = 1
    cov[5760:5770] = 2
    cov[45770:45860] = 9
    return cov


def _cut_refs(refs, width, p0=1):
    """Each reference cut into blocks of `width` (None: one block): (a, b, p0, s, e) rows."""
    rows = []
    for s, e in refs:
        w = width or (e - s)
        rows += [(a, min(a + w, e), p0 + (a - s), s, e) for a in range(s, e, w)]
    return rows


# R3 cut so that its blocks hold exactly 255, 256, 257, 513 and 767 starts; the others whole
CUT_STARTS = (_cut_refs(REFS2[:2], None) +
              [(a, b, 1 + a - 3072, 3072, 5120) for a, b in ((3072, 3327), (3327, 3583), (3583, 3840), (3840, 4353), (4353, 5120))] +
              _cut_refs(REFS2[3:], None))


def _model_blocks(c, rows, cut, min_cov):
    """(text, stats) per block row from the models: the lines of the runs of the row's
    reference that start inside [a, b), printed relative to the block."""
    cache, out = {}, []
    for a, b, p0, s, e in rows:
        if (s, e) not in cache:
            cov = table.coverage(c[:, s:e])
            cache[(s, e)] = (cov, table.depth_runs([v < cut for v in cov] if cut else cov))
        cov, runs = cache[(s, e)]
        lines, st = [], list(EMPTY)
        for rs, re_, v in runs:
            g, end = s + rs, s + re_
            if not a <= g < b:
                continue
            S, E = p0 + (g - a), p0 + (end - a) - 1
            if cut:
                if v:
                    lines.append("%d\t%d\n" % (S, E))
                continue
            lines.append("%d\t%d\t%d\n" % (S, E, v))
            n = end - g
            st = [st[0] + 1, st[1] + (n if v >= 1 else 0), st[2] + (n if v >= min_cov else 0), st[3] + n * v,
                  min(st[4], v), max(st[5], v)]
        out.append(("".join(lines).encode(), tuple(st)))
    return out


def _dev_counts(c):
    import torch
    return torch.from_numpy(np.ascontiguousarray(c).view(np.int32)).cuda()


def _runs_mark(counts_d, padded, cut):
    import torch
    from sam2consensus_amd import _lib
    words = (padded + 63) // 64
    mask = torch.full((words + 2,), -1, dtype=torch.int64, device="cuda")   # (two guard words)
    _lib.check(_lib.lib.s2c_runs_mark(_ptr(counts_d), padded, cut, _ptr(mask), _stream()))
    return mask


def _runs_len(counts_d, padded, mask, rows, cut, min_cov, with_stats=True):
    import torch
    from sam2consensus_amd import _lib
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    n = len(rows)
    lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    stats = torch.full((n * 6,), -7, dtype=torch.int64, device="cuda") if with_stats else None
    b, r = tt._dev_i64(rows[:, :3]), tt._dev_i64(rows[:, 3:])
    _lib.check(_lib.lib.s2c_runs_len(_ptr(counts_d), padded, _ptr(mask), _ptr(b), _ptr(r), n, cut, min_cov, _ptr(lens),
                                     _ptr(stats), _stream()))
    return lens.cpu().numpy(), (stats.cpu().numpy().reshape(n, 6) if with_stats else None)


def _runs_write(counts_d, padded, mask, rows, offs, cut, dst_len, alloc):
    import torch
    from sam2consensus_amd import _lib
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    dst = torch.full((alloc,), 0xEE, dtype=torch.uint8, device="cuda")
    b, r, f = tt._dev_i64(rows[:, :3]), tt._dev_i64(rows[:, 3:]), tt._dev_i64(offs)
    _lib.check(_lib.lib.s2c_runs_write(_ptr(counts_d), padded, _ptr(mask), _ptr(b), _ptr(r), _ptr(f), len(rows), cut,
                                       _ptr(dst), dst_len, _stream()))
    torch.cuda.synchronize()
    return dst.cpu().numpy().tobytes()


def _check_mask(mask, c, cut, padded):
    cov = c.astype(np.uint64).sum(axis=0)
    cls = (cov < cut) if cut else cov
    want = np.ones(padded, dtype=bool)
    want[1:] = cls[1:padded] != cls[:padded - 1]
    got = mask.cpu().numpy().view(np.uint64)
    assert got[-2:].tolist() == [2 ** 64 - 1] * 2
    bits = np.unpackbits(got[:-2].view(np.uint8), bitorder="little").astype(bool)
    assert (bits[:padded] == want).all(), np.flatnonzero(bits[:padded] != want)[:10]
    assert not bits[padded:].any()


def _kernels(c, counts_d, mask, rows, cut, min_cov, shift=0):
    """lens, stats and the written text of `rows` against the model; returns the model's pairs."""
    padded = c.shape[1]
    want = _model_blocks(c, rows, cut, min_cov)
    lens, stats = _runs_len(counts_d, padded, mask, rows, cut, min_cov, with_stats=not cut)
    assert lens.tolist() == [len(t) for t, _ in want], \
        [(rows[k], int(lens[k]), len(want[k][0])) for k in range(len(rows)) if lens[k] != len(want[k][0])][:5]
    if not cut:
        bad = [(rows[k], stats[k].tolist(), want[k][1]) for k in range(len(rows)) if tuple(stats[k].tolist()) != want[k][1]]
        assert not bad, bad[:5]
    offs = np.concatenate([[0], np.cumsum(lens)]) + shift
    total = int(offs[-1])
    got = _runs_write(counts_d, padded, mask, rows, offs, cut, total, total + 64)
    assert got[:shift] == b"\xEE" * shift and got[total:] == b"\xEE" * 64
    for k, (t, _) in enumerate(want):
        assert got[offs[k]:offs[k + 1]] == t, (rows[k], tt._first_diff(got[offs[k]:offs[k + 1]], t))
    return want


def test_scene_holds_what_the_kernel_tests_need():
    cov = _scene_cov()
    c = _counts_of(cov)
    assert 6 * 4 * P2 < 1.2e6 and all(s % 64 == 0 and e <= P2 for s, e in REFS2)
    assert (c[:, 10] != c[:, 11]).any() and cov[10] == cov[11]          # equal coverage, different counts
    runs = {r: table.depth_runs(table.coverage(c[:, r[0]:r[1]])) for r in REFS2}
    assert (10, 100, 5) in runs[REFS2[0]] and (200, 300, 7) in runs[REFS2[0]]   # over 64; over 256
    assert runs[REFS2[0]][-1] == (310, 3000, 0) and not cov[3000:3008].any()    # ends at e, padding behind
    assert runs[REFS2[1]] == [(0, 1, 0)] and cov[3007] == cov[3008]
    assert len(runs[REFS2[2]]) == 2048 and cov[3071] != cov[3072]
    assert cov[5119] == cov[5120] == 5
    assert runs[REFS2[4]] == [(0, 10, 2), (10, 40010, 0), (40010, 40100, 9)]
    assert (45770 - 7808) // 64 > 2 * 256        # cut at 2,048 the lookup passes 512 words: more than one step
    per_block = [len(t.split(b"\n")) - 1 for t, _ in _model_blocks(c, CUT_STARTS, 0, 1)]
    assert per_block[2:7] == [255, 256, 257, 513, 767]
    whole = _model_blocks(c, _cut_refs(REFS2, 2048), 0, 1)
    assert sum(1 for t, st in whole if t == b"" and st == EMPTY) >= 18  # whole blocks inside the 40,000-position run
    low = _model_blocks(c, _cut_refs(REFS2, None), 5, 1)
    assert low[2][0].count(b"\n") == 1024 and low[3][0] == b"281\t600\n"


@pytest.mark.gpu
@pytest.mark.parametrize("cut,min_cov", [(0, 1), (0, 6), (5, 1), (1, 1)], ids=["depth", "depth-m6", "low5", "low1"])
def test_kernels_on_the_shapes_scene(cut, min_cov):
    """The mask, and block for block the lengths, statistics and bytes against the model, with
    the references whole, cut into blocks of 64 and of 2,048, and cut at 255, 256, 257 and 513
    starts; the four cuttings give one text and one set of sums per reference."""
    c = _counts_of(_scene_cov())
    counts_d = _dev_counts(c)
    mask = _runs_mark(counts_d, P2, cut)
    _check_mask(mask, c, cut, P2)
    per_ref = []
    for k, rows in enumerate((_cut_refs(REFS2, None), _cut_refs(REFS2, 64), _cut_refs(REFS2, 2048), CUT_STARTS)):
        # (block-relative positions: p0 follows the cutting, so the printed numbers do not change)
        want = _kernels(c, counts_d, mask, rows, cut, min_cov, shift=k % 2)
        acc = {}
        for (a, b, p0, s, e), (t, st) in zip(rows, want):
            text, tot = acc.get((s, e), (b"", EMPTY))
            acc[(s, e)] = (text + t, (tot[0] + st[0], tot[1] + st[1], tot[2] + st[2], tot[3] + st[3],
                                      min(tot[4], st[4]), max(tot[5], st[5])))
        per_ref.append(acc)
    assert per_ref[0] == per_ref[1] == per_ref[2] == per_ref[3]
    for s, e in REFS2:
        text, st = per_ref[0][(s, e)]
        if cut:
            assert text == table.format_lowcov(c[:, s:e], 1, cut)
        else:
            assert text == table.format_depth(c[:, s:e]) and st == table.depth_stats(c[:, s:e], min_cov)


LADDER_ROWS = [(a, b, p0, 0, tt.PADDED) for a, b, p0 in tt.BLOCKS] + \
              [(1000, 1100, 9999999900, 1000, 1100), (1000, 1001, 9999999999, 1000, 1001), (950, 1050, 95, 900, 1200),
               (900, 950, 1, 900, 1200), (0, 4096, 9999995904, 0, 4096), (4095, 4096, 1, 4032, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [0, 1000000, 25769803771], ids=["depth", "low1e6", "lowall"])
def test_kernels_on_the_digit_ladder(cut):
    """test_table.py's counts (every digit count in the counts, an 11-digit coverage) and its
    blocks (lengths around the wave and sub-block sizes, odd starts, 10-digit positions)."""
    c = tt._synthetic_counts()
    counts_d = _dev_counts(c)
    mask = _runs_mark(counts_d, tt.PADDED, cut)
    _check_mask(mask, c, cut, tt.PADDED)
    want = _kernels(c, counts_d, mask, LADDER_ROWS, cut, 1000000, shift=1)
    k = LADDER_ROWS.index((1000, 1001, 9999999999, 1000, 1001))
    low = {0: b"\t25769803770\n", 1000000: None, 25769803771: b"\n"}[cut]   # (the stretch is low below the last cut alone)
    assert want[k][0] == (b"9999999999\t9999999999" + low if low else b"")
    k = LADDER_ROWS.index((1000, 1100, 9999999900, 1000, 1100))
    assert want[k][0] == (b"9999999900\t9999999999" + low if low else b"")
    assert all(p0 + (e - a) <= 10 ** 10 for a, b, p0, s, e in LADDER_ROWS)
    # a length that is no multiple of 64: the last word's unused bits are zero
    short = np.ascontiguousarray(c[:, :4000])
    m2 = _runs_mark(_dev_counts(short), 4000, cut)
    _check_mask(m2, short, cut, 4000)
    assert len(m2) == 63 + 2


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [0, 5], ids=["depth", "low5"])
def test_guards(cut):
    """A block violating each bound gets length 0 and the empty statistics and no byte; ranges
    of offs that do not match the lengths cut or pad the text and leave the 100 sentinel bytes
    around them untouched; bad arguments are refused."""
    from sam2consensus_amd import _lib
    c = _counts_of(_scene_cov())
    counts_d = _dev_counts(c)
    mask = _runs_mark(counts_d, P2, cut)
    good = [(0, 3000, 1, 0, 3000), (3072, 4000, 1, 3072, 5120), (4000, 5120, 929, 3072, 5120)]
    bad = [(0, 100, 1, -64, 3000), (0, 100, 1, 64, 3000), (100, 99, 1, 0, 3000), (0, 3000, 1, 0, 2999),
           (5760, P2 + 1, 1, 5760, P2 + 1), (5760, 5800, 1, 5760, P2 + 64), (0, 100, -1, 0, 3000),
           (0, 100, 10 ** 10 - 2999, 0, 3000), (-64, 0, 1, -64, 3000)]
    assert _model_blocks(c, [(0, 100, 10 ** 10 - 3000, 0, 3000)], cut, 1)[0][0] != b""   # (the last p0 that is allowed)
    rows = good + [(0, 100, 10 ** 10 - 3000, 0, 3000)] + bad
    want = _model_blocks(c, rows[:4], cut, 1)
    lens, stats = _runs_len(counts_d, P2, mask, rows, cut, 1, with_stats=not cut)
    assert lens.tolist() == [len(t) for t, _ in want] + [0] * len(bad)
    if not cut:
        assert [tuple(r) for r in stats.tolist()] == [st for _, st in want] + [EMPTY] * len(bad)
    else:   # (stats is not written when cut >= 1)
        _, untouched = _runs_len(counts_d, P2, mask, rows, cut, 1, with_stats=True)
        assert (untouched == -7).all()
    # every block followed by an empty one that owns 100 sentinel bytes; the good blocks get
    # their length − 7, + 5, − 3000 and exactly; the bad ones 100 bytes that must stay
    texts = [t for t, _ in want]
    assert all(len(t) > 7 for t in texts)
    assert len(texts[2]) > 3000                    # (several emits: the cut falls in a later one)
    room = [len(texts[0]) - 7, len(texts[1]) + 5, len(texts[2]) - 3000, len(texts[3])] + [100] * len(bad)
    rows2, sizes = [], []
    for r, n in zip(rows, room):
        rows2 += [r, (64, 64, 1, 0, 3000)]
        sizes += [n, 100]
    offs = np.concatenate([[0], np.cumsum(sizes)]) + 100
    total = int(offs[-1])
    got = _runs_write(counts_d, P2, mask, rows2, offs, cut, total, total + 64)
    assert got[:100] == b"\xEE" * 100 and got[total:] == b"\xEE" * 64
    expect = [texts[0][:-7], texts[1] + b"\xEE" * 5, texts[2][:-3000], texts[3]] + [b"\xEE" * 100] * len(bad)
    for k, w in enumerate(expect):
        assert got[offs[2 * k]:offs[2 * k + 1]] == w, (rows[k], tt._first_diff(got[offs[2 * k]:offs[2 * k + 1]], w))
        assert got[offs[2 * k + 1]:offs[2 * k + 2]] == b"\xEE" * 100, rows[k]
    # ranges that are no ranges: descending, negative, past dst_len — nothing is written
    offs_bad = np.array([50, 40, -5, 10, total + 200, total + 300], dtype=np.int64)
    got = _runs_write(counts_d, P2, mask, good + good[:2], offs_bad, cut, total, total + 64)
    assert got == b"\xEE" * (total + 64)
    # the argument errors, with real buffers
    lib, ARG = _lib.lib, _lib.S2C_ERR_ARG
    b, r = tt._dev_i64([g[:3] for g in good]), tt._dev_i64([g[3:] for g in good])
    lens_d, f = tt._dev_i64([0] * 3), tt._dev_i64([0] * 4)
    assert lib.s2c_runs_mark(_ptr(counts_d), P2, -1, _ptr(mask), _stream()) == ARG
    assert lib.s2c_runs_mark(_ptr(counts_d), P2, 0, None, _stream()) == ARG
    assert lib.s2c_runs_len(_ptr(counts_d), P2, _ptr(mask), _ptr(b), _ptr(r), -1, 0, 1, _ptr(lens_d), _ptr(lens_d), _stream()) == ARG
    assert lib.s2c_runs_len(_ptr(counts_d), P2, _ptr(mask), _ptr(b), _ptr(r), 3, -1, 1, _ptr(lens_d), _ptr(lens_d), _stream()) == ARG
    assert lib.s2c_runs_len(_ptr(counts_d), P2, _ptr(mask), _ptr(b), None, 3, 0, 1, _ptr(lens_d), _ptr(lens_d), _stream()) == ARG
    assert lib.s2c_runs_len(_ptr(counts_d), P2, _ptr(mask), _ptr(b), _ptr(r), 3, 0, 1, _ptr(lens_d), None, _stream()) == ARG
    assert lib.s2c_runs_write(_ptr(counts_d), P2, _ptr(mask), _ptr(b), _ptr(r), _ptr(f), -1, 0, _ptr(mask), 0, _stream()) == ARG
    assert lib.s2c_runs_write(_ptr(counts_d), P2, _ptr(mask), _ptr(b), _ptr(r), _ptr(f), 3, -1, _ptr(mask), 0, _stream()) == ARG
    assert lib.s2c_runs_write(_ptr(counts_d), P2, _ptr(mask), _ptr(b), _ptr(r), _ptr(f), 3, 0, None, 0, _stream()) == ARG
    assert lib.s2c_runs_write(_ptr(counts_d), P2, _ptr(mask), _ptr(b), _ptr(r), None, 3, 0, _ptr(mask), 0, _stream()) == ARG


# ---------------------------------------------------------------------------- GPU tier: end to end
def _check_case(idx, extra, **kw):
    from sam2consensus_amd.cli import run_text
    case = CASES[idx]
    status, files = run_text(case["sam"], list(case["args"]) + extra, **kw)
    assert status == case["status"], case["name"]
    if status != "ok":
        assert files == {}, case["name"]
        return
    assert {k: v for k, v in files.items() if k.endswith(".fasta")} == case["files"], case["name"]
    assert {k: v for k, v in files.items() if not k.endswith(".fasta")} == _oracle_runs(idx), case["name"]


CHUNK = 100   # golden cases per test: a run takes milliseconds, most of a test of one would be its set-up


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, len(CASES), CHUNK))
def test_golden_cases_with_depth_and_lowcov(first):
    """run_text(..., depth=True, lowcov=True) on every golden case, CHUNK to a test: the case's
    status; on ok the reference's FASTA files, a depth and a low-coverage table per reference
    with Σcoverage > 0 and the summary, equal to the oracle's counts through the models, the
    least coverage the case's -m."""
    for idx in range(first, min(first + CHUNK, len(CASES))):
        _check_case(idx, [], depth=True, lowcov=True)


@pytest.mark.gpu
def test_kat_cases_with_the_flags_among_the_args():
    for idx in range(KAT):
        _check_case(idx, ["--lowcov", "--depth"])


def _model_counts(hb):
    import batch_model as bm
    runs, _ = bm.model_reads(hb)
    return bm.model_counts(hb, runs)


def _model_runs(hb, want, prefix, min_cov, depth=True, lowcov=True):
    out, low, summary = {}, {}, SUMMARY_HEADER
    for r in range(hb.info.n_refs):
        if hb.ref_reads[r] > 0:
            a, ln = int(hb.ref_off[r]), int(hb.ref_len[r])
            c = want[:, a:a + ln]
            name = hb.names[r].encode()
            out[name + b"__" + prefix + b".depth.tsv"] = DEPTH_HEADER + table.format_depth(c)
            low[name + b"__" + prefix + b".lowcov.tsv"] = LOWCOV_HEADER + table.format_lowcov(c, 1, min_cov)
            summary += _summary_line(hb.names[r], c, min_cov).encode()
    res = dict(out) if depth else {}
    if lowcov:
        res.update(low)
    if depth:
        res[prefix + b".depth_summary.tsv"] = summary
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name,over", tt.TILE_KINDS, ids=[n for n, _ in tt.TILE_KINDS])
def test_every_tile_kind(name, over):
    """General tiles with insertions (c2), dense tiles (c5), maxdel drops (c5nd), deep tiles
    (c4): the run tables and the summary == the batch model's counts through the models, in
    the order depth tables, low-coverage tables, summary after the FASTA files, which equal the
    fused route's."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch(name, **over)
    m = 30 if name == "c2" else 3
    plain = consensus_batch(hb, [0.25, 0.75], b"x", min_depth=m)
    both = consensus_batch(hb, [0.25, 0.75], b"x", min_depth=m, depth=True, lowcov=True)
    nf = len(plain)
    assert plain and list(both)[:nf] == list(plain)
    for k, v in plain.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
    want = _model_runs(hb, _model_counts(hb), b"x", m)
    assert list(both)[nf:] == list(want)
    lines = 0
    for k, v in want.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
        lines += v.count(b"\n") - 1
    assert lines > len(want), "the configuration must hold runs"


@pytest.mark.gpu
def test_all_four_tables_equal_the_separate_runs():
    """--counts --variants --depth --lowcov in one run: every file what the run with its flag
    alone gives, the files in the order FASTA, counts, variants, depth, lowcov, summary; -m 0
    is a least coverage of 1."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch("c2", n_refs=3)
    kw = dict(min_depth=30)
    plain = consensus_batch(hb, [0.25], b"x", **kw)
    alone = [consensus_batch(hb, [0.25], b"x", counts=True, **kw), consensus_batch(hb, [0.25], b"x", variants=(1, 0.0), **kw),
             consensus_batch(hb, [0.25], b"x", depth=True, **kw), consensus_batch(hb, [0.25], b"x", lowcov=True, **kw)]
    every = consensus_batch(hb, [0.25], b"x", counts=True, variants=(1, 0.0), depth=True, lowcov=True, **kw)
    order = list(plain)
    for files in alone:
        assert list(files)[:len(plain)] == list(plain) and len(files) > len(plain)
        order += list(files)[len(plain):]
    summary = order.pop(order.index(b"x.depth_summary.tsv"))
    assert list(every) == order + [summary]
    for files in alone:
        for k, v in files.items():
            assert every[k] == v, (k, tt._first_diff(every[k], v))
    counts = _model_counts(hb)
    got = {}
    for m in (0, 1, 30):
        files = consensus_batch(hb, [0.25], b"x", min_depth=m, depth=True, lowcov=True)
        got[m] = {k: v for k, v in files.items() if not k.endswith(b".fasta")}
        assert got[m] == _model_runs(hb, counts, b"x", max(m, 1))
    assert got[0] == got[1] != got[30]
    assert any(v != LOWCOV_HEADER for k, v in got[30].items() if k.endswith(b".lowcov.tsv"))


@pytest.mark.gpu
def test_workspace_reuse():
    """run_with_tables with the run tables twice on one workspace: the same tables, statistics
    and FASTA results; it returns exactly the tables asked for; depth_table needs filled
    counts."""
    import torch
    from sam2consensus_amd import configs
    from sam2consensus_amd.engine import DeviceBatch, Workspace

    def fetched(ws):
        stats, offs, out = ws.fetch()
        return stats.tobytes(), offs.tobytes(), bytes(out)

    hb = configs.synth_batch("c2", n_refs=18)
    ws0 = Workspace(DeviceBatch(hb), [0.25])
    ws0.run()
    base = fetched(ws0)
    ws = Workspace(DeviceBatch(hb, dense_layers=True), [0.25], keep_counts=True)
    with pytest.raises(ValueError):
        ws.depth_table()          # (nothing has filled the counts)
    runs = []
    for _ in range(2):
        res = ws.run_with_tables({"depth": (2,), "lowcov": (2,)})
        assert list(res) == ["depth", "lowcov"] and res["lowcov"][2] is None
        (doffs, dtext, dstats), (loffs, ltext, _) = res["depth"], res["lowcov"]
        runs.append((doffs.tobytes(), dtext.cpu().numpy().tobytes(), dstats.tobytes(), loffs.tobytes(),
                     ltext.cpu().numpy().tobytes(), fetched(ws)))
    assert runs[0] == runs[1] and runs[0][5] == base
    assert dstats.shape == (int(hb.info.n_tiles), 6) and dstats.dtype == np.int64
    want = _model_runs(hb, _model_counts(hb), b"x", 2)
    got = table.table_files(hb, b"x", doffs, runs[0][1], table.DEPTH_HEADER, table.DEPTH_SUFFIX)
    got.update(table.table_files(hb, b"x", loffs, runs[0][4], table.LOWCOV_HEADER, table.LOWCOV_SUFFIX))
    got.update(table.summary_file(hb, b"x", dstats))
    assert got == want
    two = ws.run_with_tables({"counts": (), "variants": (1, 2, 0.05)})
    assert list(two) == ["counts", "variants"] and fetched(ws) == base
    one = ws.run_with_tables({"lowcov": (2,)})
    assert set(one) == {"lowcov"} and one["lowcov"][1].cpu().numpy().tobytes() == runs[0][4] and fetched(ws) == base
    with pytest.raises(ValueError):
        ws.run_with_tables({"lowcov": (0,)})
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_cli_process_c1(tmp_path):
    """sam2consensus.py with all four flags on the full C1 (10 x 1,000 bp): the reference's 10
    FASTA files; the run tables and the summary equal (by hash) to the models over the count
    tables' rows; stdout exact, the new lines after the variant lines and before Done.  Without
    the flags stdout and the file set are the parent's."""
    import subprocess
    import sys
    from sam2consensus_amd import configs
    from sam2consensus_amd.batch import parse_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = tt.CONFIGS["c1"]
    sam = str(tmp_path / "c1.sam")
    configs.synth_write("c1", sam)
    hb = parse_file(sam)
    names = list(hb.names)
    n_reads, n_mapped = int(hb.info.lines_total - hb.info.header_lines), int(hb.info.reads_mapped)
    assert hb.info.n_refs == 10 and 0 < n_reads < 500000
    hb.free()
    outs = {}
    for tag, extra in (("plain", []), ("every", ["--depth", "--variants", "--lowcov", "--counts"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(root, "sam2consensus.py"), "-i", sam, "-o", str(out)] +
                           g["args"] + extra, capture_output=True, text=True, timeout=240, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (r.stdout, {fn: open(os.path.join(out, fn), "rb").read() for fn in os.listdir(out)})

    def saved(d, what, suffix):
        return "".join("%s saved for %s in: %s/%s__c1.%s\n" % (what, n, d, n, suffix) for n in names)

    sha = lambda v: hashlib.sha256(v).hexdigest()  # noqa: E731
    golden = {k: v["sha256"] for k, v in g["files"].items()}
    so, files = outs["plain"]
    d = str(tmp_path / "plain")
    assert so == tt.C1_STDOUT.format(sam=sam, n=n_reads, m=n_mapped, saved=saved(d, "Consensus sequence at 25%", "fasta"))
    assert {k: sha(v) for k, v in files.items()} == golden
    so, files = outs["every"]
    d = str(tmp_path / "every")
    assert so == tt.C1_STDOUT.format(sam=sam, n=n_reads, m=n_mapped, saved=(
        saved(d, "Consensus sequence at 25%", "fasta") + saved(d, "Count table", "counts.tsv") +
        saved(d, "Variant table", "variants.tsv") + saved(d, "Depth table", "depth.tsv") +
        saved(d, "Low-coverage table", "lowcov.tsv") + "Depth summary saved in: %s/c1.depth_summary.tsv\n" % d))
    assert {k: sha(v) for k, v in files.items() if k.endswith(".fasta")} == golden
    assert len(files) == 51
    min_cov = max(o.parse_argv(["-i", "in.sam"] + list(g["args"])).min_depth, 1)
    want, summary, lines = {}, SUMMARY_HEADER, 0
    for n in names:
        rows = files[n + "__c1.counts.tsv"].split(b"\n")[1:-1]
        c = np.array([[int(x) for x in row.split(b"\t")[2:]] for row in rows], dtype=np.int64).T
        want[n + "__c1.depth.tsv"] = DEPTH_HEADER + table.format_depth(c)
        want[n + "__c1.lowcov.tsv"] = LOWCOV_HEADER + table.format_lowcov(c, 1, min_cov)
        summary += _summary_line(n, c, min_cov).encode()
        lines += want[n + "__c1.depth.tsv"].count(b"\n") - 1
    want["c1.depth_summary.tsv"] = summary
    assert lines > 100
    assert {k: sha(v) for k, v in files.items() if k in want} == {k: sha(v) for k, v in want.items()}
