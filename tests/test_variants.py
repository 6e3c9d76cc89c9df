"""--variants: the sparse tables of mixed sites (sam2consensus_amd/table.py, csrc/s2c_sites.hip).

Without a GPU: the rule and the line format literally, at their edges, and against a restatement
in exact fractions on every golden case; the flags and their refused combinations; the
bindings.  On the GPU: the three kernels alone on synthetic counts (test_table.py's digit
ladder plus stretches without a site, of sites only, of single sites at the wave and sub-block
edges, alternating, tied and at the rule's edges; the guards), the golden cases end to end,
every tile kind against the batch model, a reused workspace, and the CLI process on C1."""
import hashlib
import os
from fractions import Fraction

import numpy as np
import pytest

import golden_io
import s2c_oracle as o
import test_table as tt
from devmem import _ptr, _stream

from sam2consensus_amd import table

CASES = tt.CASES
KAT = len(golden_io.load("kat"))
SYM = "-ACGNT"
HEADER = b"pos\tcov\t-\tA\tC\tG\tN\tT\tmajor\talt\taf\n"


def _col(*n):
    return np.array([n], dtype=np.uint32).T


def _min_cov(case):
    return max(o.parse_argv(["-i", "in.sam"] + list(case["args"])).min_depth, 1)


def _oracle_sites(idx, min_alt, min_frac):
    """{file name: content} the oracle's counts give: one table per reference with Σcoverage > 0."""
    refs, counts, prefix = tt._oracle(idx)
    mc = _min_cov(CASES[idx])
    return {r + "__" + prefix + ".variants.tsv":
            (HEADER + table.format_sites(tt._c6(counts[r]), 1, mc, min_alt, min_frac)).decode("latin-1")
            for r in refs if sum(sum(c) for c in counts[r]) > 0}


# ---------------------------------------------------------------------------- CPU tier
def test_constants():
    assert table.SITES_HEADER == HEADER and table.SITES_SUFFIX == b".variants.tsv"


def test_tiny_sites_literal():
    idx = next(k for k, c in enumerate(CASES) if c["name"] == "tiny")
    refs, counts, _ = tt._oracle(idx)
    c = tt._c6(counts["g1"])
    assert table.SITES_HEADER + table.format_sites(c, 1, 1, 1, 0.05) == HEADER + b"4\t2\t0\t0\t0\t1\t0\t1\tG\tT\t0.5000\n"
    assert table.SITES_HEADER + table.format_sites(c) == HEADER      # (alt 1 < the default 2 reads)
    assert table.site_mask(c, 1, 1, 0.05).tolist() == [False] * 3 + [True] + [False] * 6


def test_format_sites_numbers():
    big = np.full((6, 1), 4294967295, dtype=np.uint32)
    line = table.format_sites(big, 9999999999)
    assert line == b"9999999999\t25769803770" + b"\t4294967295" * 6 + b"\t-\tACGNT\t0.8333\n"
    assert len(line) == 104
    assert table.format_sites(np.zeros((6, 0), dtype=np.uint32)) == b""
    assert table.site_mask(np.zeros((6, 0), dtype=np.uint32)).shape == (0,)
    with pytest.raises(ValueError):
        table.format_sites(np.zeros((5, 3)))
    with pytest.raises(ValueError):
        table.site_mask(np.zeros((5, 3)))


def test_edges_of_the_rule():
    def site(c, min_cov, min_alt, min_frac):
        m = bool(table.site_mask(c, min_cov, min_alt, min_frac)[0])
        assert (table.format_sites(c, 1, min_cov, min_alt, min_frac) != b"") == m
        return m
    assert site(_col(0, 5, 2, 0, 0, 0), 1, 2, 0.0) and not site(_col(0, 5, 1, 0, 0, 0), 1, 2, 0.0)   # alt == min_alt, − 1
    assert site(_col(0, 3, 1, 0, 0, 0), 1, 1, 0.25)          # 0.25 · 4 == 1.0
    assert not site(_col(0, 4, 1, 0, 0, 0), 1, 1, 0.25)      # 0.25 · 5 > 1
    assert 0.1 * 10.0 == 1.0
    assert site(_col(0, 9, 1, 0, 0, 0), 1, 1, 0.1)
    # cov 10, alt 7 at 0.7: the exact product 6.99999999999999955591… lies halfway between 7.0 and
    # the double below it and rounds to even, 7.0, so by the rule's one fp64 product and compare
    # the position is a site (it is not 7.000000000000001).  Products that do round above the
    # exact integer keep a position out that exact arithmetic would take:
    assert 0.7 * 10.0 == 7.0
    assert site(_col(3, 3, 2, 2, 0, 0), 1, 1, 0.7)
    assert 0.07 * 100.0 > 7.0 and 0.55 * 100.0 > 55.0
    assert not site(_col(93, 7, 0, 0, 0, 0), 1, 1, 0.07)
    assert not site(_col(45, 30, 25, 0, 0, 0), 1, 1, 0.55)
    assert site(_col(27, 3, 0, 0, 0, 0), 1, 1, 0.1) and not site(_col(28, 3, 0, 0, 0, 0), 1, 1, 0.1)
    assert site(_col(92, 8, 0, 0, 0, 0), 1, 1, 0.07)
    assert site(_col(0, 1000, 1, 0, 0, 0), 1, 1, 0.0) and not site(_col(0, 1000, 1, 0, 0, 0), 1, 2, 0.0)   # min_frac 0: min_alt alone
    assert site(_col(0, 2, 1, 0, 0, 0), 3, 1, 0.0) and not site(_col(0, 2, 1, 0, 0, 0), 4, 1, 0.0)           # cov < min_cov
    assert not site(_col(0, 0, 0, 0, 0, 0), 1, 1, 0.0) and not site(_col(0, 9, 0, 0, 0, 0), 1, 1, 0.0)
    assert table.format_sites(_col(2, 0, 2, 0, 1, 2), 7, 1, 1, 0.0) == b"7\t7\t2\t0\t2\t0\t1\t2\t-\tCTN\t0.7142\n"


def _restated(n, min_cov, min_alt, min_frac):
    """None, or the fields (cov, major, alt string, af digits) of a site, from §1 in exact
    arithmetic (the one fp64 product and compare apart)."""
    cov = sum(n)
    rank = [sum(1 for t in range(6) if n[t] > n[s] or (n[t] == n[s] and t < s)) for s in range(6)]
    assert sorted(rank) == list(range(6))
    by_rank = [rank.index(k) for k in range(6)]
    alt = cov - n[by_rank[0]]
    if not (cov >= min_cov and alt >= min_alt and float(alt) >= min_frac * float(cov)):
        return None
    af = Fraction(alt * 10000, cov)
    return cov, SYM[by_rank[0]], "".join(SYM[s] for s in by_rank[1:] if n[s] > 0), "0.%04d" % (af.numerator // af.denominator)


@pytest.mark.parametrize("min_alt,min_frac,n_sites", [(2, 0.05, 1120), (1, 0.0, 4206)], ids=["defaults", "all"])
def test_model_against_restatement_on_every_ok_case(min_alt, min_frac, n_sites):
    """Every field of every line, and no line for a non-site, against the restatement; the
    cases hold enough sites, ties for the major symbol and sites of three or more symbols for
    that to mean something."""
    positions = sites = ties = three = with_sites = ok = 0
    for idx, case in enumerate(CASES):
        if case["status"] != "ok":
            continue
        ok += 1
        refs, counts, _ = tt._oracle(idx)
        mc = _min_cov(case)
        before = sites
        for r, ln in refs.items():
            c = tt._c6(counts[r])
            lines = table.format_sites(c, 1, mc, min_alt, min_frac).decode().split("\n")
            assert lines.pop() == ""
            mask = table.site_mask(c, mc, min_alt, min_frac)
            assert mask.shape == (ln,) and mask.dtype == bool
            want = []
            for p, n in enumerate(counts[r], 1):
                positions += 1
                f = _restated([int(v) for v in n], mc, min_alt, min_frac)
                assert bool(mask[p - 1]) == (f is not None), (case["name"], r, p)
                if f is None:
                    continue
                want.append("\t".join([str(p), str(f[0])] + [str(int(v)) for v in n] + list(f[1:])))
                sites += 1
                ties += sorted(n)[-1] == sorted(n)[-2]
                three += sum(1 for v in n if v) >= 3
            assert lines == want, (case["name"], r)
        with_sites += sites > before
    assert sites == n_sites
    if (min_alt, min_frac) == (2, 0.05):
        assert (ok, with_sites, positions, ties, three) == (1107, 286, 42959, 727, 1068)
        assert sites >= 1000 and ties >= 500 and three >= 1000 and 2 * sites < positions


def test_parser_has_variants_flags():
    from sam2consensus_amd.cli import build_parser, variants_of
    p = build_parser()
    a = p.parse_args(["-i", "x.sam"])
    assert a.variants is False and variants_of(p, a) is None
    a = p.parse_args(["-i", "x.sam", "--variants"])
    assert a.variants is True and variants_of(p, a) == (2, 0.05)
    a = p.parse_args(["-i", "x.sam", "--variants", "--min-alt-reads", "7", "--min-alt-frac", "0.5"])
    assert variants_of(p, a) == (7, 0.5)
    a = p.parse_args(["-i", "x.sam", "--variants", "--min-alt-reads", "1", "--min-alt-frac", "0"])
    assert variants_of(p, a) == (1, 0.0)
    a = p.parse_args(["-i", "x.sam", "--variants", "--min-alt-frac", "1"])
    assert variants_of(p, a) == (2, 1.0)


REFUSED = [({"WORLD_SIZE": "2"}, ["--variants"], "--variants"),
           ({"S2C_STREAM": "1M"}, ["--variants"], "--variants"),
           ({}, ["--variants", "--min-alt-reads", "0"], "--min-alt-reads"),
           ({}, ["--variants", "--min-alt-frac", "1.5"], "--min-alt-frac"),
           ({}, ["--variants", "--min-alt-frac", "nan"], "--min-alt-frac"),
           ({}, ["--min-alt-frac", "0.1"], "--min-alt-frac"),
           ({}, ["--min-alt-reads", "3"], "--min-alt-reads")]


@pytest.mark.parametrize("env,extra,flag", REFUSED,
                         ids=["world2", "stream", "reads0", "frac1.5", "fracnan", "frac-alone", "reads-alone"])
def test_variants_refused(env, extra, flag, tmp_path, monkeypatch, capsys):
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
    assert e.value.code == 2
    assert flag in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == ["in.sam"]


def test_sites_symbols_declared_and_bound():
    from sam2consensus_amd import _lib
    lib = _lib.lib
    assert {"s2c_sites_mark", "s2c_sites_len", "s2c_sites_write"} <= set(_lib.EXPORTS)
    assert lib.s2c_abi_version() == 14
    # (argument errors need no device)
    assert lib.s2c_sites_mark(None, -1, 1, 1, 0.05, None, None) == _lib.S2C_ERR_ARG
    assert lib.s2c_sites_mark(None, 0, 1, 1, 0.05, None, None) == _lib.S2C_OK
    assert lib.s2c_sites_mark(None, 64, 1, 1, 0.05, None, None) == _lib.S2C_ERR_ARG
    for bad in ((0, 1, 0.05), (1, 0, 0.05), (1, 1, -0.01), (1, 1, 1.01), (1, 1, float("nan")), (-3, 1, 0.5)):
        assert lib.s2c_sites_mark(None, 0, *bad, None, None) == _lib.S2C_ERR_ARG, bad
    assert lib.s2c_sites_mark(None, 0, 1, 1, 0.0, None, None) == _lib.S2C_OK
    assert lib.s2c_sites_mark(None, 0, 1, 1, 1.0, None, None) == _lib.S2C_OK
    assert lib.s2c_sites_len(None, 16, None, None, -1, None, None) == _lib.S2C_ERR_ARG
    assert lib.s2c_sites_len(None, -16, None, None, 0, None, None) == _lib.S2C_ERR_ARG
    assert lib.s2c_sites_len(None, 16, None, None, 0, None, None) == _lib.S2C_OK
    assert lib.s2c_sites_len(None, 16, None, None, 1, None, None) == _lib.S2C_ERR_ARG
    assert lib.s2c_sites_write(None, 16, None, None, None, 1, None, -1, None) == _lib.S2C_ERR_ARG
    assert lib.s2c_sites_write(None, 16, None, None, None, -1, None, 0, None) == _lib.S2C_ERR_ARG
    assert lib.s2c_sites_write(None, 16, None, None, None, 0, None, 0, None) == _lib.S2C_OK
    assert lib.s2c_sites_write(None, 16, None, None, None, 1, None, 0, None) == _lib.S2C_ERR_ARG


# ---------------------------------------------------------------------------- GPU tier
PADDED = tt.PADDED
QUIET = (1200, 1900)       # one symbol per position: no site at any parameters; covers [1280, 1792)
SOLID = (1900, 2300)       # every position a site
EMPTY = (2304, 3400)       # no coverage but for the single sites below
SINGLES = [2560, 2560 + 63, 2560 + 64, 2560 + 255, 2816, 3071, 3072, 3399]   # ≡ 0, 63, 64, 255, 0, 255, 0 mod 256
ALTERN = (3400, 3700)      # sites at the even positions
TIES = (3700, 3800)
EDGES = (3800, 3830)
EDGE_ROWS = [(1, 1, 0, 0, 0, 0), (2, 1, 0, 0, 0, 0), (0, 5, 2, 0, 0, 0), (0, 5, 1, 0, 0, 0), (0, 3, 1, 0, 0, 0),
             (0, 9, 1, 0, 0, 0), (3, 3, 2, 2, 0, 0), (18, 1, 1, 0, 0, 0), (27, 3, 0, 0, 0, 0), (27, 2, 1, 0, 0, 0),
             (93, 7, 0, 0, 0, 0), (92, 8, 0, 0, 0, 0), (45, 30, 25, 0, 0, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 9),
             (0, 1000, 1, 0, 0, 0), (0, 0, 90, 0, 10, 0), (0, 0, 91, 0, 9, 0), (0, 0, 0, 2, 0, 1), (1, 1, 1, 0, 0, 0),
             (4294967295, 4294967295, 0, 0, 0, 0), (4294967295, 0, 0, 0, 0, 1), (4294967295, 0, 0, 0, 1, 1),
             (2, 0, 2, 0, 1, 2), (0, 0, 0, 0, 1, 1), (1, 0, 0, 0, 0, 1), (1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1),
             (0, 17, 0, 3, 0, 0), (0, 18, 0, 2, 0, 0)]
TIE_ROWS = [(0, 5, 5, 0, 0, 2), (3, 3, 3, 3, 3, 3), (0, 0, 0, 2, 0, 2), (7, 0, 0, 0, 0, 7), (0, 4, 4, 4, 0, 1),
            (2, 2, 9, 0, 0, 0), (0, 0, 6, 6, 1, 1), (1, 1, 1, 1, 1, 8), (0, 12, 0, 12, 0, 12), (5, 0, 5, 0, 4, 4)]
# test_table.py's blocks (lengths 0, 1, 63, 64, 65, 255, 256, 257 and 2048, odd starts, the 9→10
# and 9999→10000 steps, 10-digit positions) and blocks over the stretches above: odd starts that
# share mask words with their neighbours, blocks that overlap, and two inside SOLID with exactly
# 256 and 257 sites (the queue emits at 256: none left over, and one)
BLOCKS = tt.BLOCKS + [(1100, 2100, 1), (1900, 2156, 1), (1901, 2158, 77), (2100, 2305, 9), (2305, 2561, 1),
                      (2561, 2817, 9998), (2623, 2624, 5), (2624, 2816, 1), (2500, 3500, 999999000), (3399, 3465, 1),
                      (3465, 3830, 97), (3700, 3830, 1), (1050, 1051, 9999999999), (1281, 1791, 1), (1216, 1920, 1)]
PARAMS = [(1, 1, 0.0), (3, 2, 0.1)]


def _synthetic_counts():
    c = tt._synthetic_counts()
    j = np.arange(PADDED)
    c[:, QUIET[0]:QUIET[1]] = 0
    c[j[QUIET[0]:QUIET[1]] % 6, j[QUIET[0]:QUIET[1]]] = 1 + j[QUIET[0]:QUIET[1]] % 1000
    k = j[SOLID[0]:SOLID[1]]
    c[:, SOLID[0]:SOLID[1]] = np.stack([5 + k % 7, 4 + k % 3, 3 + k % 11, k % 2, 0 * k, 1 + k % 5])
    c[:, EMPTY[0]:EMPTY[1]] = 0
    for n, g in enumerate(SINGLES):
        c[:, g] = (0, 40 + n, 0, 0, 9, 1)
    c[:, ALTERN[0]:ALTERN[1]] = 0
    c[1, ALTERN[0]:ALTERN[1]] = 50
    c[5, ALTERN[0]:ALTERN[1]:2] = 10
    for n, g in enumerate(range(*TIES)):
        c[:, g] = TIE_ROWS[n % len(TIE_ROWS)]
    assert EDGES[1] - EDGES[0] == len(EDGE_ROWS)
    c[:, EDGES[0]:EDGES[1]] = np.array(EDGE_ROWS, dtype=np.uint32).T
    return c


def test_synthetic_counts_hold_what_the_kernel_test_needs():
    c = _synthetic_counts()
    for prm in PARAMS:
        m = table.site_mask(c, *prm)
        assert not m[QUIET[0]:QUIET[1]].any() and QUIET[1] - QUIET[0] >= 600
        assert QUIET[0] <= 1280 and 1792 <= QUIET[1]          # two whole aligned sub-blocks of 256
        assert m[SOLID[0]:SOLID[1]].all()
        assert np.flatnonzero(m[EMPTY[0]:EMPTY[1]]).tolist() == [g - EMPTY[0] for g in SINGLES]
        assert m[ALTERN[0]:ALTERN[1]].tolist() == [True, False] * ((ALTERN[1] - ALTERN[0]) // 2)
        assert m[TIES[0]:TIES[1]].all()
        e = m[EDGES[0]:EDGES[1]]
        assert e.any() and not e.all()
        assert m[tt.STRETCH[0]:tt.STRETCH[1]].all()
        assert m[:1000].any()
        assert (1900, 2156, 1) in BLOCKS and (1901, 2158, 77) in BLOCKS
        assert int(m[1900:2156].sum()) == 256 and int(m[1901:2158].sum()) == 257   # the queue emits at 256: none left, one left
    assert not table.site_mask(c, *PARAMS[1])[:1000].all()      # (the digit ladder: sites and others mixed)
    assert {g % 256 for g in SINGLES} >= {0, 63, 64, 255}
    a, b = (table.site_mask(c, *prm)[EDGES[0]:EDGES[1]] for prm in PARAMS)
    assert (a != b).any()


def _dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _sites_mark(counts_d, prm, padded=PADDED):
    import torch
    from sam2consensus_amd import _lib
    words = (padded + 63) // 64
    mask = torch.full((words + 2,), -1, dtype=torch.int64, device="cuda")   # (two guard words)
    _lib.check(_lib.lib.s2c_sites_mark(_ptr(counts_d), padded, prm[0], prm[1], prm[2], _ptr(mask), _stream()))
    return mask


def _sites_len(counts_d, mask, blocks):
    import torch
    from sam2consensus_amd import _lib
    lens = torch.full((len(blocks),), -7, dtype=torch.int64, device="cuda")
    b = tt._dev_i64(blocks)
    _lib.check(_lib.lib.s2c_sites_len(_ptr(counts_d), PADDED, _ptr(mask), _ptr(b), len(blocks), _ptr(lens), _stream()))
    return lens.cpu().numpy()


def _sites_write(counts_d, mask, blocks, offs, dst_len, alloc):
    import torch
    from sam2consensus_amd import _lib
    dst = torch.full((alloc,), 0xEE, dtype=torch.uint8, device="cuda")
    b, f = tt._dev_i64(blocks), tt._dev_i64(offs)
    _lib.check(_lib.lib.s2c_sites_write(_ptr(counts_d), PADDED, _ptr(mask), _ptr(b), _ptr(f), len(blocks),
                                        _ptr(dst), dst_len, _stream()))
    torch.cuda.synchronize()
    return dst.cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("prm", PARAMS, ids=["all", "m3a2f0.1"])
def test_kernels_on_synthetic_counts(prm):
    """k_sites_mark's mask == site_mask over all positions (unused bits zero, no word past the
    mask written), k_sites_len's lengths and k_sites_write's bytes == format_sites block by
    block; a block past padded_len and blocks whose text ends past dst_len are skipped (their
    bytes and the 64 bytes after the text keep their 0xEE); a destination shifted by a byte."""
    import torch
    c = _synthetic_counts()
    counts_d = torch.from_numpy(c.view(np.int32)).cuda()
    want_mask = table.site_mask(c, *prm)
    mask = _sites_mark(counts_d, prm)
    got = mask.cpu().numpy().view(np.uint64)
    assert got[-2:].tolist() == [2 ** 64 - 1] * 2
    bits = np.unpackbits(got[:-2].view(np.uint8), bitorder="little").astype(bool)
    assert bits.shape == (PADDED,) and (bits == want_mask).all(), np.flatnonzero(bits != want_mask)[:10]
    # a length that is no multiple of 64 (rows PADDED apart, so a prefix of each row is not a
    # [6][4000] array: its own counts): the last word's unused bits are zero
    short = np.ascontiguousarray(c[:, :4000])
    m2 = _sites_mark(torch.from_numpy(short.view(np.int32)).cuda(), prm, 4000).cpu().numpy().view(np.uint64)
    assert m2[-2:].tolist() == [2 ** 64 - 1] * 2 and len(m2) == 63 + 2
    bits2 = np.unpackbits(m2[:-2].view(np.uint8), bitorder="little").astype(bool)
    assert (bits2[:4000] == want_mask[:4000]).all() and not bits2[4000:].any() and want_mask[3968:4000].any()

    want = [table.format_sites(c[:, a:b], p0, *prm) for a, b, p0 in BLOCKS]
    assert b"\n10\t" in want[3] and b"\n10000\t" in want[4] and want[BLOCKS.index((1050, 1051, 9999999999))].startswith(b"9999999999\t25769803770\t")
    assert b"\t25769803770\t" in want[5] and want[5].count(b"\t-\tACGNT\t0.8333\n") >= 100
    assert want[BLOCKS.index((1281, 1791, 1))] == b"" and want[BLOCKS.index((1216, 1920, 1))].count(b"\n") == 20
    assert want[BLOCKS.index((2623, 2624, 5))].startswith(b"5\t51\t0\t41\t0\t0\t9\t1\tA\tNT\t0.1960\n")
    bad = (4000, PADDED + 1, 1)                       # b > padded_len: skipped
    blocks = BLOCKS[:6] + [bad] + BLOCKS[6:]
    lens = _sites_len(counts_d, mask, blocks)
    assert lens[6] == 0
    assert [int(v) for v in np.delete(lens, 6)] == [len(w) for w in want]
    # the refused block gets 100 bytes of its own in dst: they must stay untouched
    room = [len(w) for w in want[:6]] + [100] + [len(w) for w in want[6:]]
    offs = np.concatenate([[0], np.cumsum(room)])
    total = int(offs[-1])
    got = _sites_write(counts_d, mask, blocks, offs, total, total + 64)
    texts = want[:6] + [b"\xEE" * 100] + want[6:]
    for k, w in enumerate(texts):
        assert got[offs[k]:offs[k + 1]] == w, (blocks[k], tt._first_diff(got[offs[k]:offs[k + 1]], w))
    assert got[total:] == b"\xEE" * 64
    # dst_len cut inside the last three blocks' text (the last but one is empty at its end:
    # it ends past the cut too): they are skipped, the others written
    assert len(texts[-1]) > 0 and len(texts[-3]) > 5
    cut = int(offs[-4]) + 5
    got = _sites_write(counts_d, mask, blocks, offs, cut, total + 64)
    assert got[:offs[-4]] == b"".join(texts[:-3])
    assert got[offs[-4]:] == b"\xEE" * (total + 64 - int(offs[-4]))
    # an odd destination: every block's text shifted by one byte
    got = _sites_write(counts_d, mask, blocks, offs + 1, total + 1, total + 65)
    assert got[:1] == b"\xEE" and got[1:total + 1] == b"".join(texts) and got[total + 1:] == b"\xEE" * 64


E2E_ARGS = ["--variants", "--min-alt-reads", "1", "--min-alt-frac", "0.1"]


def _check_case(idx, extra, min_alt, min_frac):
    from sam2consensus_amd.cli import run_text
    case = CASES[idx]
    status, files = run_text(case["sam"], list(case["args"]) + extra)
    assert status == case["status"]
    if status != "ok":
        assert files == {}
        return
    assert {k: v for k, v in files.items() if k.endswith(".fasta")} == case["files"]
    assert {k: v for k, v in files.items() if not k.endswith(".fasta")} == _oracle_sites(idx, min_alt, min_frac)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_golden_cases_with_variants(idx):
    """run_text with --variants: the case's status; on ok the reference's FASTA files and one
    table per reference with Σcoverage > 0, equal to the oracle's counts through format_sites,
    the least coverage the case's -m."""
    _check_case(idx, E2E_ARGS, 1, 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(KAT), ids=[c["name"] for c in CASES[:KAT]])
def test_kat_cases_with_variants_at_the_defaults(idx):
    _check_case(idx, ["--variants"], 2, 0.05)


def _model_counts(hb):
    import batch_model as bm
    runs, _ = bm.model_reads(hb)
    return bm.model_counts(hb, runs)


def _model_sites(hb, want, prefix, min_cov, min_alt, min_frac):
    out = {}
    for r in range(hb.info.n_refs):
        if hb.ref_reads[r] > 0:
            a, ln = int(hb.ref_off[r]), int(hb.ref_len[r])
            out[hb.names[r].encode() + b"__" + prefix + b".variants.tsv"] = \
                HEADER + table.format_sites(want[:, a:a + ln], 1, min_cov, min_alt, min_frac)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,over", tt.TILE_KINDS, ids=[n for n, _ in tt.TILE_KINDS])
def test_every_tile_kind(name, over):
    """General tiles with insertions (c2), dense tiles (c5), maxdel drops (c5nd), deep tiles
    (c4): the variants files == the batch model's counts through format_sites; --counts and
    --variants together give what each gives alone; the FASTA files of all three == the fused
    route's."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch(name, **over)
    prm = (2, 0.0) if name == "c4" else (2, 0.05)   # (c4: 12,000 reads deep, its minorities far below 5 %)
    plain = consensus_batch(hb, [0.25, 0.75], b"x")
    cnt = consensus_batch(hb, [0.25, 0.75], b"x", counts=True)
    var = consensus_batch(hb, [0.25, 0.75], b"x", variants=prm)
    both = consensus_batch(hb, [0.25, 0.75], b"x", counts=True, variants=prm)
    nf = len(plain)
    assert plain and list(var)[:nf] == list(plain) and list(both)[:len(cnt)] == list(cnt)
    for k, v in plain.items():
        assert var[k] == v and both[k] == v and cnt[k] == v, (k, tt._first_diff(var[k], v))
    want = _model_sites(hb, _model_counts(hb), b"x", 1, *prm)
    assert list(var)[nf:] == list(both)[len(cnt):] and sorted(list(var)[nf:]) == sorted(want)
    assert not any(k.endswith(b".counts.tsv") for k in var)
    lines = 0
    for k, v in want.items():
        assert var[k] == v, (k, tt._first_diff(var[k], v))
        assert both[k] == v, (k, tt._first_diff(both[k], v))
        lines += v.count(b"\n") - 1
    assert lines > 0, "the configuration must hold sites"
    for k, v in cnt.items():
        assert both[k] == v, (k, tt._first_diff(both[k], v))
    assert len(both) == len(cnt) + len(want)


@pytest.mark.gpu
def test_min_depth_is_the_least_coverage():
    """-m above 1 raises the sites' least coverage (and only then: -m 0 is 1)."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch("c2", n_refs=3)
    counts = _model_counts(hb)
    got = {}
    for m in (0, 1, 30):
        files = consensus_batch(hb, [0.25], b"x", min_depth=m, variants=(1, 0.0))
        got[m] = {k: v for k, v in files.items() if k.endswith(b".variants.tsv")}
        assert got[m] == _model_sites(hb, counts, b"x", max(m, 1), 1, 0.0)
    assert got[0] == got[1] != got[30]


@pytest.mark.gpu
def test_workspace_reuse():
    """run_with_tables twice on one workspace: the same tables and FASTA results (the counts
    are zeroed again before the second run); a variants-only run returns no count table;
    run_with_counts() still returns the count tables; a plain run() on a fresh workspace is
    unchanged."""
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
        ws.sites_table(1, 2, 0.05)          # (nothing has filled the counts)
    with pytest.raises(ValueError):
        Workspace(DeviceBatch(hb), [0.25]).run_with_tables({"variants": (1, 2, 0.05)})
    runs = []
    for _ in range(2):
        res = ws.run_with_tables({"variants": (1, 2, 0.05)})
        assert set(res) == {"variants"}
        stab = res["variants"]
        runs.append((stab[0].tobytes(), stab[1].cpu().numpy().tobytes(), fetched(ws)))
    assert runs[0] == runs[1]
    assert runs[0][2] == base
    want = _model_sites(hb, _model_counts(hb), b"x", 1, 2, 0.05)
    assert table.table_files(hb, b"x", stab[0], runs[0][1], table.SITES_HEADER, table.SITES_SUFFIX) == want
    both = ws.run_with_tables({"counts": (), "variants": (1, 2, 0.05)})
    ctab, stab2 = both["counts"], both["variants"]
    assert (stab2[0].tobytes(), stab2[1].cpu().numpy().tobytes()) == runs[0][:2] and fetched(ws) == base
    offs, text = ws.run_with_counts()
    assert offs.tobytes() == ctab[0].tobytes() and text.cpu().numpy().tobytes() == ctab[1].cpu().numpy().tobytes()
    assert table.table_files(hb, b"x", offs, text.cpu().numpy().tobytes()) == tt._model_tables(hb, b"x")
    assert fetched(ws) == base
    ws1 = Workspace(DeviceBatch(hb), [0.25])
    ws1.run()
    assert fetched(ws1) == base
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_cli_process_variants_c1(tmp_path):
    """sam2consensus.py --variants, and --counts --variants, on the full C1 (10 x 1,000 bp): the
    reference's 10 FASTA files, 10 variants files equal to the model's over the count tables'
    rows, stdout exact (the variant lines after the count lines, before Done.); without the flag
    stdout and files as before."""
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
    for tag, extra in (("plain", []), ("variants", ["--variants"]), ("both", ["--variants", "--counts"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(root, "sam2consensus.py"), "-i", sam, "-o", str(out)] +
                           g["args"] + extra, capture_output=True, text=True, timeout=240, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (r.stdout, {fn: open(os.path.join(out, fn), "rb").read() for fn in os.listdir(out)})

    def saved(d, what, suffix):
        return "".join("%s saved for %s in: %s/%s__c1.%s\n" % (what, n, d, n, suffix) for n in names)

    golden = {k: v["sha256"] for k, v in g["files"].items()}
    so, files = outs["plain"]
    d = str(tmp_path / "plain")
    assert so == tt.C1_STDOUT.format(sam=sam, n=n_reads, m=n_mapped, saved=saved(d, "Consensus sequence at 25%", "fasta"))
    assert {k: hashlib.sha256(v).hexdigest() for k, v in files.items()} == golden
    so, both = outs["both"]
    d = str(tmp_path / "both")
    assert so == tt.C1_STDOUT.format(sam=sam, n=n_reads, m=n_mapped, saved=saved(d, "Consensus sequence at 25%", "fasta") +
                                     saved(d, "Count table", "counts.tsv") + saved(d, "Variant table", "variants.tsv"))
    so, files = outs["variants"]
    d = str(tmp_path / "variants")
    assert so == tt.C1_STDOUT.format(sam=sam, n=n_reads, m=n_mapped, saved=saved(d, "Consensus sequence at 25%", "fasta") +
                                     saved(d, "Variant table", "variants.tsv"))
    min_cov = max(o.parse_argv(["-i", "in.sam"] + list(g["args"])).min_depth, 1)
    n_lines = 0
    for fs in (files, both):
        fa = {k: v for k, v in fs.items() if k.endswith(".fasta")}
        assert {k: hashlib.sha256(v).hexdigest() for k, v in fa.items()} == golden
        assert sorted(k for k in fs if k.endswith(".variants.tsv")) == sorted(n + "__c1.variants.tsv" for n in names)
    assert len(files) == 20 and len(both) == 30
    for n in names:
        rows = both[n + "__c1.counts.tsv"].split(b"\n")[1:-1]
        c = np.array([[int(x) for x in row.split(b"\t")[2:]] for row in rows], dtype=np.int64).T
        want = HEADER + table.format_sites(c, 1, min_cov, 2, 0.05)
        assert files[n + "__c1.variants.tsv"] == want == both[n + "__c1.variants.tsv"], n
        n_lines += want.count(b"\n") - 1
    assert n_lines > 0
