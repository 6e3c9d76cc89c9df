"""--counts: the per-position count tables (sam2consensus_amd/table.py, csrc/s2c_table.hip).

Without a GPU: the row format against the oracle's pileup on every golden case, the flag and
its refused combinations.  On the GPU: the two kernels alone on synthetic counts (every digit
count, an 11-digit coverage, 10-digit positions, block lengths around the wave and sub-block
sizes, the guards), the golden cases end to end, every tile kind against the batch model, a
reused workspace, and the CLI process on C1."""
import functools
import hashlib
import os

import numpy as np
import pytest

import batch_model as bm
from devmem import _dev_i64
import golden_io
import s2c_oracle as o

from sam2consensus_amd import table

CASES = golden_io.cases()
CONFIGS = golden_io.load("configs")

TINY_TABLE = ("pos\tcov\t-\tA\tC\tG\tN\tT\n"
              "1\t1\t0\t1\t0\t0\t0\t0\n"
              "2\t2\t0\t2\t0\t0\t0\t0\n"
              "3\t2\t0\t2\t0\t0\t0\t0\n"
              "4\t2\t0\t0\t0\t1\t0\t1\n"
              "5\t2\t0\t0\t0\t2\t0\t0\n"
              "6\t1\t0\t0\t0\t1\t0\t0\n"
              "7\t0\t0\t0\t0\t0\t0\t0\n"
              "8\t0\t0\t0\t0\t0\t0\t0\n"
              "9\t0\t0\t0\t0\t0\t0\t0\n"
              "10\t0\t0\t0\t0\t0\t0\t0\n").encode()


def _c6(per_pos):
    """The oracle's counts[pos][code] of one reference as [6][L]."""
    return np.array(per_pos, dtype=np.int64).reshape(-1, 6).T


@functools.lru_cache(maxsize=None)
def _oracle(idx):
    """(refs, counts) of golden case idx from the oracle's two passes; its prefix."""
    case = CASES[idx]
    opt = o.parse_argv(["-i", "in.sam"] + list(case["args"]))
    lines = o._lines(case["sam"])
    refs = o.read_header(lines)
    counts, _ = o.pileup(lines, refs, opt)
    return refs, counts, opt.prefix


def _oracle_tables(idx):
    """{file name: content} the oracle's counts give: one table per reference with Σcoverage > 0."""
    refs, counts, prefix = _oracle(idx)
    return {r + "__" + prefix + ".counts.tsv": (table.HEADER + table.format_rows(_c6(counts[r]))).decode("latin-1")
            for r in refs if sum(sum(c) for c in counts[r]) > 0}


# ---------------------------------------------------------------------------- CPU tier
def test_tiny_table_literal():
    idx = next(k for k, c in enumerate(CASES) if c["name"] == "tiny")
    refs, counts, _ = _oracle(idx)
    assert list(refs) == ["g1"] and refs["g1"] == 10
    assert table.HEADER + table.format_rows(_c6(counts["g1"])) == TINY_TABLE


def test_format_rows_numbers():
    big = np.full((6, 2), 4294967295, dtype=np.uint32)
    assert table.format_rows(big, 999999999) == (
        b"999999999\t25769803770" + b"\t4294967295" * 6 + b"\n1000000000\t25769803770" + b"\t4294967295" * 6 + b"\n")
    assert table.format_rows(np.zeros((6, 0), dtype=np.uint32)) == b""
    with pytest.raises(ValueError):
        table.format_rows(np.zeros((5, 3)))


def test_rows_equal_oracle_counts_on_every_ok_case():
    """Row p of a reference's table: the six counts of pileup[ref][p - 1] in order, and the
    coverage the oracle's consensus uses there (sum of the six, :237)."""
    n = 0
    for idx, case in enumerate(CASES):
        if case["status"] != "ok":
            continue
        refs, counts, _ = _oracle(idx)
        for r, ln in refs.items():
            rows = table.format_rows(_c6(counts[r])).decode().split("\n")
            assert rows.pop() == "" and len(rows) == ln == len(counts[r]), (case["name"], r)
            for p, row in enumerate(rows, 1):
                f = row.split("\t")
                assert f[0] == str(p) and f[1] == str(sum(counts[r][p - 1])), (case["name"], r, p)
                assert f[2:] == [str(v) for v in counts[r][p - 1]], (case["name"], r, p)
                n += 1
    assert n > 0


def test_parser_has_counts_flag():
    from sam2consensus_amd.cli import build_parser
    assert build_parser().parse_args(["-i", "x.sam"]).counts is False
    assert build_parser().parse_args(["-i", "x.sam", "--counts"]).counts is True
    with pytest.raises(TypeError):
        table.request(bogus=True)


def test_registry_flags_and_refusals(tmp_path, monkeypatch, capsys):
    """Every entry of table.TABLES: the parser has the flag -- + key; main with more than one
    process, and with streamed batches, exits 2 naming that flag and leaves the folder empty.
    table.request: the public keyword forms as one mapping in TABLES order."""
    from sam2consensus_amd.cli import build_parser, main
    assert [t.key for t in table.TABLES] == ["counts", "variants", "depth", "lowcov", "insertions", "links"]
    assert table.request(links=[1, 0.0, 2], insertions=3, depth=True, lowcov=False, variants=None, counts=True) == \
        {"counts": (), "depth": (), "insertions": (3,), "links": (1, 0.0, 2)}
    assert list(table.request(links=(1, 0.0, 2), counts=True)) == ["counts", "links"] and table.request() == {}
    sam = tmp_path / "in.sam"
    sam.write_text("@SQ\tSN:g1\tLN:10\nr\t0\tg1\t1\t60\t4M\t*\t0\t0\tAATG\t*\n")
    monkeypatch.chdir(tmp_path)
    for t in table.TABLES:
        flag = "--" + t.key
        assert getattr(build_parser().parse_args(["-i", "x.sam", flag]), t.key) is True
        for env, word in (("WORLD_SIZE", "2"), ("S2C_STREAM", "1M")):
            for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2C_STREAM"):
                monkeypatch.delenv(k, raising=False)
            monkeypatch.setenv(env, word)
            with pytest.raises(SystemExit) as e:
                main(["-i", str(sam), flag, "-o", str(tmp_path / "out")])
            assert e.value.code == 2 and flag + " is not available with" in capsys.readouterr().err
            assert sorted(os.listdir(tmp_path)) == ["in.sam"]


@pytest.mark.parametrize("env", [{"WORLD_SIZE": "2"}, {"S2C_STREAM": "1M"}], ids=["world2", "stream"])
def test_counts_refused_combinations(env, tmp_path, monkeypatch, capsys):
    """--counts with more than one process or with streamed batches: the argparse error,
    before a folder is made or a device touched."""
    from sam2consensus_amd.cli import main
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2C_STREAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sam = tmp_path / "in.sam"
    sam.write_text("@SQ\tSN:g1\tLN:10\nr\t0\tg1\t1\t60\t4M\t*\t0\t0\tAATG\t*\n")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(["-i", str(sam), "--counts", "-o", str(tmp_path / "out")])
    assert e.value.code == 2
    assert "--counts" in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == ["in.sam"]


def test_table_symbols_declared_and_bound():
    from sam2consensus_amd import _lib
    assert {"s2c_table_len", "s2c_table_write"} <= set(_lib.EXPORTS)
    assert _lib.lib.s2c_abi_version() == 14
    # (argument errors need no device)
    assert _lib.lib.s2c_table_len(None, 16, None, -1, None, None) == _lib.S2C_ERR_ARG
    assert _lib.lib.s2c_table_len(None, 16, None, 0, None, None) == _lib.S2C_OK
    assert _lib.lib.s2c_table_len(None, 16, None, 1, None, None) == _lib.S2C_ERR_ARG
    assert _lib.lib.s2c_table_write(None, 16, None, None, 1, None, -1, None) == _lib.S2C_ERR_ARG
    assert _lib.lib.s2c_table_write(None, 16, None, None, 0, None, 0, None) == _lib.S2C_OK
    assert _lib.lib.s2c_table_write(None, 16, None, None, 1, None, 0, None) == _lib.S2C_ERR_ARG


# ---------------------------------------------------------------------------- GPU tier
PADDED = 4096
DIGITS = [0] + [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [4294967295]
STRETCH = (1000, 1100)   # all six counts 4294967295: coverage 25769803770 (11 digits, above 2^32)
# {a, b, p0}: lengths 0, 1, 63, 64, 65, 255, 256, 257 and 2048; odd starts; a 9→10, 99→100 and
# 9999→10000 step inside a block; 10-digit positions
BLOCKS = [(0, 0, 1), (3, 4, 1), (3, 66, 95), (64, 128, 1), (100, 165, 9995), (900, 1155, 999999990),
          (1024, 1280, 1), (1279, 1536, 95), (2048, 4096, 9995), (0, 2048, 1), (4095, 4096, 9999999999)]


def _synthetic_counts():
    j = np.arange(PADDED)
    c = np.stack([np.array(DIGITS, dtype=np.uint64)[(j * st + s) % len(DIGITS)]
                  for s, st in enumerate((1, 3, 7, 9, 11, 13))]).astype(np.uint32)
    c[:, STRETCH[0]:STRETCH[1]] = 4294967295
    return c


def _table_len(counts_d, blocks):
    import ctypes as C
    import torch
    from sam2consensus_amd import _lib
    lens = torch.full((len(blocks),), -7, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    b = _dev_i64(blocks)
    _lib.check(_lib.lib.s2c_table_len(C.c_void_p(counts_d.data_ptr()), PADDED, C.c_void_p(b.data_ptr()),
                                      len(blocks), C.c_void_p(lens.data_ptr()), st))
    return lens.cpu().numpy()


def _table_write(counts_d, blocks, offs, dst_len, alloc):
    import ctypes as C
    import torch
    from sam2consensus_amd import _lib
    dst = torch.full((alloc,), 0xEE, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    b, f = _dev_i64(blocks), _dev_i64(offs)
    _lib.check(_lib.lib.s2c_table_write(C.c_void_p(counts_d.data_ptr()), PADDED, C.c_void_p(b.data_ptr()),
                                        C.c_void_p(f.data_ptr()), len(blocks), C.c_void_p(dst.data_ptr()), dst_len, st))
    torch.cuda.synchronize()
    return dst.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_kernels_on_synthetic_counts():
    """k_table_len's lengths and k_table_write's bytes == format_rows, block by block; a block
    past padded_len and a block whose text ends past dst_len are skipped (their bytes and the
    64 bytes after the text keep their 0xEE)."""
    import torch
    c = _synthetic_counts()
    assert int(c[:, STRETCH[0]].astype(np.uint64).sum()) == 25769803770
    counts_d = torch.from_numpy(c.view(np.int32)).cuda()
    want = [table.format_rows(c[:, a:b], p0) for a, b, p0 in BLOCKS]
    assert b"\n9\t" in want[3] and b"\n10\t" in want[3] and b"\n100\t" in want[2] and b"\n10000\t" in want[4]
    assert b"\n1000000000\t" in want[5] and b"\t25769803770\t" in want[5] and want[10].startswith(b"9999999999\t")
    bad = (4000, PADDED + 1, 1)                       # b > padded_len: skipped
    blocks = BLOCKS[:6] + [bad] + BLOCKS[6:]
    lens = _table_len(counts_d, blocks)
    assert lens[6] == 0
    assert [int(v) for v in np.delete(lens, 6)] == [len(w) for w in want]
    # the refused block gets 100 bytes of its own in dst: they must stay untouched
    room = [len(w) for w in want[:6]] + [100] + [len(w) for w in want[6:]]
    offs = np.concatenate([[0], np.cumsum(room)])
    total = int(offs[-1])
    got = _table_write(counts_d, blocks, offs, total, total + 64)
    texts = want[:6] + [b"\xEE" * 100] + want[6:]
    for k, w in enumerate(texts):
        assert got[offs[k]:offs[k + 1]] == w, (blocks[k], got[offs[k]:offs[k] + 60], w[:60])
    assert got[total:] == b"\xEE" * 64
    # dst_len cut inside the last two blocks' text: both are skipped, the others written
    cut = int(offs[-3]) + 5
    got = _table_write(counts_d, blocks, offs, cut, total + 64)
    assert got[:offs[-3]] == b"".join(texts[:-2])
    assert got[offs[-3]:] == b"\xEE" * (total + 64 - int(offs[-3]))
    # an odd destination: every block's text shifted by one byte
    got = _table_write(counts_d, blocks, offs + 1, total + 1, total + 65)
    assert got[:1] == b"\xEE" and got[1:total + 1] == b"".join(texts) and got[total + 1:] == b"\xEE" * 64


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_golden_cases_with_counts(idx):
    """run_text with --counts: the case's status; on ok the reference's FASTA files and one
    table per reference with Σcoverage > 0, equal to the oracle's counts formatted."""
    from sam2consensus_amd.cli import run_text
    case = CASES[idx]
    status, files = run_text(case["sam"], list(case["args"]) + ["--counts"])
    assert status == case["status"]
    if status != "ok":
        assert files == {}
        return
    assert {k: v for k, v in files.items() if k.endswith(".fasta")} == case["files"]
    assert {k: v for k, v in files.items() if not k.endswith(".fasta")} == _oracle_tables(idx)


TILE_KINDS = [("c2", {"n_refs": 18}), ("c5", {"ref_len": 400_000}), ("c5nd", {"ref_len": 400_000, "long_del_frac": 0.05}),
              ("c4", {"ref_len": 2000, "depth": 12000.0})]


def _model_tables(hb, prefix):
    runs, _ = bm.model_reads(hb)
    want = bm.model_counts(hb, runs)
    out = {}
    for r in range(hb.info.n_refs):
        if hb.ref_reads[r] > 0:
            a, ln = int(hb.ref_off[r]), int(hb.ref_len[r])
            out[hb.names[r].encode() + b"__" + prefix + b".counts.tsv"] = table.HEADER + table.format_rows(want[:, a:a + ln])
    return out


def _first_diff(a, b):
    n = min(len(a), len(b))
    i = next((k for k in range(n) if a[k] != b[k]), n)
    return "lengths %d / %d, first difference at byte %d: %r vs %r" % (len(a), len(b), i, a[i:i + 40], b[i:i + 40])


@pytest.mark.gpu
@pytest.mark.parametrize("name,over", TILE_KINDS, ids=[n for n, _ in TILE_KINDS])
def test_every_tile_kind(name, over):
    """General tiles with insertions (c2), dense tiles (c5), maxdel drops (c5nd), deep tiles
    (c4): the tables == the batch model's counts formatted; the FASTA files of the counts route
    == the fused route's."""
    from sam2consensus_amd import configs
    from sam2consensus_amd.cli import consensus_batch
    hb = configs.synth_batch(name, **over)
    if name.startswith("c5"):
        assert hb.info.n_dense > 0
    if name == "c4":
        assert (hb.tiles[:, 3] & 1 == 1).any(), "deep config must exercise chunked (atomic) tiles"
    plain = consensus_batch(hb, [0.25, 0.75], b"x")
    both = consensus_batch(hb, [0.25, 0.75], b"x", counts=True)
    assert plain and list(both)[:len(plain)] == list(plain)
    for k, v in plain.items():
        assert both[k] == v, (k, _first_diff(both[k], v))
    want = _model_tables(hb, b"x")
    assert sorted(k for k in both if k not in plain) == sorted(want)
    for k, v in want.items():
        assert both[k] == v, (k, _first_diff(both[k], v))


@pytest.mark.gpu
def test_workspace_reuse():
    """run_with_counts twice on one workspace: the same tables and FASTA results (the counts
    are zeroed again before the second run); a plain run() on a fresh workspace is unchanged."""
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
        ws.counts_table()          # (nothing has filled the counts)
    runs = []
    for _ in range(2):
        offs, text = ws.run_with_counts()
        runs.append((offs.tobytes(), text.cpu().numpy().tobytes(), fetched(ws)))
    assert runs[0] == runs[1]
    assert runs[0][2] == base
    want = _model_tables(hb, b"x")
    got = table.table_files(hb, b"x", offs, runs[0][1])
    assert got == want
    ws1 = Workspace(DeviceBatch(hb), [0.25])
    ws1.run()
    assert fetched(ws1) == base
    torch.cuda.synchronize()


C1_STDOUT = ("\nProcessing file {sam}:\n\n"
             "SAM header processed, 10 references found.\n\n"
             "0 reads processed.\n"
             "A total of {n} reads were processed, out of which, {m} reads were mapped.\n\n"
             "{saved}"
             "Done.\n\n")


@pytest.mark.gpu
def test_cli_process_counts_c1(tmp_path):
    """sam2consensus.py --counts on the full C1 (10 x 1,000 bp): the reference's 10 FASTA
    files, 10 tables of 1,001 lines whose coverage sums to the batch's aligned bases, the
    table lines after the consensus lines; without the flag stdout and files as before."""
    import subprocess
    import sys
    from sam2consensus_amd import configs
    from sam2consensus_amd.batch import parse_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = CONFIGS["c1"]
    sam = str(tmp_path / "c1.sam")
    configs.synth_write("c1", sam)
    hb = parse_file(sam)
    aligned, names = hb.aligned_bases, list(hb.names)
    n_reads, n_mapped = int(hb.info.lines_total - hb.info.header_lines), int(hb.info.reads_mapped)
    assert hb.info.n_refs == 10 and 0 < n_reads < 500000
    hb.free()
    outs = {}
    for tag, extra in (("plain", []), ("counts", ["--counts"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, os.path.join(root, "sam2consensus.py"), "-i", sam, "-o", str(out)] +
                           g["args"] + extra, capture_output=True, text=True, timeout=240, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (r.stdout, {fn: open(os.path.join(out, fn), "rb").read() for fn in os.listdir(out)})

    def saved(d):
        return "".join("Consensus sequence at 25%% saved for %s in: %s/%s__c1.fasta\n" % (n, d, n) for n in names)

    so, files = outs["plain"]
    assert so == C1_STDOUT.format(sam=sam, n=n_reads, m=n_mapped, saved=saved(str(tmp_path / "plain")))
    assert {k: hashlib.sha256(v).hexdigest() for k, v in files.items()} == {k: v["sha256"] for k, v in g["files"].items()}
    so, files = outs["counts"]
    d = str(tmp_path / "counts")
    tabs = "".join("Count table saved for %s in: %s/%s__c1.counts.tsv\n" % (n, d, n) for n in names)
    assert so == C1_STDOUT.format(sam=sam, n=n_reads, m=n_mapped, saved=saved(d) + tabs)
    fa = {k: v for k, v in files.items() if k.endswith(".fasta")}
    tb = {k: v for k, v in files.items() if k.endswith(".counts.tsv")}
    assert len(fa) + len(tb) == len(files) and len(tb) == 10
    assert {k: hashlib.sha256(v).hexdigest() for k, v in fa.items()} == {k: v["sha256"] for k, v in g["files"].items()}
    cov = 0
    for k, v in tb.items():
        rows = v.split(b"\n")
        assert rows[0] + b"\n" == table.HEADER and rows[-1] == b"" and len(rows) == 1002, k
        for p, row in enumerate(rows[1:-1], 1):
            f = [int(x) for x in row.split(b"\t")]
            assert f[0] == p and f[1] == sum(f[2:]) and len(f) == 8, (k, p)
            cov += f[1]
    assert cov == aligned
