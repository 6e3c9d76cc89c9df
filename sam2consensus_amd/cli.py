"""Drop-in ``sam2consensus.py`` command line (reference sam2consensus.py:86-430).

Same flags, same outputs (``outfolder/REF__PREFIX.fasta``), same stdout text and the
same failure behaviour: the reference's exception class propagates (traceback, exit
status 1) and no FASTA file is written.  The pileup-and-vote work runs on the GPU
through libs2c.so; host SAM parsing runs in libs2c.so's C++ parser.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

from . import table

__version__ = "2.1"
DESCRIPTION = """
+------------------------------------------------------------------+
| sam2consensus.py: extract the consensus sequence from a SAM file |
+------------------------------------------------------------------+

Consensus sequences (Geneious threshold rule, IUPAC ambiguity codes) from reads mapped
to one or more references (.sam or .sam.gz), one FASTA file per reference with one
record per consensus threshold.  MI355X implementation: pileup, insertion and vote run
as HIP kernels (libs2c.so); output is byte-identical to sam2consensus.py v2.1.
"""


def build_parser():
    p = argparse.ArgumentParser(description=DESCRIPTION, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-i", "--input", action="store", dest="filename", required=True,
                   help="Name of the SAM file, SAM does not need to be sorted and can be compressed with gzip")
    p.add_argument("-c", "--consensus-thresholds", action="store", dest="thresholds", type=str, default="0.25",
                   help="List of consensus thresold(s) separated by commas, no spaces, example: -c 0.25,0.75,0.50, default=0.25")
    p.add_argument("-n", action="store", dest="n", type=int, default=0,
                   help="Split FASTA output sequences every n nucleotides, default=do not split sequence")
    p.add_argument("-o", "--outfolder", action="store", dest="outfolder", default="./",
                   help="Name of output folder, default=same folder as input")
    p.add_argument("-p", "--prefix", action="store", dest="prefix", default="",
                   help="Prefix for output file name, default=input filename without .sam extension")
    p.add_argument("-m", "--min-depth", action="store", dest="min_depth", type=int, default=1,
                   help="Minimum read depth at each site to report the nucleotide in the consensus, default=1")
    p.add_argument("-f", "--fill", action="store", dest="fill", default="-",
                   help="Character for padding regions not covered in the reference, default= - (gap)")
    # no type= on purpose (:102): a given -d stays a string, which Python 2 compares
    # as greater than every int, so the maxdel filter (:210) is then never applied.
    p.add_argument("-d", "--maxdel", action="store", dest="maxdel", default=150,
                   help="Ignore deletions longer than this value, default=150")
    p.add_argument("--counts", action="store_true", dest="counts", default=False,
                   help="Also write REF__PREFIX.counts.tsv beside each FASTA file: one line per reference position "
                        "with the position, the coverage and the counts of -, A, C, G, N, T (tab-separated; "
                        "insertion columns are not part of the table; independent of -c, -m, -f and -n). "
                        "Not available with more than one process or with S2C_STREAM")
    p.add_argument("--variants", action="store_true", dest="variants", default=False,
                   help="Also write REF__PREFIX.variants.tsv beside each FASTA file: the --counts line of every "
                        "position where a minority is present (coverage at least max(-m, 1), at least "
                        "--min-alt-reads reads not of the major symbol, and at least --min-alt-frac of the "
                        "coverage), followed by the major symbol, the other symbols present in order of their "
                        "counts, and the minority's share of the coverage; all six symbols take part, - and N "
                        "included; insertion columns are not part of the table. "
                        "Not available with more than one process or with S2C_STREAM")
    p.add_argument("--depth", action="store_true", dest="depth", default=False,
                   help="Also write REF__PREFIX.depth.tsv beside each FASTA file: one line start, end, cov "
                        "(tab-separated, 1-based, inclusive) per maximal run of positions with the same coverage, "
                        "uncovered runs included, and one PREFIX.depth_summary.tsv with a line per reference: "
                        "its length, the positions with coverage >= 1 and >= max(-m, 1), the sum, least and "
                        "largest coverage and the number of runs. "
                        "Not available with more than one process or with S2C_STREAM")
    p.add_argument("--lowcov", action="store_true", dest="lowcov", default=False,
                   help="Also write REF__PREFIX.lowcov.tsv beside each FASTA file: one line start, end per "
                        "maximal run of positions with coverage below max(-m, 1), where the consensus holds "
                        "the -f character. Not available with more than one process or with S2C_STREAM")
    p.add_argument("--insertions", action="store_true", dest="insertions", default=False,
                   help="Also write REF__PREFIX.insertions.tsv beside each FASTA file: one line pos, cov, reads, len, "
                        "motif (tab-separated) per distinct insertion motif at a position: the 1-based position whose "
                        "consensus letter the inserted columns follow, the coverage there, the reads carrying exactly "
                        "this motif, its length and its characters; ordered by position, then reads (falling), "
                        "length and motif; independent of -c, -m, -f, -n and -d. "
                        "Not available with more than one process or with S2C_STREAM")
    p.add_argument("--min-ins-reads", action="store", dest="min_ins_reads", type=int, default=None, metavar="N",
                   help="With --insertions: list a motif only when at least N reads carry it, default=1")
    p.add_argument("--min-alt-reads", action="store", dest="min_alt_reads", type=int, default=None, metavar="N",
                   help="With --variants or --links: least number of reads not of the major symbol at a site, default=2")
    p.add_argument("--min-alt-frac", action="store", dest="min_alt_frac", type=float, default=None, metavar="F",
                   help="With --variants or --links: least share of the coverage not of the major symbol at a site, "
                        "between 0 and 1, default=0.05")
    p.add_argument("--links", action="store_true", dest="links", default=False,
                   help="Also write REF__PREFIX.links.tsv beside each FASTA file: one line pos1, pos2, reads, haps, pairs "
                        "(tab-separated) per pair of neighbouring --variants sites (same -m, --min-alt-reads and "
                        "--min-alt-frac; --variants itself is not needed) that at least one read, or one part of a read "
                        "around the POS <= 0 wrap, observes together: the two 1-based positions, the reads that carry a "
                        "counted symbol at both, the number of distinct symbol pairs, and those pairs as XY:count with X "
                        "and Y from -ACGNT, by count (falling), then by X and Y; independent of -c, -f and -n. "
                        "Not available with more than one process or with S2C_STREAM")
    p.add_argument("--min-link-reads", action="store", dest="min_link_reads", type=int, default=None, metavar="N",
                   help="With --links: list a pair of sites only when at least N reads observe both, default=1")
    p.add_argument("--deletions", action="store_true", dest="deletions", default=False,
                   help="Also write one PREFIX.deletions.tsv in the output folder: one line ref, start, end, len, reads, "
                        "dropped, cov (tab-separated, positions 1-based and inclusive) per distinct gap event the reads "
                        "carry, a maximal run of D, N and P characters inside a read, or inside one of its two parts "
                        "around the POS <= 0 wrap (I, S and H between two of them do not split it, a base does): the "
                        "reads that carry exactly this event, those among them whose gaps the -d rule kept out of the "
                        "counts (0 everywhere when -d is given), and the coverage at start; ordered by reference, "
                        "start and len; independent of -c, -m, -f and -n. "
                        "Not available with more than one process or with S2C_STREAM")
    p.add_argument("--min-del-reads", action="store", dest="min_del_reads", type=int, default=None, metavar="N",
                   help="With --deletions: list an event only when at least N reads carry it, default=1")
    return p


MIN_ALT_READS, MIN_ALT_FRAC = 2, 0.05


def _site_rule(parser, args):
    """(min_alt, min_frac) of the sites --variants lists and --links pairs, or None with neither
    flag; a bad value, or either option with neither flag, is the parser's error (exit status 2)."""
    n, f = args.min_alt_reads, args.min_alt_frac
    if not args.variants and not args.links:
        for opt, v in (("--min-alt-reads", n), ("--min-alt-frac", f)):
            if v is not None:
                parser.error(opt + " needs --variants")
        return None
    n = MIN_ALT_READS if n is None else n
    f = MIN_ALT_FRAC if f is None else f
    if n < 1:
        parser.error("--min-alt-reads must be at least 1")
    if not 0.0 <= f <= 1.0:   # (a NaN too)
        parser.error("--min-alt-frac must be between 0 and 1")
    return n, f


def variants_of(parser, args):
    """(min_alt, min_frac) of --variants or None (the checks: ``_site_rule``)."""
    rule = _site_rule(parser, args)
    return rule if args.variants else None


MIN_LINK_READS = 1


def links_of(parser, args):
    """(min_alt, min_frac, min_reads) of --links or None; --min-link-reads outside [1, 2^32) or
    without --links is the parser's error (exit status 2)."""
    n = args.min_link_reads
    if not args.links:
        if n is not None:
            parser.error("--min-link-reads needs --links")
        return None
    n = MIN_LINK_READS if n is None else n
    if not 1 <= n < 2 ** 32:
        parser.error("--min-link-reads must be at least 1 and below 2^32")
    return _site_rule(parser, args) + (n,)


MIN_INS_READS = 1


def insertions_of(parser, args):
    """min_reads of --insertions or None; --min-ins-reads below 1 or without --insertions is
    the parser's error (exit status 2)."""
    n = args.min_ins_reads
    if not args.insertions:
        if n is not None:
            parser.error("--min-ins-reads needs --insertions")
        return None
    n = MIN_INS_READS if n is None else n
    if not 1 <= n < 2 ** 32:
        parser.error("--min-ins-reads must be at least 1")
    return n


MIN_DEL_READS = 1


def deletions_of(parser, args):
    """min_reads of --deletions or None; --min-del-reads outside [1, 2^32) or without --deletions
    is the parser's error (exit status 2)."""
    n = args.min_del_reads
    if not args.deletions:
        if n is not None:
            parser.error("--min-del-reads needs --deletions")
        return None
    n = MIN_DEL_READS if n is None else n
    if not 1 <= n < 2 ** 32:
        parser.error("--min-del-reads must be at least 1 and below 2^32")
    return n


def tables_of(parser, args):
    """The tables the flags ask for as ``table.request``'s mapping: ``counts``, ``depth`` and
    ``lowcov`` without parameters, the others with what ``variants_of``, ``insertions_of`` and
    ``links_of`` return (their checks, in that order)."""
    return table.request(counts=args.counts, variants=variants_of(parser, args), depth=args.depth, lowcov=args.lowcov,
                         insertions=insertions_of(parser, args), links=links_of(parser, args))


class RunResult:
    def __init__(self, files, timings, info, pending=None):
        self.files = files          # {filename: bytes}
        self.timings = timings      # phase → seconds
        self.info = info            # s2c_batch_info
        self.pending = pending      # the host batch's release, still running (HostBatch.free_async)

    def wait(self):
        """Join the batch's release (the CLI does, after writing its files)."""
        if self.pending is not None:
            self.pending.join()
            self.pending = None
        return self


# the tables whose engine rule begins with the least coverage max(-m, 1) (Workspace.run_with_tables)
LEAST_FIRST = ("variants", "depth", "lowcov", "links")


def consensus_batch(hb, thresholds, prefix, min_depth=1, fill=b"-", nchar=0, device=None, timings=None, deletions=None,
                    **tables):
    """Device pipeline on a parsed HostBatch → {``REF__PREFIX.fasta``: bytes}.  ``tables``: the
    text tables to add, by the keys of ``table.TABLES`` (``table.request`` normalises them) —
    ``counts``, ``depth``, ``lowcov`` = True, ``variants`` = (min_alt, min_frac), ``insertions`` =
    min_reads, ``links`` = (min_alt, min_frac, min_reads); the sites of ``variants`` and ``links``,
    ``depth``'s ``passed`` and ``lowcov``'s cut take the least coverage max(min_depth, 1).  Their
    ``REF__PREFIX<suffix>`` files follow the FASTA entries table by table in ``TABLES`` order, the
    one ``PREFIX.depth_summary.tsv`` of ``depth`` where ``table.SUMMARY_AFTER`` puts it — the run
    then takes the counts route (``Workspace.run_with_tables``).  ``deletions`` = min_reads adds the
    run's one ``PREFIX.deletions.tsv`` (``table.deletions_file``) after every other file; alone it
    takes the counts route too."""
    import torch

    from .engine import _UPLOADERS, DeviceBatch, Workspace, needs_dense_layers, to_host
    from .records import fasta_files

    t = timings if timings is not None else {}
    t0 = time.perf_counter()
    req = table.request(**tables)
    dels = None if deletions is None or deletions is False else (MIN_DEL_READS if deletions is True else int(deletions))
    route = bool(req) or dels is not None   # (the counts route: every tile's counts kept for the tables)
    db = DeviceBatch(hb, device, dense_layers=needs_dense_layers(fill, route))
    t1 = time.perf_counter()
    ws = Workspace(db, thresholds, min_depth, fill, keep_counts=route)
    torch.cuda.synchronize(db.device)
    t["h2d"] = time.perf_counter() - t0
    t["h2d_issue"] = t1 - t0   # (layers + pinned staging + copies issued; the rest: workspace + drain)
    up = _UPLOADERS.get(db.device)
    if up is not None:   # (the pinned ring's cumulative host seconds: alloc, wait, pack, issue)
        t.update(("h2d_up_" + k, v) for k, v in up.timing.items())
    t0 = time.perf_counter()
    res = {}
    if route:
        least = (max(int(min_depth), 1),)
        res = ws.run_with_tables({k: (least if k in LEAST_FIRST else ()) + v for k, v in req.items()}, deletions=dels)
    else:
        ws.run()
    torch.cuda.synchronize(db.device)
    t1 = time.perf_counter()
    stats, offs, out = ws.fetch()
    t["device"] = time.perf_counter() - t0
    t["device_run"] = t1 - t0   # (the launches to completion; the rest: the results' D2H)
    t0 = time.perf_counter()
    files = fasta_files(hb, thresholds, prefix, nchar, stats, offs, out)
    for tab in table.TABLES:   # (after the records: a vote error raises and no file is returned)
        if tab.key in res:
            files.update(table.table_files(hb, prefix, res[tab.key][0], to_host(res[tab.key][1]), tab.header, tab.suffix))
        if tab.key == table.SUMMARY_AFTER and "depth" in res:
            # (the summary: the host sums the tiles' statistics; it never reads the counts)
            files.update(table.summary_file(hb, prefix, res["depth"][2]))
    if table.DEL_KEY in res:   # (the run's one deletion table: last)
        files.update(table.deletions_file(hb, prefix, res[table.DEL_KEY][0], to_host(res[table.DEL_KEY][1])))
    t["format"] = time.perf_counter() - t0
    return files


PROGRESS_EVERY = 500000   # :224


def progress_lines(header_lines, lines_total):
    """The reference's progress lines (:182, :194, :224-225): its counter starts at
    -header_length, is incremented for every line of the data pass (header lines
    included) and a line is printed whenever it is a multiple of 500000 — "0 reads
    processed." right after a non-empty header, negative multiples for headers longer
    than 500000 lines."""
    lo, hi = 1 - header_lines, lines_total - header_lines   # counter values after each increment
    first = -((-lo) // PROGRESS_EVERY) * PROGRESS_EVERY      # smallest multiple >= lo
    return [str(v) + " reads processed." for v in range(first, hi + 1, PROGRESS_EVERY)]


def _log_summary(log, info):
    log("SAM header processed, " + str(info.n_refs) + " references found.\n")
    for line in progress_lines(info.header_lines, info.lines_total):
        log(line)
    log("A total of " + str(info.lines_total - info.header_lines) + " reads were processed, out of which, " +
        str(info.reads_mapped) + " reads were mapped.\n")


REF_ERRORS = (KeyError, IndexError, ValueError, ZeroDivisionError, OverflowError)


class _Partial:
    """_log_summary's fields from the parser's counters (a run that failed after the read pass)."""

    def __init__(self, n_refs, counters):
        self.n_refs = n_refs
        self.header_lines, self.lines_total, self.reads_mapped = counters[0], counters[1], counters[2]


def _log_failed_parse(log, parser):
    """What the reference has printed when the read pass or its insertion checks raise: its
    header line once the header is read (:182), the progress lines of the lines before the
    failing one (:224-225); after a clean read pass (an insertion check failed, :284-294) the
    whole summary (:227)."""
    ended, n_refs, header_lines, lines, err = parser.progress()
    if not err:
        _log_summary(log, _Partial(n_refs, parser.counters()))
        return
    if not ended:
        return   # (the header pass raised: nothing after "Processing file")
    log("SAM header processed, " + str(n_refs) + " references found.\n")
    for line in progress_lines(header_lines, lines - 1):
        log(line)


def _warm_session(sess, reserve, timing):
    """Bring up the HIP runtime and the device on a side thread (the first device call costs
    tenths of a second) so it overlaps the host parse, and reserve the batch's device buffer
    and pinned staging (``reserve`` bytes: a large input's estimate) there too; join() before
    the upload.  A failure is raised on the main thread by ``_join_session``."""
    import threading

    def run():
        try:
            sess.reserve(reserve)
        except Exception as e:  # noqa: BLE001 - re-raised by _join_session on the main thread
            sess.error = e
        timing.update(sess.timing)
    sess.error = None
    th = threading.Thread(target=run, daemon=True)
    th.start()
    return th


def _join_session(sess, th):
    th.join()
    if sess.error is not None:
        raise sess.error


def upload_estimate(filename):
    """A device block that holds the packed batch of a large input (0 below 64 MB of input):
    the batch is ≈ 0.42 of a plain SAM file's bytes on C5 (short reads, qualities dropped,
    bases in 2-bit planes) — 0.6 × the file (2.4 × a gzip file) leaves room for longer CIGARs."""
    try:
        size = os.path.getsize(filename)
    except OSError:
        return 0   # (the parser reports the reference's error for a missing file)
    if size < (64 << 20):
        return 0
    return int(size * (2.4 if filename.endswith(".gz") else 0.6))


def consensus_batch_hip(sess, hb, thresholds, prefix, min_depth=1, fill=b"-", nchar=0, timings=None):
    """consensus_batch through hiprun.Session (no PyTorch): the one-process CLI's device side."""
    from .records import fasta_files

    t = timings if timings is not None else {}
    t0 = time.perf_counter()
    stats, offs, out = sess.run(hb, thresholds, min_depth, fill, t)
    t["device"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    files = fasta_files(hb, thresholds, prefix, nchar, stats, offs, out)
    t["format"] = time.perf_counter() - t0
    return files


def _parse_file(filename, maxdel_active, log, timings, t0):
    """The read pass over one file → its HostBatch; ``timings["parse"]``: the seconds since ``t0``,
    the run's start.  A reference error is logged as the reference would have (``_log_failed_parse``)
    and raised; the summary of a clean pass is the caller's to log."""
    from .batch import Parser

    p = Parser(maxdel_active, 150)
    try:
        p.feed_file(filename)
        hb = p.finish()
    except REF_ERRORS:
        if log:
            _log_failed_parse(log, p)
        raise
    finally:
        p.close()
    timings["parse"] = time.perf_counter() - t0
    return hb


def _consensus_files_tables(filename, thresholds, prefix, min_depth, fill, nchar, maxdel_active, device, log, req,
                            deletions=None):
    """consensus_files with the tables of ``req`` (table.request) and the deletion table: the
    torch engine path (consensus_batch)."""
    from . import _lib
    from .engine import _dev

    t = {}
    t0 = time.perf_counter()
    dev = _dev(device)
    _lib.plan_for_device(dev)   # (the plan's grid shaping, before the parse builds it)
    hb = _parse_file(filename, maxdel_active, log, t, t0)
    if log:
        _log_summary(log, hb.info)
    files = consensus_batch(hb, thresholds, prefix, min_depth, fill, nchar, dev, t, deletions=deletions, **req)
    return RunResult(files, t, hb.info, hb.free_async())


def consensus_files(filename, thresholds, prefix, min_depth=1, fill=b"-", nchar=0, maxdel_active=True,
                    device=None, log=None, deletions=None, **tables):
    """Run the whole pipeline on one SAM/SAM.gz file; returns a RunResult whose
    ``files`` maps ``REF__PREFIX.fasta`` → content bytes (nothing written).  The device side
    runs through the HIP runtime directly (hiprun.py): this path never imports PyTorch.
    With any of ``consensus_batch``'s ``tables`` the files also hold those tables, and the run
    goes through the torch engine path instead (``consensus_batch``); so it does with
    ``deletions`` = min_reads, which adds the run's ``PREFIX.deletions.tsv``."""
    req = table.request(**tables)
    if req or (deletions is not None and deletions is not False):
        return _consensus_files_tables(filename, thresholds, prefix, min_depth, fill, nchar, maxdel_active, device, log, req,
                                       deletions)
    from .hiprun import Session, device_index

    t = {}
    t0 = time.perf_counter()
    sess = Session(device_index(device))
    warm = _warm_session(sess, upload_estimate(filename), t)   # (the device comes up while the host parses)
    try:
        hb = _parse_file(filename, maxdel_active, log, t, t0)
        _join_session(sess, warm)
        if log:
            _log_summary(log, hb.info)
        files = consensus_batch_hip(sess, hb, thresholds, prefix, min_depth, fill, nchar, t)
    finally:
        warm.join()
        sess.close()
    # the batch's host arrays (GBs for a large input: ~60 ms of munmap on the box) released
    # beside the caller's file writes
    return RunResult(files, t, hb.info, hb.free_async())


def run_text(sam_text, argv, device=None, deletions=None, **tables):
    """Library entry for tests: SAM text + CLI args (without -i) → (status, {fname: str}).
    status is "ok" or the reference's exception class name; nothing touches the disk.
    ``tables``: ``consensus_batch``'s; a table given among the args (``--variants`` and its
    options, ...) is added, and wins over its keyword; so do ``deletions`` = min_reads and
    ``--deletions`` / ``--min-del-reads``."""
    from .batch import parse_text

    parser = build_parser()
    args = parser.parse_args(["-i", "in.sam"] + list(argv))
    req = {**table.request(**tables), **tables_of(parser, args)}
    dels = deletions_of(parser, args)
    dels = deletions if dels is None else dels
    try:
        thresholds = [float(i) for i in args.thresholds.split(",")]
        prefix = args.prefix or "in"
        hb = parse_text(sam_text, not isinstance(args.maxdel, str), 150)
        files = consensus_batch(hb, thresholds, os.fsencode(prefix), args.min_depth,
                                os.fsencode(args.fill), args.n, device, deletions=dels, **req)
    except REF_ERRORS as e:
        return type(e).__name__, {}
    return "ok", {k.decode("latin-1"): v.decode("latin-1") for k, v in files.items()}


def _dist_env():
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), \
        int(os.environ.get("LOCAL_RANK", "0"))


class _Counters:
    """The summary counters of the distributed read pass (``_log_summary``'s fields)."""

    def __init__(self, n_refs, parsed):
        self.n_refs = n_refs
        self.header_lines, self.lines_total, self.reads_mapped = \
            parsed.header_lines, parsed.lines_total, parsed.reads_mapped


def consensus_files_sharded(filename, thresholds, prefix, min_depth, fill, nchar, maxdel_active, log=None):
    """One process per GPU (torchrun): the file is parsed once across the ranks and each
    rank receives the reads of its tile range (sam2consensus_amd.dparse), runs it, the
    stats are all-reduced and the FASTA bodies gathered over the process group (RCCL; the
    gloo backend with S2C_DIST_BACKEND=gloo); rank 0 returns the files, other ranks None."""
    import torch
    import torch.distributed as dist

    from .dparse import parse_distributed
    from .engine import DeviceBatch, Workspace, needs_dense_layers
    from .records import fasta_files
    from .shard import gather_device

    world, rank, local = _dist_env()
    backend = os.environ.get("S2C_DIST_BACKEND", "nccl")
    ndev = max(torch.cuda.device_count(), 1)
    if local >= ndev:
        if backend != "gloo":   # RCCL: one device per rank
            raise RuntimeError("LOCAL_RANK %d but %d GPU(s) visible: launch one process per GPU "
                               "(S2C_DIST_BACKEND=gloo lets ranks share a device)" % (local, ndev))
        local %= ndev   # (ranks sharing a device: gloo tests on one GPU)
    torch.cuda.set_device(local)
    from . import _lib
    _lib.plan_for_device(torch.device("cuda", local))
    owned = not dist.is_initialized()   # (this call's process group: destroyed on the way out)
    if owned:
        dist.init_process_group(backend, device_id=torch.device("cuda", local) if backend == "nccl" else None)
    try:
        P = parse_distributed(filename, rank, world, maxdel_active)
        if log and rank == 0:
            _log_summary(log, _Counters(P.hb.info.n_refs, P))
        ws = Workspace(DeviceBatch(P.sub, "cuda:%d" % local, dense_layers=needs_dense_layers(fill)), thresholds,
                       min_depth, fill)
        ws.run()
        res = gather_device(ws, P.sub, rank, world, len(thresholds))
    finally:
        if owned and dist.is_initialized():
            dist.destroy_process_group()
    if rank != 0:
        return None
    P.hb.ref_reads = P.ref_flags   # Σcoverage > 0 over every rank's reads (:334-341)
    return fasta_files(P.hb, thresholds, prefix, nchar, *res)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    req = tables_of(parser, args)
    dels = deletions_of(parser, args)
    for key in list(req) + ([table.DEL_KEY] if dels is not None else []):   # (refused before a folder is made or a device touched)
        if _dist_env()[0] > 1:
            parser.error("--" + key + " is not available with more than one process (WORLD_SIZE > 1)")
        if os.environ.get("S2C_STREAM"):
            parser.error("--" + key + " is not available with streamed batches (S2C_STREAM)")
    filename = args.filename
    thresholds = [float(i) for i in args.thresholds.split(",")]                # :117-118
    if args.prefix == "":
        prefix = "".join(args.filename.split("/")[-1]).split(".")[0]            # :121-122
    else:
        prefix = args.prefix
    outfolder = args.outfolder.rstrip("/")                                       # :127-130
    world, rank, _ = _dist_env()
    if rank == 0 and not os.path.exists(outfolder):   # (one process creates it: rank 0 writes the files)
        os.makedirs(outfolder)
    outfolder += "/"
    maxdel_active = not isinstance(args.maxdel, str)
    res = None
    if rank == 0:
        print("\nProcessing file " + filename + ":\n")
    if world > 1:
        files = consensus_files_sharded(filename, thresholds, os.fsencode(prefix), args.min_depth,
                                        os.fsencode(args.fill), args.n, maxdel_active, log=print)
        if files is None:
            return 0
    else:
        from .stream import consensus_files_streamed, stream_bytes_from_env
        sb = stream_bytes_from_env()
        if sb > 0:   # coordinate-sorted input in bounded host memory (stream.py)
            files = consensus_files_streamed(filename, thresholds, os.fsencode(prefix), args.min_depth,
                                             os.fsencode(args.fill), args.n, maxdel_active, log=print,
                                             batch_bytes=sb).files
        else:
            res = consensus_files(filename, thresholds, os.fsencode(prefix), args.min_depth,
                                  os.fsencode(args.fill), args.n, maxdel_active, log=lambda s: print(s), deletions=dels, **req)
            files = res.files
    tables, last = [], None
    for fname, body in files.items():                                             # :411-424
        path = os.fsencode(outfolder) + fname
        with open(path, "wb") as fh:
            fh.write(body)
        shown = os.fsdecode(path)
        noun = next((t.noun for t in table.TABLES if t.key in req and fname.endswith(t.suffix)), None)
        if dels is not None and fname == os.fsencode(prefix) + table.DEL_SUFFIX:   # (PREFIX alone; the files' last)
            last = "Deletion table saved in: " + shown
        elif "depth" in req and fname.endswith(table.SUMMARY_SUFFIX):   # (PREFIX alone: no reference)
            tables.append("Depth summary saved in: " + shown)
        elif noun is not None:   # (the tables' lines after the consensus lines, in the files' order)
            tables.append(noun + " saved for " + os.fsdecode(fname[: fname.rfind(b"__")]) + " in: " + shown)
        elif len(thresholds) == 1:
            print("Consensus sequence at " + str(int(thresholds[0] * 100)) + "% saved for " +
                  os.fsdecode(fname[: fname.rfind(b"__")]) + " in: " + shown)
        else:
            print("Consensus sequences at " + ",".join([str(int(i * 100)) + "%" for i in thresholds]) +
                  " saved for " + os.fsdecode(fname[: fname.rfind(b"__")]) + " in: " + shown)
    for line in tables + ([last] if last is not None else []):
        print(line)
    if res is not None:
        res.wait()
    print("Done.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
