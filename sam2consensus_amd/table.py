"""Per-position count tables (``--counts``): ``REF__PREFIX.counts.tsv`` beside each FASTA file.

One line per reference position, covered or not: the 1-based position, the coverage (the sum
of the six counts, sam2consensus.py:237) and the counts of ``sequences[ref][pos]`` (:210-218)
in ``-ACGNT`` order, tab-separated plain decimal.  Insertion columns (:262-311) are not part
of the table.  The device formats the text (csrc/s2c_table.hip, ``Workspace.counts_table``);
``format_rows`` is the same format in plain Python — the tests' model, and enough for small
inputs on the host.

Tables of mixed sites (``--variants``): ``REF__PREFIX.variants.tsv``, the count table's lines of
the positions where a minority is present, each with three more fields.  With ``cov`` the sum
of the six counts, ``rank(s) = #{s' : c[s'] > c[s] or (c[s'] == c[s] and s' < s)}``, ``major``
the symbol of rank 0 (ties: the earlier symbol in ``-ACGNT``) and ``alt = cov - c[major]``, a
position is a site iff ``cov >= min_cov``, ``alt >= min_alt`` and ``float(alt) >= min_frac *
float(cov)`` (one fp64 product and compare).  Its line ends ``\tM\tALT\t0.dddd``: the major
symbol, the other symbols with a non-zero count in rank order, ``dddd = alt * 10000 // cov``.
All six symbols take part, ``-`` and ``N`` included, as in the vote; insertion columns do not.
The device selects and formats (csrc/s2c_sites.hip, ``Workspace.sites_table``); ``site_mask``
and ``format_sites`` are the model.

Depth intervals (``--depth``): ``REF__PREFIX.depth.tsv``, one line ``start\tend\tcov`` per
maximal run of equal coverage (the sum of the six counts), zero-coverage runs included,
positions 1-based and inclusive: the runs partition [1, LN].  One ``PREFIX.depth_summary.tsv``
per run of the program holds a line per reference: its length, the positions with coverage
>= 1 and >= max(-m, 1), the sum, least and largest coverage and the number of runs.  The
low-coverage mask (``--lowcov``): ``REF__PREFIX.lowcov.tsv``, one line ``start\tend`` per
maximal run of positions with coverage < max(-m, 1) — where the vote wrote the fill character
(sam2consensus.py:358).  The device finds and formats the runs (csrc/s2c_runs.hip,
``Workspace.depth_table``); ``depth_runs``, ``format_depth``, ``format_lowcov`` and
``depth_stats`` are the model.

Insertion motif tables (``--insertions``): ``REF__PREFIX.insertions.tsv``, one line ``pos\tcov\t
reads\tlen\tmotif`` per distinct (position, motif) among the insertion events the consensus is
voted from (:73-75, :221, :262-271): ``pos`` the 1-based position whose consensus letter the
inserted columns follow (:371-372), ``cov`` the coverage there (:294; it can be 0 or below
``reads``: a read whose CIGAR ends in ``I`` does not cover its own key), ``reads`` the reads
carrying exactly this motif, its length and its characters from ``-ACGNT``.  Lines are ordered
by ``pos``, then ``reads`` falling, ``len`` rising, then the motif symbol by symbol in
``-ACGNT`` order.  The device groups, orders and formats (csrc/s2c_ins.hip,
``Workspace.insertions_table``); ``format_insertions`` is the model.

Link tables (``--links``): ``REF__PREFIX.links.tsv``, one line ``pos1\tpos2\treads\thaps\tpairs``
per pair of neighbouring mixed sites that at least one read fragment observes together.  The
sites are the positions ``--variants`` lists under the same ``-m``, ``--min-alt-reads`` and
``--min-alt-frac``.  A fragment is a read, or each of the two parts of a read around the
``POS <= 0`` wrap (:212's negative index).  It observes symbol ``s`` at position ``p`` iff it
adds one to ``counts[s][p]`` (:210-218): a ``-`` of a read over ``-d`` is no observation, ``N``
is a symbol like the others, and the observations of all fragments sum to the count table.  For
sites ``p1 < p2`` of one reference with no site between them ``n[s1][s2]`` is the number of
fragments that observe ``s1`` at ``p1`` and ``s2`` at ``p2``; a fragment that passes a site
without observing it (its ``-`` dropped) links nothing across it.  ``reads`` = Σ n, ``haps`` the
number of non-zero ``n[s1][s2]``, ``pairs`` those entries as ``XY:count`` joined by ``,``, by
count falling, then by ``(s1, s2)`` in ``-ACGNT`` order — a total order.  A pair is listed iff
``reads >= --min-link-reads`` (>= 1).  The device walks the reads and formats (csrc/s2c_links.hip,
``Workspace.links_table``); ``link_pairs`` and ``format_links`` are the model.

The deletion table (``--deletions``): one ``PREFIX.deletions.tsv`` per run of the program, like
the depth summary, one line ``ref\tstart\tend\tlen\treads\tdropped\tcov`` per distinct gap event.
A gap character is a character of parsecigar's ``seqout`` that a ``D``, ``N`` or ``P`` token
produced (:70-72; a ``-`` of SEQ is a base).  A read is dropped when the ``-d`` rule is active and
``seqout.count("-") > 150`` (:210): its ``-`` are not counted.  A read's span runs from its first
counted character to its last; a fragment is the span, or each of its two parts around the
``POS <= 0`` wrap.  An event is a maximal run of consecutive gap characters inside one fragment
— ``I``, ``S``, ``H`` and an ``M`` after SEQ ran out do not split it, a base does — keyed by
(reference, start, len), 1-based and inclusive; ``reads`` the fragments that carry exactly it,
``dropped`` those among them of dropped reads, ``cov`` the sum of the six counts at ``start``.
Listed iff ``reads >= --min-del-reads``; ordered by reference in header order, ``start``, ``len``.
The device walks, merges and formats (csrc/s2c_dels.hip, ``Workspace.deletions_table``);
``gap_events`` and ``format_deletions`` are the model.
"""
from __future__ import annotations

import collections

import numpy as np

HEADER = b"pos\tcov\t-\tA\tC\tG\tN\tT\n"
SUFFIX = b".counts.tsv"
SITES_HEADER = b"pos\tcov\t-\tA\tC\tG\tN\tT\tmajor\talt\taf\n"
SITES_SUFFIX = b".variants.tsv"
SYMBOLS = "-ACGNT"
DEPTH_HEADER = b"start\tend\tcov\n"
DEPTH_SUFFIX = b".depth.tsv"
LOWCOV_HEADER = b"start\tend\n"
LOWCOV_SUFFIX = b".lowcov.tsv"
SUMMARY_HEADER = b"ref\tlen\tcovered\tpassed\tsumcov\tmincov\tmaxcov\truns\n"
SUMMARY_SUFFIX = b".depth_summary.tsv"
EMPTY_STATS = (0, 0, 0, 0, 2 ** 63 - 1, -1)   # a block without a run start (s2c_runs_len)
INS_HEADER = b"pos\tcov\treads\tlen\tmotif\n"
INS_SUFFIX = b".insertions.tsv"
LINKS_HEADER = b"pos1\tpos2\treads\thaps\tpairs\n"
LINKS_SUFFIX = b".links.tsv"

# Every per-reference table, in file order and launch order; the command-line flag is "--" + key,
# the stdout line "<noun> saved for REF in: PATH".  The one file that is no per-reference table,
# the depth summary (with ``depth``), comes after the tables of SUMMARY_AFTER.
Table = collections.namedtuple("Table", "key suffix header noun")
TABLES = (Table("counts", SUFFIX, HEADER, "Count table"),
          Table("variants", SITES_SUFFIX, SITES_HEADER, "Variant table"),
          Table("depth", DEPTH_SUFFIX, DEPTH_HEADER, "Depth table"),
          Table("lowcov", LOWCOV_SUFFIX, LOWCOV_HEADER, "Low-coverage table"),
          Table("insertions", INS_SUFFIX, INS_HEADER, "Insertion table"),
          Table("links", LINKS_SUFFIX, LINKS_HEADER, "Link table"))
SUMMARY_AFTER = "lowcov"
# The second file that is no per-reference table: the deletion table of a run, after every file
# above (the flag --deletions, the stdout line "Deletion table saved in: PATH").
DEL_HEADER = b"ref\tstart\tend\tlen\treads\tdropped\tcov\n"
DEL_SUFFIX = b".deletions.tsv"
DEL_KEY = "deletions"


def request(**kw):
    """The tables asked for by keyword as one mapping {key: parameter tuple} in ``TABLES`` order:
    ``True`` gives ``()``, ``False`` / ``None`` leaves the table out, a bare number (``insertions``'
    min_reads) gives a 1-tuple, a sequence its tuple.  A keyword that names no table is a
    ``TypeError``."""
    unknown = sorted(set(kw) - {t.key for t in TABLES})
    if unknown:
        raise TypeError("no such table: " + ", ".join(unknown))
    asked = ((t.key, kw.get(t.key)) for t in TABLES)
    return {k: () if v is True else tuple(v) if isinstance(v, (tuple, list)) else (v,)
            for k, v in asked if v is not None and v is not False}


def format_rows(counts_6xL, p0=1):
    """The table rows (no header) of counts[6][L], position ``p0`` printed for column 0."""
    c = np.asarray(counts_6xL)
    if c.ndim != 2 or c.shape[0] != 6:
        raise ValueError("counts must be [6][L]")
    rows = np.empty((c.shape[1], 8), dtype=object)   # (Python ints: the coverage may pass 2^32)
    rows[:, 2:] = c.T.astype(object)
    rows[:, 1] = rows[:, 2:].sum(axis=1) if c.shape[1] else 0
    rows[:, 0] = np.arange(int(p0), int(p0) + c.shape[1], dtype=object)
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % tuple(r) for r in rows.tolist()).encode("ascii")


def _c6(counts_6xL):
    c = np.asarray(counts_6xL)
    if c.ndim != 2 or c.shape[0] != 6:
        raise ValueError("counts must be [6][L]")
    return c


def site_mask(counts_6xL, min_cov=1, min_alt=2, min_frac=0.05):
    """bool[L]: the positions of counts[6][L] that are sites.  Integers in int64 (cov < 2^35),
    the last test in float64 as the device's: both operands below 2^53, so the conversions are
    exact and the one product rounds as Python's ``min_frac * float(cov)`` does."""
    c = _c6(counts_6xL).astype(np.int64)
    cov = c.sum(axis=0)
    alt = cov - (c.max(axis=0) if c.shape[1] else cov)
    return (cov >= int(min_cov)) & (alt >= int(min_alt)) & (alt.astype(np.float64) >= np.float64(min_frac) * cov.astype(np.float64))


def format_sites(counts_6xL, p0=1, min_cov=1, min_alt=2, min_frac=0.05):
    """The site lines (no header) of counts[6][L], position ``p0`` printed for column 0."""
    c = _c6(counts_6xL)
    out = []
    for j in np.flatnonzero(site_mask(c, min_cov, min_alt, min_frac)).tolist():
        n = [int(v) for v in c[:, j]]
        cov = sum(n)
        order = sorted(range(6), key=lambda s: (-n[s], s))   # by rank
        alt = cov - n[order[0]]
        out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t0.%04d\n" % (
            int(p0) + j, cov, n[0], n[1], n[2], n[3], n[4], n[5], SYMBOLS[order[0]],
            "".join(SYMBOLS[s] for s in order[1:] if n[s]), alt * 10000 // cov))
    return "".join(out).encode("ascii")


def format_insertions(entries, cov, p0=1, min_reads=1):
    """The insertion lines (no header) of ``entries``: (pos, motif, reads) with ``pos`` the
    0-based index into ``cov`` (the coverage per position), ``motif`` a non-empty string over
    ``-ACGNT`` and ``reads`` >= 1, each (pos, motif) once; position ``p0`` is printed for index
    0.  Entries with ``reads < min_reads`` are left out.  The order: ``pos`` rising, ``reads``
    falling, ``len`` rising, the motif symbol by symbol in ``-ACGNT`` order."""
    rows = []
    for pos, motif, reads in entries:
        motif = motif.decode("ascii") if isinstance(motif, (bytes, bytearray)) else str(motif)
        if not motif or any(ch not in SYMBOLS for ch in motif):
            raise ValueError("a motif is a non-empty string over -ACGNT")
        if int(reads) >= int(min_reads):
            rows.append((int(pos), -int(reads), len(motif), [SYMBOLS.index(ch) for ch in motif], motif))
    rows.sort(key=lambda r: r[:4])
    return "".join("%d\t%d\t%d\t%d\t%s\n" % (int(p0) + pos, int(cov[pos]), -nr, n, motif)
                   for pos, nr, n, _, motif in rows).encode("ascii")


def link_pairs(fragments, site_positions):
    """{k: n[6][6]} of the pairs (site k, site k + 1) that a fragment observes together.
    ``fragments``: one list per fragment of its observations ``(pos, sym)`` in rising position,
    ``sym`` an index into ``-ACGNT`` or the character; ``site_positions``: the sites of the
    fragments' reference, rising.  Only an observation at site k followed, as the fragment's
    next observation at a site, by one at site k + 1 counts."""
    rank = {int(p): k for k, p in enumerate(site_positions)}
    pairs = {}
    for obs in fragments:
        prev = None
        for pos, sym in obs:
            k = rank.get(int(pos))
            if k is None:
                continue
            s = SYMBOLS.index(sym) if isinstance(sym, str) else int(sym)
            if prev is not None and prev[0] + 1 == k:
                pairs.setdefault(prev[0], [[0] * 6 for _ in range(6)])[prev[1]][s] += 1
            prev = (k, s)
    return pairs


def format_links(pairs, site_positions, p0=1, min_reads=1):
    """The link lines (no header) of ``pairs`` = {k: n[6][6]} over the sites ``site_positions``
    (0-based, rising; position ``p0`` is printed for index 0): the pairs with ``reads >=
    min_reads`` (>= 1) in site order."""
    if int(min_reads) < 1:
        raise ValueError("min_reads must be at least 1")
    out = []
    for k in sorted(pairs):
        e = [(int(pairs[k][a][b]), a, b) for a in range(6) for b in range(6) if int(pairs[k][a][b])]
        reads = sum(n for n, _, _ in e)
        if reads < int(min_reads):
            continue
        e.sort(key=lambda x: (-x[0], x[1], x[2]))
        out.append("%d\t%d\t%d\t%d\t%s\n" % (int(p0) + int(site_positions[k]), int(p0) + int(site_positions[k + 1]), reads, len(e),
                                             ",".join("%s%s:%d" % (SYMBOLS[a], SYMBOLS[b], n) for n, a, b in e)))
    return "".join(out).encode("ascii")


def gap_events(fragments):
    """{(start, len): [reads, dropped]} of one reference's fragments.  ``fragments``: one pair
    ``(chars, dropped)`` per fragment — ``chars`` its characters in seqout order as ``(pos, gap)``,
    ``pos`` the 0-based position the character lands on and ``gap`` whether a D, N or P token
    produced it; ``dropped`` whether the read's ``-`` are kept out of the counts.  An event is a
    maximal run of gap characters next to each other in ``chars``."""
    events = {}
    for chars, dropped in fragments:
        run = None   # [start, len]
        for pos, gap in list(chars) + [(None, False)]:
            if gap and run is not None:
                run[1] += 1
            elif gap:
                run = [int(pos), 1]
            elif run is not None:
                e = events.setdefault((run[0], run[1]), [0, 0])
                e[0] += 1
                e[1] += 1 if dropped else 0
                run = None
    return events


def format_deletions(events, cov, min_reads=1):
    """The deletion lines (no header) of ``events`` = {ref name: ``gap_events``' mapping} with
    ``cov`` = {ref name: the coverage per position}; the references in the mapping's order (the
    header's), a reference's events by ``start``, then ``len``; those with ``reads < min_reads``
    (>= 1) are left out."""
    if int(min_reads) < 1:
        raise ValueError("min_reads must be at least 1")
    out = []
    for ref, ev in events.items():
        name = ref.decode("latin-1") if isinstance(ref, (bytes, bytearray)) else str(ref)
        for (start, ln), (reads, dropped) in sorted(ev.items()):
            if int(reads) >= int(min_reads):
                out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, start + 1, start + ln, ln, reads, dropped, int(cov[ref][start])))
    return "".join(out).encode("latin-1")


def deletions_file(hb, prefix, offs, body):
    """{``PREFIX.deletions.tsv``: bytes} from ``Workspace.deletions_table``'s text on the host:
    the header and the tiles' lines as they lie (tiles are emitted reference by reference, so the
    text is in file order; ``offs`` is not needed to cut it)."""
    pre = prefix.encode("latin-1") if isinstance(prefix, str) else prefix
    end = int(offs[-1]) if len(offs) else 0
    return {pre + DEL_SUFFIX: DEL_HEADER + bytes(body[:end])}


def table_files(hb, prefix, offs, body, header=HEADER, suffix=SUFFIX):
    """{``REF__PREFIX.counts.tsv``: bytes} from ``Workspace.counts_table``'s text on the host
    (with ``SITES_HEADER`` and ``SITES_SUFFIX``: the ``.variants.tsv`` files from
    ``Workspace.sites_table``'s; a reference without a site gets the header alone):
    ``offs[k]`` the byte offset of tile k's rows in ``body`` (n_tiles + 1 entries; tiles are
    emitted reference by reference).  One table per reference with Σcoverage > 0 (the
    reference's own pruning rule, :334-341 — not the FASTA records' keep rule)."""
    pre = prefix.encode("latin-1") if isinstance(prefix, str) else prefix
    files = {}
    for r in range(hb.info.n_refs):
        if hb.ref_reads[r] == 0:
            continue
        f0, n = int(hb.ref_first_block[r]), int(hb.ref_nblocks[r])
        a, b = int(offs[f0]), int(offs[f0 + n])
        files[hb.names[r].encode("latin-1") + b"__" + pre + suffix] = header + body[a:b]
    return files


def coverage(counts_6xL):
    """The coverage of every position of counts[6][L] as Python ints (it may pass 2^32)."""
    c = _c6(counts_6xL)
    return c.astype(np.int64).sum(axis=0).tolist() if c.shape[1] else []


def depth_runs(cov):
    """The maximal runs of equal value in ``cov``: (start, end, value) triples, ``start`` the
    0-based first index and ``end`` the index after the last; they partition [0, len(cov))."""
    runs, start = [], 0
    for j in range(1, len(cov) + 1):
        if j == len(cov) or cov[j] != cov[start]:
            runs.append((start, j, cov[start]))
            start = j
    return runs


def format_depth(counts_6xL, p0=1):
    """The depth lines (no header) of counts[6][L], position ``p0`` printed for column 0."""
    return "".join("%d\t%d\t%d\n" % (int(p0) + s, int(p0) + e - 1, v)
                   for s, e, v in depth_runs(coverage(counts_6xL))).encode("ascii")


def format_lowcov(counts_6xL, p0=1, min_cov=1):
    """The low-coverage lines (no header) of counts[6][L]: the runs of coverage < ``min_cov``."""
    low = [v < int(min_cov) for v in coverage(counts_6xL)]
    return "".join("%d\t%d\n" % (int(p0) + s, int(p0) + e - 1) for s, e, v in depth_runs(low) if v).encode("ascii")


def depth_stats(counts_6xL, min_cov):
    """(runs, covered, passed, sumcov, mincov, maxcov) of counts[6][L], as s2c_runs_len's
    stats: the depth lines, the positions with coverage >= 1 and >= ``min_cov``, the sum, least
    and largest coverage; ``EMPTY_STATS`` for L = 0."""
    cov = coverage(counts_6xL)
    if not cov:
        return EMPTY_STATS
    return (len(depth_runs(cov)), sum(v >= 1 for v in cov), sum(v >= int(min_cov) for v in cov), sum(cov),
            min(cov), max(cov))


def summary_file(hb, prefix, stats):
    """{``PREFIX.depth_summary.tsv``: bytes} from ``Workspace.depth_table``'s per-tile
    ``stats[n_tiles][6]``: one line per reference with a depth table (``table_files``' rule),
    in reference order, its tiles' statistics summed (the least and largest coverage: the
    least and largest)."""
    pre = prefix.encode("latin-1") if isinstance(prefix, str) else prefix
    lines = [SUMMARY_HEADER]
    for r in range(hb.info.n_refs):
        if hb.ref_reads[r] == 0:
            continue
        f0, n = int(hb.ref_first_block[r]), int(hb.ref_nblocks[r])
        st = [[int(v) for v in row] for row in stats[f0:f0 + n]] or [list(EMPTY_STATS)]
        runs, covered, passed, sumcov = (sum(row[k] for row in st) for k in range(4))
        fields = (int(hb.ref_len[r]), covered, passed, sumcov, min(row[4] for row in st), max(row[5] for row in st), runs)
        lines.append(hb.names[r].encode("latin-1") + b"\t" + "\t".join(str(v) for v in fields).encode("ascii") + b"\n")
    return {pre + SUMMARY_SUFFIX: b"".join(lines)}
