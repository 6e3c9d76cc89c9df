"""Per-position count tables (``--counts``): ``REF__PREFIX.counts.tsv`` beside each FASTA file.

One line per reference position, covered or not: the 1-based position, the coverage (the sum
of the six counts, sam2consensus.py:237) and the counts of ``sequences[ref][pos]`` (:210-218)
in ``-ACGNT`` order, tab-separated plain decimal.  Insertion columns (:262-311) are not part
of the table.  The device formats the text (csrc/s2c_table.hip, ``Workspace.counts_table``);
``format_rows`` is the same format in plain Python — the tests' model, and enough for small
inputs on the host.
"""
from __future__ import annotations

import numpy as np

HEADER = b"pos\tcov\t-\tA\tC\tG\tN\tT\n"
SUFFIX = b".counts.tsv"


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


def table_files(hb, prefix, offs, body):
    """{``REF__PREFIX.counts.tsv``: bytes} from ``Workspace.counts_table``'s text on the host:
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
        files[hb.names[r].encode("latin-1") + b"__" + pre + SUFFIX] = HEADER + body[a:b]
    return files
