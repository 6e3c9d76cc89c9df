"""The deletion table's device cost on C2, C4 or C5: the six kernels of s2c_dels.hip on a resident
batch — the two walks of every piece (s2c_dels_count; s2c_dels_collect with the zeroing of its
table), the bucketing (s2c_dels_tiles, the prefix sum, s2c_dels_scatter), s2c_dels_len and
s2c_dels_write — next to two yardsticks in the same process that read the same pieces:
s2c_links_count against the default site rule's mask, and s2c_pileup_counts, whose first launch
is k_reads over every piece (k_reads alone has no entry point, so its share is read from a
kernel trace of this script: rocprofv3 --kernel-trace --stats, the rows k_reads, k_links_count
and k_dels_*).  Then the deletions-only run against the counts-only run.  Times are HIP events
(kernels) or a host clock around work that ends in a device synchronise (whole runs); all of
`--reps` after a warm-up.

    python scripts/bench_dels.py --config c5 [--scale S] [--reps N] [--out profiles/dels_c5.json]

C4 draws no D token and C5 runs with -d (the rule off): --del-frac and --long-del-frac override
the configuration, and c5nd is C5 with the rule on, so that each has events, some of dropped reads."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_table import events, wall  # noqa: E402
from sam2consensus_amd import _lib as L  # noqa: E402
from sam2consensus_amd import configs  # noqa: E402
from sam2consensus_amd.cli import MIN_ALT_FRAC, MIN_ALT_READS  # noqa: E402
from sam2consensus_amd.engine import DeviceBatch, Workspace, _ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5", choices=["c2", "c4", "c5", "c5nd"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--del-frac", type=float, default=None)
    ap.add_argument("--long-del-frac", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or "profiles/dels_%s.json" % a.config
    dev = torch.device("cuda", 0)
    L.plan_for_device(dev)
    over = {}
    if a.del_frac is not None:
        over.update(del_frac=a.del_frac, del_max=5)
    if a.long_del_frac is not None:
        over.update(long_del_frac=a.long_del_frac)
    hb = configs.synth_batch(a.config, scale=a.scale, **over)
    db = DeviceBatch(hb, dev, dense_layers=True)
    ws = Workspace(db, [0.25], keep_counts=True)
    i, d = hb.info, ws.dev
    nt, plen, npc, nops, nq, nw = int(i.n_tiles), int(i.padded_len), int(i.n_pieces), int(i.n_ops), int(i.n_qwords), int(i.word_hi)
    st = ws.stream_handle()
    lib = L.lib
    t_pileup = events(lambda: (ws.counts.zero_(), L.check(lib.s2c_pileup_counts(C.byref(ws.dev), st))), a.reps)
    ws._counts_filled = True
    # the links walk over the same pieces (the default site rule's mask)
    mw = (plen + 63) // 64
    mask = torch.empty(max(mw, 1), dtype=torch.int64, device=dev)
    pop = torch.empty(max(mw, 1), dtype=torch.int32, device=dev)
    rank = torch.zeros(mw + 1, dtype=torch.int32, device=dev)
    L.check(lib.s2c_sites_mark(_ptr(ws.counts), plen, 1, MIN_ALT_READS, MIN_ALT_FRAC, _ptr(mask), st))
    L.check(lib.s2c_links_pop(_ptr(mask), plen, _ptr(pop), st))
    torch.cumsum(pop[:mw], 0, dtype=torch.int32, out=rank[1:])
    ns = int(rank[-1].item()) & 0xFFFFFFFF
    pairs = torch.empty(max(144 * ns, 16), dtype=torch.uint8, device=dev)

    def k_links():
        pairs.zero_()
        L.check(lib.s2c_links_count(_ptr(db.pc), _ptr(db.ops), _ptr(db.bq), _ptr(db.bx), npc, nq, int(d.maxdel_active),
                                    int(d.maxdel), _ptr(mask), _ptr(rank), plen, ns, _ptr(pairs), st))
    t_links = events(k_links, a.reps)
    del pairs
    # the six kernels
    total = torch.zeros(1, dtype=torch.int64, device=dev)

    def k_count():
        total.zero_()
        L.check(lib.s2c_dels_count(_ptr(db.pc), _ptr(db.ops), npc, nops, plen, _ptr(total), st))
    t_count = events(k_count, a.reps)
    E = int(total.item())
    n_slots = 1 << max((2 * max(E, 1) - 1).bit_length(), 1)
    slots = torch.empty(16 * n_slots, dtype=torch.uint8, device=dev)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    t_zero = events(lambda: slots.zero_(), a.reps)

    def k_collect():
        slots.zero_()
        L.check(lib.s2c_dels_collect(_ptr(db.pc), _ptr(db.ops), _ptr(db.bq), _ptr(db.bx), npc, nops, nq, int(d.maxdel_active),
                                     int(d.maxdel), plen, _ptr(slots), n_slots, _ptr(flag), st))
    t_collect = events(k_collect, a.reps)
    rows = slots.view(torch.int32).view(-1, 4)
    distinct = int((rows[:, 1] != 0).sum().item())
    dropped = int((rows[:, 3] != 0).sum().item())
    most = int(rows[:, 2].max().item()) if E else 0
    tcount, cursor, tn = (torch.zeros(max(nt, 4), dtype=torch.int32, device=dev) for _ in range(3))
    tstart = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
    ent = torch.empty(16 * max(E, 1), dtype=torch.uint8, device=dev)
    tmp = torch.empty(16 * max(E, 1), dtype=torch.uint8, device=dev)

    def k_bucket():
        tcount.zero_()
        cursor.zero_()
        L.check(lib.s2c_dels_tiles(_ptr(slots), n_slots, _ptr(db.wtile), nw, nt, _ptr(tcount), st))
        torch.cumsum(tcount[:nt], 0, dtype=torch.int64, out=tstart[1:])
        L.check(lib.s2c_dels_scatter(_ptr(slots), n_slots, _ptr(db.wtile), nw, nt, _ptr(tstart), _ptr(cursor), _ptr(ent), E, st))
    t_bucket = events(k_bucket, a.reps)
    names, tab, nbytes = ws._ref_names()
    blocks = ws._table_blocks()
    lens = torch.empty(nt, dtype=torch.int64, device=dev)
    offs_d = torch.zeros(nt + 1, dtype=torch.int64, device=dev)

    def k_len():   # (it orders ent in place; with min_reads 1 a repeat finds the same entries, ordered already)
        L.check(lib.s2c_dels_len(_ptr(ent), _ptr(tmp), E, _ptr(tstart), _ptr(db.tiles), nt, _ptr(blocks), _ptr(names), nbytes, _ptr(tab),
                                 int(i.n_refs), _ptr(ws.counts), plen, 1, _ptr(tn), _ptr(lens), st))
    t_len = events(k_len, a.reps) if E else [0.0]
    if not E:
        lens.zero_()
    torch.cumsum(lens, 0, out=offs_d[1:])
    nbytes_out = int(offs_d[-1].item())
    text = torch.empty(max(nbytes_out, 16), dtype=torch.uint8, device=dev)
    t_write = events(lambda: L.check(lib.s2c_dels_write(_ptr(ent), E, _ptr(tstart), _ptr(tn), _ptr(db.tiles), nt, _ptr(blocks), _ptr(names),
                                                        nbytes, _ptr(tab), int(i.n_refs), _ptr(ws.counts), plen, _ptr(offs_d), _ptr(text),
                                                        nbytes_out, st)), a.reps) if E else [0.0]
    lines = int(text[:nbytes_out].eq(10).sum().item())
    r_counts, r_dels = [], []
    for _ in range(a.reps):
        r_counts += wall(lambda: ws.run_with_tables({"counts": ()}), 1)
        r_dels += wall(lambda: ws.run_with_tables({}, deletions=1), 1)
    walks = min(t_count) + min(t_collect)
    res = {"workload": a.config, "scale": a.scale, "device": torch.cuda.get_device_name(dev), "overrides": over,
           "maxdel_active": int(d.maxdel_active), "pieces": npc, "tiles": nt, "positions": int(i.total_len),
           "events": E, "distinct": distinct, "distinct_with_dropped": dropped, "most_reads": most, "slots": n_slots,
           "overflow": int(flag[0].item()), "lines": lines, "bytes": nbytes_out,
           "k_dels_count_ms": t_count, "slots_zero_ms": t_zero, "k_dels_collect_with_zero_ms": t_collect,
           "bucket_ms": t_bucket, "k_dels_len_ms": t_len, "k_dels_write_ms": t_write,
           "k_links_count_with_zero_ms": t_links, "pileup_counts_ms": t_pileup,
           "dels_best_ms": round(walks + min(t_bucket) + min(t_len) + min(t_write), 4),
           "walks_over_links_count": round(walks / min(t_links), 3),
           "walks_over_pileup_counts": round(walks / min(t_pileup), 3),
           "run_counts_only_ms": r_counts, "run_deletions_only_ms": r_dels}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
