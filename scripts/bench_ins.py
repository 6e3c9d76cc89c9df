"""The insertion tables' device cost on C2 (353 x 1,000 bp at 500x, 5 % of the reads with an
insertion): the two kernels of s2c_ins.hip on the resident insertion tables of the whole C2 and
of C2 with motifs of up to 40 bases (the long-event lists filled), next to the count table's two
kernels on the same counts in the same process, and the insertions-only run against the count
tables' run.  Times are HIP events (kernels) or a host clock around work that ends in a device
synchronise (whole runs); best and all of `--reps` after a warm-up.

    python scripts/bench_ins.py [--scale S] [--reps N] [--out profiles/ins_c2.json]

k_ins_len reads every hash slot and long event three times (count, scatter, then the entries it
bucketed), compares the entries of one position with each other and reads the six counts of
every line's position; k_ins_write reads the ordered entries and the six counts again and
stores the text byte by byte."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_table import events, wall  # noqa: E402
from sam2consensus_amd import _lib as L  # noqa: E402
from sam2consensus_amd import configs  # noqa: E402
from sam2consensus_amd.engine import DeviceBatch, Workspace, _ptr  # noqa: E402


def one(tag, over, a, dev):
    hb = configs.synth_batch("c2", scale=a.scale, **over)
    db = DeviceBatch(hb, dev, dense_layers=True)
    ws = Workspace(db, [0.25], keep_counts=True)
    ws.accumulate(keep_tables=True)       # every tile's counts and the insertion tables resident
    ws._counts_filled = True
    i = hb.info
    nt, plen = int(i.n_tiles), int(i.padded_len)
    n_bkt, n_lng, nq = int(i.n_bkt), int(i.n_lng), int(i.n_qwords)
    blocks = ws._table_blocks()
    st = ws.stream_handle()
    lens = torch.empty(nt, dtype=torch.int64, device=dev)
    offs_d = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(32 * (n_bkt + n_lng), 16), dtype=torch.uint8, device=dev)
    counts = _ptr(ws.counts)

    def two(length, write):
        t_len = events(length, a.reps)
        torch.cumsum(lens, 0, out=offs_d[1:])
        total = int(offs_d[-1].item())
        text = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        t_write = events(lambda: write(text, total), a.reps)
        return t_len, t_write, int(text[:total].eq(10).sum().item()), total

    i_len, i_write, lines, total = two(
        lambda: L.check(L.lib.s2c_ins_len(_ptr(db.tiles), nt, _ptr(ws.ibkt), n_bkt, _ptr(ws.ilong), n_lng, _ptr(ws.ilong_n),
                                          _ptr(db.bq), _ptr(db.bx), nq, counts, plen, _ptr(blocks), 1, _ptr(scratch),
                                          _ptr(lens), st)),
        lambda text, n: L.check(L.lib.s2c_ins_write(_ptr(db.tiles), nt, n_bkt, n_lng, _ptr(db.bq), _ptr(db.bx), nq, counts,
                                                    plen, _ptr(blocks), _ptr(scratch), _ptr(offs_d), _ptr(text), n, st)))
    # what went in: the occupied hash slots (one per distinct short motif at a position) and the long events
    slots = ws.ibkt[:16 * n_bkt].view(torch.int32).view(-1, 4) if n_bkt else torch.zeros((0, 4), dtype=torch.int32, device=dev)
    short_entries = int(((slots[:, 0] != 0) | (slots[:, 1] != 0)).sum().item())
    long_events = int(ws.ilong_n[:4 * nt].view(torch.int32).sum().item())
    t_len, t_write, t_lines, t_total = two(
        lambda: L.check(L.lib.s2c_table_len(counts, plen, _ptr(blocks), nt, _ptr(lens), st)),
        lambda text, n: L.check(L.lib.s2c_table_write(counts, plen, _ptr(blocks), _ptr(offs_d), nt, _ptr(text), n, st)))
    ws.vote_all()                          # (the tables consumed: the whole runs below start clean)
    r_counts, r_ins = [], []
    for _ in range(a.reps):
        r_counts += wall(ws.run_with_counts, 1)
        r_ins += wall(lambda: ws.run_with_tables({"insertions": (1,)}), 1)
    ins_ms, table_ms = min(i_len) + min(i_write), min(t_len) + min(t_write)
    return {tag: {"over": over, "tiles": nt, "events": int(i.n_ins), "event_bases": int(i.n_ins_bases), "hash_slots": n_bkt,
                  "long_slots": n_lng, "short_entries": short_entries, "long_events": long_events, "lines": lines, "bytes": total,
                  "k_ins_len_ms": i_len, "k_ins_write_ms": i_write, "ins_best_ms": round(ins_ms, 4),
                  "table_lines": t_lines, "table_bytes": t_total, "k_table_len_ms": t_len, "k_table_write_ms": t_write,
                  "table_best_ms": round(table_ms, 4), "ins_over_table": round(ins_ms / table_ms, 3),
                  "run_with_counts_ms": r_counts, "run_insertions_only_ms": r_ins}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/ins_c2.json")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.plan_for_device(dev)
    res = {"workload": "c2", "scale": a.scale, "device": torch.cuda.get_device_name(dev)}
    res.update(one("c2", {}, a, dev))
    res.update(one("c2_ins40", {"ins_max": 40}, a, dev))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
