"""The link tables' device cost on C2, C4 or C5: the four kernels of s2c_links.hip on a resident
batch — the ranks (s2c_links_pop and the prefix sum), the walk of every piece against the site
mask (s2c_links_count, with the zeroing of `pairs`), s2c_links_len and s2c_links_write — next to
two yardsticks in the same process: s2c_sites_len + s2c_sites_write over the same mask (the
formatter's), and s2c_pileup_counts, whose first launch is k_reads over every piece (the walk's;
k_reads alone has no entry point, so its share is read from a kernel trace of this script:
rocprofv3 --kernel-trace --stats, the rows k_reads and k_links_count).  Then the links-only run
against the variants-only run.  Times are HIP events (kernels) or a host clock around work that
ends in a device synchronise (whole runs); best and all of `--reps` after a warm-up.

    python scripts/bench_links.py --config c5 [--scale S] [--reps N] [--min-alt-frac F] [--out profiles/links_c5.json]

C4's minorities are substitutions at 1 % of 100,000 reads, far below the default 5 %: it is also
run with --min-alt-frac 0.0105, which leaves the positions whose minority is about two standard
deviations above the mean."""
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
    ap.add_argument("--config", default="c5", choices=["c2", "c4", "c5"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-alt-frac", type=float, default=MIN_ALT_FRAC)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or "profiles/links_%s.json" % a.config
    dev = torch.device("cuda", 0)
    L.plan_for_device(dev)
    hb = configs.synth_batch(a.config, scale=a.scale)
    db = DeviceBatch(hb, dev, dense_layers=True)
    ws = Workspace(db, [0.25], keep_counts=True)
    i = hb.info
    nt, plen, npc, nq = int(i.n_tiles), int(i.padded_len), int(i.n_pieces), int(i.n_qwords)
    st = ws.stream_handle()
    # the walk's yardstick: k_reads over every piece, then every tile's counts (left filled)
    t_pileup = events(lambda: (ws.counts.zero_(), L.check(L.lib.s2c_pileup_counts(C.byref(ws.dev), st))), a.reps)
    ws._counts_filled = True
    prm = (1, MIN_ALT_READS, a.min_alt_frac)
    blocks, refs = ws._table_blocks(), ws._table_refs()
    lens = torch.empty(nt, dtype=torch.int64, device=dev)
    offs_d = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
    nw = (plen + 63) // 64
    mask = torch.empty(max(nw, 1), dtype=torch.int64, device=dev)
    pop = torch.empty(max(nw, 1), dtype=torch.int32, device=dev)
    rank = torch.zeros(nw + 1, dtype=torch.int32, device=dev)
    t_mark = events(lambda: L.check(L.lib.s2c_sites_mark(_ptr(ws.counts), plen, prm[0], prm[1], prm[2], _ptr(mask), st)), a.reps)

    def k_rank():
        L.check(L.lib.s2c_links_pop(_ptr(mask), plen, _ptr(pop), st))
        torch.cumsum(pop[:nw], 0, dtype=torch.int32, out=rank[1:])
    t_rank = events(k_rank, a.reps)
    ns = int(rank[-1].item()) & 0xFFFFFFFF
    pairs = torch.empty(max(144 * ns, 16), dtype=torch.uint8, device=dev)
    d = ws.dev
    t_zero = events(lambda: pairs.zero_(), a.reps)

    def k_count():
        pairs.zero_()
        L.check(L.lib.s2c_links_count(_ptr(db.pc), _ptr(db.ops), _ptr(db.bq), _ptr(db.bx), npc, nq, int(d.maxdel_active),
                                      int(d.maxdel), _ptr(mask), _ptr(rank), plen, ns, _ptr(pairs), st))
    t_count = events(k_count, a.reps)
    adds = int(pairs.view(torch.int32).sum(dtype=torch.int64).item()) if ns else 0

    def two(length, write):
        t_len = events(length, a.reps)
        torch.cumsum(lens, 0, out=offs_d[1:])
        total = int(offs_d[-1].item())
        text = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        t_write = events(lambda: write(text, total), a.reps)
        return t_len, t_write, int(text[:total].eq(10).sum().item()), total

    l_len, l_write, lines, total = two(
        lambda: L.check(L.lib.s2c_links_len(_ptr(mask), _ptr(rank), plen, _ptr(pairs), ns, _ptr(blocks), _ptr(refs), nt, 1,
                                            _ptr(lens), st)),
        lambda text, n: L.check(L.lib.s2c_links_write(_ptr(mask), _ptr(rank), plen, _ptr(pairs), ns, _ptr(blocks), _ptr(refs),
                                                      _ptr(offs_d), nt, 1, _ptr(text), n, st)))
    s_len, s_write, s_lines, s_total = two(
        lambda: L.check(L.lib.s2c_sites_len(_ptr(ws.counts), plen, _ptr(mask), _ptr(blocks), nt, _ptr(lens), st)),
        lambda text, n: L.check(L.lib.s2c_sites_write(_ptr(ws.counts), plen, _ptr(mask), _ptr(blocks), _ptr(offs_d), nt,
                                                      _ptr(text), n, st)))
    del pairs
    r_sites, r_links = [], []
    for _ in range(a.reps):
        r_sites += wall(lambda: ws.run_with_tables({"variants": prm}), 1)
        r_links += wall(lambda: ws.run_with_tables({"links": prm + (1,)}), 1)
    links_ms = min(t_rank) + min(t_count) + min(l_len) + min(l_write)
    res = {"workload": a.config, "scale": a.scale, "device": torch.cuda.get_device_name(dev),
           "min_cov": prm[0], "min_alt": prm[1], "min_frac": prm[2],
           "pieces": npc, "tiles": nt, "positions": int(i.total_len), "n_sites": ns, "pairs_bytes": 144 * ns, "pair_adds": adds,
           "lines": lines, "bytes": total, "site_lines": s_lines, "site_bytes": s_total,
           "k_sites_mark_ms": t_mark, "rank_ms": t_rank, "pairs_zero_ms": t_zero, "k_links_count_with_zero_ms": t_count,
           "k_links_len_ms": l_len, "k_links_write_ms": l_write,
           "k_sites_len_ms": s_len, "k_sites_write_ms": s_write, "pileup_counts_ms": t_pileup,
           "links_best_ms": round(links_ms, 4), "count_share": round(min(t_count) / links_ms, 3),
           "format_over_sites_format": round((min(l_len) + min(l_write)) / (min(s_len) + min(s_write)), 3),
           "count_over_pileup_counts": round(min(t_count) / min(t_pileup), 3),
           "run_variants_only_ms": r_sites, "run_links_only_ms": r_links}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
