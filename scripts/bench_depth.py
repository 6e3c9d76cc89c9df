"""The run tables' device cost on C5 (64.4 M positions): the three kernels of s2c_runs.hip on
resident counts for the depth intervals (cut = 0) and for the low-coverage mask (cut = max(-m,
1)), against the sites route's three kernels and the count table's two on the same counts in
the same process, and the runs-only run against the whole counts route.  Times are HIP events
(kernels) or a host clock around work that ends in a device synchronise (whole runs); best and
all of `--reps` after a warm-up.

    python scripts/bench_depth.py [--scale S] [--reps N] [--min-depth M] [--out profiles/depth_c5.json]

mark reads the counts once, 24 B per position, as k_sites_mark does; len and write read 1/8 B
per position of mask each plus the six counts of every run's first position, and write reads
them again for the text."""
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
from sam2consensus_amd.cli import MIN_ALT_FRAC, MIN_ALT_READS  # noqa: E402
from sam2consensus_amd.engine import DeviceBatch, Workspace, _ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-depth", type=int, default=1)
    ap.add_argument("--out", default="profiles/depth_c5.json")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.plan_for_device(dev)
    hb = configs.synth_batch("c5", scale=a.scale)
    db = DeviceBatch(hb, dev, dense_layers=True)
    ws = Workspace(db, [0.25], keep_counts=True)
    ws.accumulate(keep_tables=False)      # every tile's counts resident
    ws._counts_filled = True
    i = hb.info
    nt, plen = int(i.n_tiles), int(i.padded_len)
    least = max(a.min_depth, 1)
    blocks, refs = ws._table_blocks(), ws._table_refs()
    st = ws.stream_handle()
    lens = torch.empty(nt, dtype=torch.int64, device=dev)
    stats = torch.empty(nt * 6, dtype=torch.int64, device=dev)
    offs_d = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
    mask = torch.empty(max((plen + 63) // 64, 1), dtype=torch.int64, device=dev)
    counts = _ptr(ws.counts)

    def three(mark, length, write):
        """ms of the three launches of one route, the lines and the bytes of its text"""
        t_mark = events(mark, a.reps)
        t_len = events(length, a.reps)
        torch.cumsum(lens, 0, out=offs_d[1:])
        total = int(offs_d[-1].item())
        text = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        t_write = events(lambda: write(text, total), a.reps)
        lines = int(text[:total].eq(10).sum().item())   # one newline per line
        return t_mark, t_len, t_write, lines, total

    res = {"workload": "c5", "scale": a.scale, "tiles": nt, "min_cov": least}
    for tag, cut in (("depth", 0), ("lowcov", least)):
        t_mark, t_len, t_write, lines, total = three(
            lambda: L.check(L.lib.s2c_runs_mark(counts, plen, cut, _ptr(mask), st)),
            lambda: L.check(L.lib.s2c_runs_len(counts, plen, _ptr(mask), _ptr(blocks), _ptr(refs), nt, cut, least, _ptr(lens),
                                               _ptr(stats), st)),
            lambda text, total: L.check(L.lib.s2c_runs_write(counts, plen, _ptr(mask), _ptr(blocks), _ptr(refs), _ptr(offs_d),
                                                             nt, cut, _ptr(text), total, st)))
        res.update({tag + "_lines": lines, tag + "_bytes": total, "k_runs_mark_" + tag + "_ms": t_mark,
                    "k_runs_len_" + tag + "_ms": t_len, "k_runs_write_" + tag + "_ms": t_write,
                    tag + "_best_ms": round(min(t_mark) + min(t_len) + min(t_write), 4),
                    "mark_" + tag + "_GBps": round(24 * plen / min(t_mark) / 1e6, 1)})
        if not cut:
            s = stats.view(nt, 6)
            res.update(covered=int(s[:, 1].sum().item()), passed=int(s[:, 2].sum().item()), sumcov=int(s[:, 3].sum().item()),
                       maxcov=int(s[:, 5].max().item()))
    # the yardsticks: the sites route at the default parameters and the dense table, same counts
    prm = (least, MIN_ALT_READS, MIN_ALT_FRAC)
    s_mark, s_len, s_write, n_sites, s_total = three(
        lambda: L.check(L.lib.s2c_sites_mark(counts, plen, prm[0], prm[1], prm[2], _ptr(mask), st)),
        lambda: L.check(L.lib.s2c_sites_len(counts, plen, _ptr(mask), _ptr(blocks), nt, _ptr(lens), st)),
        lambda text, total: L.check(L.lib.s2c_sites_write(counts, plen, _ptr(mask), _ptr(blocks), _ptr(offs_d), nt, _ptr(text),
                                                          total, st)))
    _, t_len, t_write, _, t_total = three(
        lambda: None,
        lambda: L.check(L.lib.s2c_table_len(counts, plen, _ptr(blocks), nt, _ptr(lens), st)),
        lambda text, total: L.check(L.lib.s2c_table_write(counts, plen, _ptr(blocks), _ptr(offs_d), nt, _ptr(text), total, st)))
    b = blocks.view(-1, 3)
    positions = int((b[:, 1] - b[:, 0]).sum().item())
    # the whole routes on the same resident batch, alternated
    r_counts, r_depth, r_low = [], [], []
    for _ in range(a.reps):
        r_counts += wall(ws.run_with_counts, 1)
        r_depth += wall(lambda: ws.run_with_tables({"depth": (least,)}), 1)
        r_low += wall(lambda: ws.run_with_tables({"lowcov": (least,)}), 1)
    sites_ms = min(s_mark) + min(s_len) + min(s_write)
    table_ms = min(t_len) + min(t_write)
    res.update({"positions": positions, "sites": n_sites, "sites_bytes": s_total, "table_bytes": t_total,
                "k_sites_mark_ms": s_mark, "k_sites_len_ms": s_len, "k_sites_write_ms": s_write,
                "k_table_len_ms": t_len, "k_table_write_ms": t_write,
                "sites_best_ms": round(sites_ms, 4), "table_best_ms": round(table_ms, 4),
                "depth_over_sites": round(res["depth_best_ms"] / sites_ms, 3),
                "depth_over_table": round(res["depth_best_ms"] / table_ms, 3),
                "lowcov_over_sites": round(res["lowcov_best_ms"] / sites_ms, 3),
                "run_with_counts_ms": r_counts, "run_depth_only_ms": r_depth, "run_lowcov_only_ms": r_low,
                "device": torch.cuda.get_device_name(dev)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
