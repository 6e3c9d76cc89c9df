"""The tables of mixed sites' device cost on C5 (64.4 M positions): the three kernels of
s2c_sites.hip on resident counts at the default parameters against the count table's two
kernels on the same counts in the same process (the yardstick: a dense table filtered on the
host would need them), and the variants-only run against the whole counts route.  Times are
HIP events (kernels) or a host clock around work that ends in a device synchronise (whole
runs); best and all of `--reps` after a warm-up.

    python scripts/bench_sites.py [--scale S] [--reps N] [--out profiles/sites_c5.json]

Two passes over the counts cost 48 B per position; mark, then len and write over the mask, cost
24 B + 2 x 1/8 B per position plus the rows of the sites themselves."""
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
    ap.add_argument("--out", default="profiles/sites_c5.json")
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
    prm = (1, MIN_ALT_READS, MIN_ALT_FRAC)
    blocks = ws._table_blocks()
    st = ws.stream_handle()
    lens = torch.empty(nt, dtype=torch.int64, device=dev)
    offs_d = torch.zeros(nt + 1, dtype=torch.int64, device=dev)
    mask = torch.empty(max((plen + 63) // 64, 1), dtype=torch.int64, device=dev)

    def k_mark():
        L.check(L.lib.s2c_sites_mark(_ptr(ws.counts), plen, prm[0], prm[1], prm[2], _ptr(mask), st))

    def k_len():
        L.check(L.lib.s2c_sites_len(_ptr(ws.counts), plen, _ptr(mask), _ptr(blocks), nt, _ptr(lens), st))
    t_mark = events(k_mark, a.reps)
    t_len = events(k_len, a.reps)
    torch.cumsum(lens, 0, out=offs_d[1:])
    total = int(offs_d[-1].item())
    text = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)

    def k_write():
        L.check(L.lib.s2c_sites_write(_ptr(ws.counts), plen, _ptr(mask), _ptr(blocks), _ptr(offs_d), nt, _ptr(text),
                                      total, st))
    t_write = events(k_write, a.reps)
    n_sites = int(text[:total].eq(10).sum().item())   # one newline per site line
    del text

    # the yardstick: the dense table's kernels on the same counts
    def t_klen():
        L.check(L.lib.s2c_table_len(_ptr(ws.counts), plen, _ptr(blocks), nt, _ptr(lens), st))
    t_tlen = events(t_klen, a.reps)
    torch.cumsum(lens, 0, out=offs_d[1:])
    ttotal = int(offs_d[-1].item())
    ttext = torch.empty(max(ttotal, 16), dtype=torch.uint8, device=dev)

    def t_kwrite():
        L.check(L.lib.s2c_table_write(_ptr(ws.counts), plen, _ptr(blocks), _ptr(offs_d), nt, _ptr(ttext), ttotal, st))
    t_twrite = events(t_kwrite, a.reps)
    del ttext
    b = blocks.view(-1, 3)
    positions = int((b[:, 1] - b[:, 0]).sum().item())
    # the whole routes on the same resident batch, alternated
    t_counts, t_sites = [], []
    for _ in range(a.reps):
        t_counts += wall(ws.run_with_counts, 1)
        t_sites += wall(lambda: ws.run_with_tables({"variants": prm}), 1)
    sites_ms = min(t_mark) + min(t_len) + min(t_write)
    table_ms = min(t_tlen) + min(t_twrite)
    res = {"workload": "c5", "scale": a.scale, "positions": positions, "tiles": nt,
           "min_cov": prm[0], "min_alt": prm[1], "min_frac": prm[2],
           "sites": n_sites, "sites_bytes": total, "table_bytes": ttotal,
           "k_sites_mark_ms": t_mark, "k_sites_len_ms": t_len, "k_sites_write_ms": t_write,
           "k_table_len_ms": t_tlen, "k_table_write_ms": t_twrite,
           "sites_best_ms": round(sites_ms, 4), "table_best_ms": round(table_ms, 4),
           "sites_over_table": round(sites_ms / table_ms, 3),
           "sites_over_table_len": round(sites_ms / min(t_tlen), 3),
           "mark_GBps": round(24 * plen / min(t_mark) / 1e6, 1),
           "run_with_counts_ms": t_counts, "run_variants_only_ms": t_sites,
           "device": torch.cuda.get_device_name(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
