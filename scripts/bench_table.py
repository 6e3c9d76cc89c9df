"""The count tables' device cost on C5 (64.4 M positions): the two kernels of s2c_table.hip on
resident counts against a device-to-device copy of the bytes they move, and the whole counts
route against the plain run.  Times are HIP events (kernels, copy) or a host clock around work
that ends in a device synchronise (whole runs); best and all of `--reps` after a warm-up.

    python scripts/bench_table.py [--scale S] [--reps N] [--out profiles/table_c5.json]

The copy is the yardstick: each pass reads the six u32 rows (24 B per position, 48 B for the
two), the second writes the text; a copy of n bytes reads n and writes n, so it is sized at
half of (48 B x positions + text bytes)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sam2consensus_amd import _lib as L  # noqa: E402
from sam2consensus_amd import configs  # noqa: E402
from sam2consensus_amd.engine import DeviceBatch, Workspace, _ptr  # noqa: E402


def events(f, reps):
    """ms of f() on the current stream by device events: one warm-up, then reps."""
    out = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        if k:
            out.append(e0.elapsed_time(e1))
    return out


def wall(f, reps):
    """ms of f() + device synchronise by the host clock: one warm-up, then reps."""
    out = []
    for k in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/table_c5.json")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.plan_for_device(dev)
    hb = configs.synth_batch("c5", scale=a.scale)
    db = DeviceBatch(hb, dev, dense_layers=True)
    ws = Workspace(db, [0.25], keep_counts=True)
    ws.accumulate(keep_tables=False)      # every tile's counts resident
    ws._counts_filled = True
    i = hb.info
    nt = int(i.n_tiles)
    blocks = ws._table_blocks()
    st = ws.stream_handle()
    lens = torch.empty(nt, dtype=torch.int64, device=dev)
    offs_d = torch.zeros(nt + 1, dtype=torch.int64, device=dev)

    def k_len():
        L.check(L.lib.s2c_table_len(_ptr(ws.counts), i.padded_len, _ptr(blocks), nt, _ptr(lens), st))
    t_len = events(k_len, a.reps)
    torch.cumsum(lens, 0, out=offs_d[1:])
    total = int(offs_d[-1].item())
    text = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)

    def k_write():
        L.check(L.lib.s2c_table_write(_ptr(ws.counts), i.padded_len, _ptr(blocks), _ptr(offs_d), nt, _ptr(text), total, st))
    t_write = events(k_write, a.reps)
    b = blocks.view(-1, 3)
    positions = int((b[:, 1] - b[:, 0]).sum().item())
    moved = 48 * positions + total
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev).fill_(7)
    dst = torch.empty_like(src)
    t_copy = events(lambda: dst.copy_(src), a.reps)
    del src, dst, text
    # the whole routes on the same resident batch, alternated
    wp = Workspace(db, [0.25])
    t_plain, t_counts = [], []
    for _ in range(a.reps):
        t_plain += wall(wp.run, 1)
        t_counts += wall(ws.run_with_counts, 1)
    kern = min(t_len) + min(t_write)
    res = {"workload": "c5", "scale": a.scale, "positions": positions, "tiles": nt, "table_bytes": total,
           "bytes_per_position": round(total / max(positions, 1), 3), "bytes_moved": moved,
           "k_table_len_ms": t_len, "k_table_write_ms": t_write, "d2d_copy_ms": t_copy, "d2d_copy_bytes": moved // 2,
           "kernels_best_ms": round(kern, 4), "copy_best_ms": round(min(t_copy), 4),
           "kernels_over_copy": round(kern / min(t_copy), 3),
           "kernels_GBps": round(moved / kern / 1e6, 1), "copy_GBps": round(moved / min(t_copy) / 1e6, 1),
           "run_plain_ms": t_plain, "run_with_counts_ms": t_counts,
           "device": torch.cuda.get_device_name(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
