"""The cluster CSV's export rate with both writers, in one session: `--n` synthetic rows (default 1 M) with mzML-style identifiers
(`controllerType=0 controllerNumber=1 scan=N`) from `--files` peak files, collected as falcon collects them -- one block per
precursor charge, each in the order the files were read.

The host path in full (`--csv_writer host`: a tuple per row, the sort by `_natural_key`, `_write_cluster_info`), once, its three
steps timed apart; the device path (`--csv_writer device`) step by step -- the blobs and file ranks (`csv_io.device_columns`,
host), the order (`Context.csv_order`, upload included), sizing plus formatting plus the copy to pinned memory
(`Context.format_csv`), the file write -- as the median of `--reps` passes after `--warmup` warm-ups, and end to end through
`falcon._write_outputs`.  The two files must be equal byte for byte.  Prints one JSON line, and writes the report to `--out`.

    python tools/csv_rate.py [--n 1000000] [--files 7] [--reps 3] [--warmup 1] [--dir DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def synthetic_blocks(n, n_files, seed=42):
    """-> column blocks, one per charge (2, 3, none), rows in file and scan order inside a block"""
    from falcon_amd.ms_io import csv_io
    rng = np.random.default_rng(seed)
    per_file = -(-n // n_files)
    names = np.array([f"/data/run{7 * f + 3}_fraction{f}.mzML" for f in range(n_files)])
    file_of = np.repeat(np.arange(n_files), per_file)[:n]
    scan = np.tile(np.arange(1, per_file + 1), n_files)[:n]
    ident = np.char.add("controllerType=0 controllerNumber=1 scan=", scan.astype(str))
    charge = rng.choice([2, 3, 0], size=n, p=[0.55, 0.4, 0.05])
    pmz = rng.uniform(300, 1500, n).astype(np.float32)
    rt = rng.uniform(0, 7200, n).astype(np.float32)
    blocks, base = [], 0
    for z in (2, 3, 0):
        rows = np.flatnonzero(charge == z)
        labels = rng.integers(0, max(len(rows) // 2, 1), len(rows)).astype(np.int64) + base
        base += max(len(rows) // 2, 1)
        blocks.append(csv_io.column_block(names[file_of[rows]], ident[rows], z, pmz[rows], rt[rows], labels))
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--files", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="timed passes of the device path's steps")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", type=str, default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "peakfiles", "csv_write_rate_1M.txt"))
    a = ap.parse_args()
    import torch
    from falcon_amd import falcon
    from falcon_amd.config import config
    from falcon_amd.device import Context
    from falcon_amd.ms_io import csv_io
    ctx = Context(0)
    ctx.plan(0)
    blocks = synthetic_blocks(a.n, a.files)
    clock = time.perf_counter
    res = dict(tool="csv_rate", n=a.n, files=a.files, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        # ---- host path, in full, once
        config.parse(["in.mzML", os.path.join(tmp, "host"), "--work_dir", "w", "--csv_writer", "host"])
        t0 = clock()
        rows_all = list(csv_io.block_tuples(blocks))
        t1 = clock()
        rows_all.sort(key=lambda r: (falcon._natural_key(r[0]), falcon._natural_key(r[1])))
        t2 = clock()
        falcon._write_cluster_info(rows_all)
        t3 = clock()
        del rows_all
        res.update(host_tuples_s=round(t1 - t0, 3), host_sort_s=round(t2 - t1, 3), host_write_s=round(t3 - t2, 3),
                   host_total_s=round(t3 - t0, 3))
        # ---- device path, step by step
        steps = dict(blobs=[], order=[], format=[], file=[])
        n_bytes = 0
        for rep in range(a.warmup + a.reps):
            t0 = clock()
            cols, why = csv_io.device_columns(blocks, falcon._natural_key)
            assert why is None, why
            t1 = clock()
            order = csv_io.sort_rows(ctx, cols)
            assert order is not None
            ctx.sync()
            t2 = clock()
            columns = {k: v for k, v in cols.items() if k != "file_rank"}
            chunks = [c for c in ctx.format_csv(**columns, order=order)]        # (copies: what a chunk's file write then takes)
            t3 = clock()
            with open(os.path.join(tmp, "steps.csv"), "wb") as f:
                for c in chunks:
                    f.write(memoryview(c))
            t4 = clock()
            n_bytes = sum(len(c) for c in chunks)
            del chunks
            if rep >= a.warmup:
                for k, v in zip(("blobs", "order", "format", "file"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    steps[k].append(v)
        for k, v in steps.items():
            res[f"device_{k}_s"] = round(float(np.median(v)), 4)
            res[f"device_{k}_min_s"] = round(float(min(v)), 4)
        # ---- device path, end to end through falcon._write_outputs
        ends = []
        for rep in range(a.warmup + a.reps):
            config.parse(["in.mzML", os.path.join(tmp, "device"), "--work_dir", "w", "--csv_writer", "device"])
            if os.path.exists(os.path.join(tmp, "device.csv")):
                os.remove(os.path.join(tmp, "device.csv"))
            t0 = clock()
            falcon._write_outputs([], [], ctx, csv_blocks=blocks)
            if rep >= a.warmup:
                ends.append(clock() - t0)
        res.update(device_total_s=round(float(np.median(ends)), 4), device_total_min_s=round(float(min(ends)), 4), rows_bytes=n_bytes)
        host, dev = (open(os.path.join(tmp, f"{w}.csv"), "rb").read() for w in ("host", "device"))
        res.update(file_bytes=len(host), files_equal=bool(host == dev))
    res["host_over_device"] = round(res["host_total_s"] / res["device_total_s"], 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# python tools/csv_rate.py --n {a.n} --files {a.files} --reps {a.reps} --warmup {a.warmup}\n")
            f.write("# host: tuples, sort by _natural_key, _write_cluster_info, once; device: median (and minimum) of the timed passes\n")
            for k, v in res.items():
                f.write(f"{k} = {v}\n")
            f.write(line + "\n")
    ctx.close()
    return 0 if res["files_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
