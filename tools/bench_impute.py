#!/usr/bin/env python3
"""Times the imputation of a dense X with NaN (NewUsers.impute, cmfrec_hip_newrows_impute) on an explicit model with random
factors: the HIP-event time of the fill kernel alone (impute_kernels.hpp, summed over the blocks of a call) and the wall time of
the call (uploads, the solve of the rows' factors, the fill, the download).

    sizes      4,096 x 10,000 with half of the entries missing; 4,096 x 160,112 with 99 % missing; one block of 4,096 x 10,000
               with 1 % missing, all of it in 5 % of the rows (what the row and tile skips are for)
    models     k = 50 and 128 in double precision, k = 64 in single precision; user and item biases, a global mean

One warm-up, then the median of `--runs` runs.  The kernel time is reported against two floors, and which of them binds:
    bytes      rows * n * s read + missing * s written + the factor bytes once, over 8 TB/s
    MFMA       2 * rows * n * kk over the matrix peak of the precision (78.6 / 157.3 TFLOP/s in double / single precision)
Nothing is gated on it: there is no earlier imputation to compare with.

    python tools/bench_impute.py                # every configuration, appended to profiles/impute/bench_impute.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("float64", 50), ("float64", 128), ("float32", 64)]
SIZES = {"half": (4096, 10000, 0.5, 1.0), "headline99": (4096, 160112, 0.99, 1.0), "skips1": (4096, 10000, 0.01, 0.05)}
HBM_BYTES_PER_S = 8e12
MFMA_FLOPS = {"float64": 78.6e12, "float32": 157.3e12}


def make_model(dtype, k, n):
    """A CMF that holds random item factors and biases as if fitted."""
    import numpy as np
    from cmfrec_amd import CMF
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    mdl = CMF(k=k, lambda_=5., user_bias=True, item_bias=True, use_float=dt is np.float32)
    mdl.B_ = (0.1 * rng.standard_normal((n, k))).astype(dt)
    mdl.C_ = np.zeros((0, k), dt)
    mdl._U_colmeans = np.zeros(0, dt)
    mdl.glob_mean_ = 3.1
    mdl.item_bias_ = (0.2 * rng.standard_normal(n)).astype(dt)
    mdl.Bi_ = np.zeros((0, 0), dt)
    mdl._TransBtBinvBt = None
    mdl._TransCtCinvCt = np.zeros((0, 0), dt)
    mdl._scaling_biasA = 1.
    mdl.is_fitted_ = True
    return mdl


def make_X(seed, rows, n, missing, row_share, dt):
    """Ratings in 0.5 .. 5 with `missing` of all entries NaN, spread over `row_share` of the rows."""
    import numpy as np
    rng = np.random.default_rng(seed)
    X = (0.5 * rng.integers(1, 11, (rows, n), dtype=np.int8)).astype(dt)
    hit = np.sort(rng.choice(rows, max(1, int(round(rows * row_share))), replace=False))
    p = missing / row_share
    for r in hit:
        X[r, rng.random(n) < p] = np.nan
    return X


def worker(dtype, k, size, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    dt = np.dtype(dtype).type
    rows, n, missing, row_share = SIZES[size]
    mdl = make_model(dtype, k, n)
    X = make_X(rows + n, rows, n, missing, row_share, dt)
    nmiss = int(np.isnan(X).sum())
    wall, fill, solve = [], [], []
    with mdl.new_users() as nu:
        for it in range(warmup + runs):
            s0 = time.perf_counter()
            out = nu.impute(X)
            s1 = time.perf_counter()
            if it >= warmup:
                sm, fm = nu.kernel_ms()
                wall.append((s1 - s0) * 1e3); fill.append(fm); solve.append(sm)
    assert not np.isnan(out).any()
    s = np.dtype(dt).itemsize
    floor_bytes = (rows * n * s + nmiss * s + (rows + n) * k * s) / HBM_BYTES_PER_S * 1e3
    floor_mfma = 2.0 * rows * n * k / MFMA_FLOPS[dtype] * 1e3
    med = lambda x: round(float(np.median(x)), 4)
    print(json.dumps(dict(what="impute", dtype=dtype, k=k, size=size, rows=rows, n=n, missing=nmiss, runs=runs, warmup=warmup,
                          fill_kernel_ms=med(fill), fill_kernel_ms_min=round(min(fill), 4), fill_kernel_ms_max=round(max(fill), 4),
                          solve_ms=med(solve), wall_ms=med(wall), floor_bytes_ms=round(floor_bytes, 4), floor_mfma_ms=round(floor_mfma, 4),
                          binding_floor="bytes" if floor_bytes >= floor_mfma else "mfma",
                          kernel_over_floor=round(float(np.median(fill)) / max(floor_bytes, floor_mfma), 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impute", "bench_impute.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:50")
    ap.add_argument("--sizes", default=",".join(SIZES), help="comma-separated subset of " + ", ".join(SIZES))
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "SIZE"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.worker[2], a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), sz] for sz in a.sizes.split(",") for dt, k in CONFIGS if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_impute: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
