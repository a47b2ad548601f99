#!/usr/bin/env python3
"""Times the explanation kernel (Ranker.explain, topn_explain_kernels.hpp) against the closed-form solve of the same users'
factors on a NewUsers handle -- the same rank-k update and factorisation, for one right-hand side.

    python tools/bench_explain.py          # every configuration, appended to profiles/explain/bench.jsonl
    python tools/bench_explain.py --only float64:50

Shape: nu = 16,384 users against n = 160,112 Gaussian items, 10 random targets each, n_top = 10, histories of lognormal length
with the mean of the benchmark's rows (17,309,518 / 358,858 = 48.2 entries), values ceil(lognormal(3, 1.5)) as bench.py draws
them.  k = 50 and 128 in double, 64 and 127 in single precision; the model is an explicit one with a user bias (k + 1 unknowns; at
k = 128, where that is one too many for the kernel, without it).  The items are Gaussian: a CMF fitted for one iteration on a
64-user problem of that many items lends the NewUsers handle its settings, then takes the Gaussian rows as its B_.

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is started
on a device that has just faulted).  Within a child the two calls alternate run by run, after the warm-up runs.  Each line: median,
minimum and maximum of the HIP-event time of the explanation kernel (cmfrec_hip_ranker_kernel_ms) and of the new-rows solve
(cmfrec_hip_newrows_kernel_ms' first value), the ratio of the medians, and the wall time of both calls."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N, NTOP, NTARG = 16384, 160112, 10, 10
MEAN_LEN = 17309518 / 358858
CONFIGS = [("float64", 50), ("float64", 128), ("float32", 64), ("float32", 127)]


def histories(rng, nu, n, mean_len):
    """COO of nu users whose row lengths are lognormal(0, 1) scaled to mean_len (at least 1, at most n), items without repeats."""
    import numpy as np
    w = rng.lognormal(0, 1, nu)
    lens = np.clip(np.rint(w * (mean_len / w.mean())), 1, n).astype(np.int64)
    row = np.repeat(np.arange(nu, dtype=np.int32), lens)
    col = np.concatenate([rng.choice(n, size=l, replace=False) for l in lens]).astype(np.int32)
    return row, col, np.ceil(rng.lognormal(3, 1.5, len(row))), lens


def worker(dtype, k, nu, n, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import CMF, Ranker
    dt = np.dtype(dtype)
    rng = np.random.default_rng(k)
    bias = k < 128
    row, col, val, lens = histories(rng, nu, n, MEAN_LEN)
    val = val.astype(dt)
    targets = rng.integers(0, n, (nu, NTARG)).astype(np.int32)
    lam = 10.0
    lin = rng.choice(64 * n, size=4000, replace=False)
    srow = (lin // n).astype(np.int32); scol = (lin % n).astype(np.int32)
    mdl = CMF(k=k, lambda_=lam, niter=1, user_bias=bias, item_bias=False, precompute_for_predictions=False,
              use_float=dt == np.float32).fit((srow, scol, np.ones(4000)), shape=(64, n))
    mdl.B_ = np.ascontiguousarray(rng.standard_normal((n, k)), dt)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    hist = (indptr, col, np.ones(len(col), dt), (val - dt.type(mdl.glob_mean_)).astype(dt))
    t = dict(explain_ms=[], explain_call_ms=[], solve_ms=[], solve_call_ms=[])
    with Ranker(mdl.B_) as rk, mdl.new_users() as nw:
        for it in range(warmup + runs):
            t0 = time.perf_counter()
            rk.explain(hist, targets, n=NTOP, lam=lam, bias_lam=lam if bias else None)
            t1 = time.perf_counter()
            ex, shape = rk.kernel_ms(), rk.launch_shape()
            t2 = time.perf_counter()
            nw.factors((row, col, val))
            t3 = time.perf_counter()
            if it >= warmup:
                t["explain_ms"].append(ex); t["explain_call_ms"].append(1e3 * (t1 - t0))
                t["solve_ms"].append(nw.kernel_ms()[0]); t["solve_call_ms"].append(1e3 * (t3 - t2))
    line = dict(kernel="topn_explain_kernel", dtype=dtype, k=k, bias=int(bias), n_top=NTOP, targets=NTARG, nu=nu, n=n, runs=runs,
                nnz=int(len(col)), longest=int(lens.max()), workgroups=shape[1])
    for name, v in t.items():
        line[name] = round(float(np.median(v)), 4); line[name + "_min"] = round(min(v), 4); line[name + "_max"] = round(max(v), 4)
    line["explain_over_solve"] = round(line["explain_ms"] / line["solve_ms"], 3) if line["solve_ms"] > 0 else None
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain", "bench.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k[,dtype:k ...] in place of the standard four, e.g. float64:96,float32:100")
    ap.add_argument("--worker", nargs=2, metavar=("DTYPE", "K"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.nu, a.n, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    configs = CONFIGS if a.only is None else [(c.split(":")[0], int(c.split(":")[1])) for c in a.only.split(",")]
    common = ["--nu", str(a.nu), "--n", str(a.n), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for dt, k in configs:
            step = ["--worker", dt, str(k)]
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_explain: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
