#!/usr/bin/env python3
"""Times the neighbour call of a ranking handle (cmfrec_amd.Ranker.similar, cosine) against the route a user had before it:
nq = 16,384 query items against n = 160,112 items at n_top = 10 (the table of all items against themselves is too long for one
timed call), k = 50 / 128 in double and k = 64 / 272 in single precision.

    python tools/bench_similar.py               # every configuration, appended to profiles/similar/bench_similar.jsonl

The route before: normalise the rows on the host, make a second Ranker over the normalised copy, upload the query rows as
"users", build one exclusion list per query that holds the query itself, and rank with CMFREC_HIP_TOPN=wide (the same matrix
product on the same tiling, the same lists).  Both routes run in one process, alternating run by run; the switches are re-read
on every call.  Per route: the HIP-event time of the kernel (cmfrec_hip_ranker_kernel_ms; median, minimum and maximum of 10 runs
after 3 warm-ups) and the wall time of the whole call.  The earlier route's call time counts what a caller repeats per batch --
gathering the query rows, the exclusion lists, the upload, the ranking -- and leaves out what it pays once (the normalised copy
and its ranker: `setup_s`); the new route's leaves out the norm kernel of the first call (`norms_first_call_s` is that call's
extra wall time).

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, N, NTOP = 16384, 160112, 10
CONFIGS = [("float64", 50), ("float64", 128), ("float32", 64), ("float32", 272)]


def worker(dtype, k, nq, n, n_top, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    B = rng.standard_normal((n, k)).astype(dt)
    q = rng.choice(n, nq, replace=False).astype(np.int32)
    t0 = time.perf_counter()
    Bn = (B / np.sqrt((B * B).sum(axis=1, dtype=dt))[:, None]).astype(dt)
    before = Ranker(Bn)
    setup_s = time.perf_counter() - t0
    kernel = {"similar": [], "before": []}
    wall = {"similar": [], "before": []}
    shape = {}
    with before, Ranker(B) as rk:
        t0 = time.perf_counter()
        rk.similar(q[:16], n=n_top)                                      # builds the norms
        first = time.perf_counter() - t0
        t0 = time.perf_counter()
        rk.similar(q[:16], n=n_top)
        norms_first_call_s = first - (time.perf_counter() - t0)
        for it in range(warmup + runs):
            os.environ.pop("CMFREC_HIP_TOPN", None)
            t0 = time.perf_counter()
            ids_new, _ = rk.similar(q, n=n_top)
            t1 = time.perf_counter()
            os.environ["CMFREC_HIP_TOPN"] = "wide"
            t2 = time.perf_counter()
            ids_old, _ = before.topN(Bn[q], n=n_top, exclude=(np.arange(nq + 1, dtype=np.uint64), q))
            t3 = time.perf_counter()
            if it >= warmup:
                kernel["similar"].append(rk.kernel_ms()); kernel["before"].append(before.kernel_ms())
                wall["similar"].append(t1 - t0); wall["before"].append(t3 - t2)
            shape["similar"] = rk.launch_shape(); shape["before"] = before.launch_shape()
    os.environ.pop("CMFREC_HIP_TOPN", None)
    agree = float((ids_new == ids_old).mean())                           # (the two round differently: near ties may swap)
    for route in ("similar", "before"):
        users, groups = shape[route]
        print(json.dumps(dict(what="bench_similar", route=route, kernel="topn_similar_kernel" if route == "similar" else "topn_wide_kernel",
                              metric="cosine", dtype=dtype, k=k, n_top=n_top, nq=nq, n=n, runs=runs,
                              kernel_ms=round(float(np.median(kernel[route])), 4), kernel_ms_min=round(min(kernel[route]), 4),
                              kernel_ms_max=round(max(kernel[route]), 4),
                              call_s=round(float(np.median(wall[route])), 4), call_s_min=round(min(wall[route]), 4),
                              call_s_max=round(max(wall[route]), 4), users_per_workgroup=users, workgroups=groups,
                              setup_s=round(setup_s, 4) if route == "before" else None,
                              norms_first_call_s=round(norms_first_call_s, 4) if route == "similar" else None,
                              ids_equal_share=round(agree, 6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar", "bench_similar.jsonl"))
    ap.add_argument("--nq", type=int, default=NQ)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--n-top", type=int, default=NTOP)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:128")
    ap.add_argument("--worker", nargs=2, metavar=("DTYPE", "K"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.nq, a.n, a.n_top, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k)] for dt, k in CONFIGS if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--nq", str(a.nq), "--n", str(a.n), "--n-top", str(a.n_top), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_similar: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
