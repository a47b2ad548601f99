#!/usr/bin/env python3
"""Times diversified top-N (Ranker.topN_diverse: the handle's ranking of n_top = pool, then topn_mmr_kernel over the pools on the
device) by the protocol of tools/bench_topn.py: nu = 16,384 random users against n = 160,112 items, n = 10, median of 10 runs
after 3 warm-ups.

    python tools/bench_topn_diverse.py          # every configuration, appended to profiles/topn_diverse/bench.jsonl
    python tools/bench_topn_diverse.py --only float64:96

Every (precision, k) runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted).  Within a child, for pool = 32, 64 and 128 two calls alternate run by run: topN_diverse,
and Ranker.topN(n = pool) -- the part of the cost that exists without the re-ranking.

Each line: the HIP-event time of the MMR kernel (cmfrec_hip_ranker_kernel_ms after topN_diverse), the wall time of the topN_diverse
call, and beside them the ranking kernel's time and the wall time of topN(n = pool) on the same handle; the workgroups of the MMR
launch."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N, NTOP = 16384, 160112, 10
CONFIGS = [("float64", 50), ("float64", 128), ("float64", 256), ("float32", 272)]
POOLS = (32, 64, 128)


def worker(dtype, k, nu, n, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    A = rng.standard_normal((nu, k)).astype(dt); B = rng.standard_normal((n, k)).astype(dt)
    with Ranker(B) as rk:
        for pool in POOLS:
            t = dict(mmr_ms=[], diverse_call_ms=[], topn_ms=[], topn_call_ms=[])
            for it in range(warmup + runs):
                t0 = time.perf_counter()
                rk.topN_diverse(A, n=NTOP, pool=pool, tradeoff=0.7)
                t1 = time.perf_counter()
                mmr, shape = rk.kernel_ms(), rk.launch_shape()
                t2 = time.perf_counter()
                rk.topN(A, n=pool)
                t3 = time.perf_counter()
                if it >= warmup:
                    t["mmr_ms"].append(mmr); t["diverse_call_ms"].append(1e3 * (t1 - t0))
                    t["topn_ms"].append(rk.kernel_ms()); t["topn_call_ms"].append(1e3 * (t3 - t2))
            line = dict(kernel="topn_mmr_kernel", dtype=dtype, k=k, n_top=NTOP, pool=pool, tradeoff=0.7, nu=nu, n=n, runs=runs, workgroups=shape[1])
            for name, v in t.items():
                line[name] = round(float(np.median(v)), 4); line[name + "_min"] = round(min(v), 4); line[name + "_max"] = round(max(v), 4)
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_diverse", "bench.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k[,dtype:k ...] in place of the standard four, e.g. float64:96,float32:128")
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
                sys.stderr.write("\nbench_topn_diverse: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
