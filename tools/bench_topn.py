#!/usr/bin/env python3
"""Times the batched top-N ranking kernels through a ranking handle (cmfrec_amd.Ranker): nu = 16,384 random users against
n = 160,112 items, the HIP-event time of the kernel (cmfrec_hip_ranker_kernel_ms), median of 10 runs after 3 warm-ups.

    python tools/bench_topn.py                  # every configuration, appended to profiles/topn/bench_topn.jsonl
    python tools/bench_topn.py --handle         # plus the end-to-end gain of the handle (k = 128, double precision)

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted).  At k <= 64 both routes are timed in one process, alternating run by run: the default
kernel (topn_kernel) and CMFREC_HIP_TOPN=wide (topn_wide_kernel); the switches are re-read on every call.

Each line: milliseconds, the product rate 2 nu n k / t as a fraction of the matrix peak of the precision (78.6 TF double,
157.3 TF single), the item bytes streamed per second (the items are read once per workgroup's users: launch_shape)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N = 16384, 160112
PEAK = {"float64": 78.6e12, "float32": 157.3e12}
CONFIGS = [("float64", k) for k in (50, 64, 128, 256)] + [("float32", k) for k in (64, 256, 272)]
NTOPS = (10, 100)


def worker(dtype, k, n_top, nu, n, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    A = rng.standard_normal((nu, k)).astype(dt); B = rng.standard_normal((n, k)).astype(dt)
    routes = ["default", "wide"] if k <= 64 else ["default"]
    ms = {r: [] for r in routes}
    shape = {}
    with Ranker(B) as rk:
        for it in range(warmup + runs):
            for route in routes:
                if route == "wide":
                    os.environ["CMFREC_HIP_TOPN"] = "wide"
                else:
                    os.environ.pop("CMFREC_HIP_TOPN", None)
                rk.topN(A, n=n_top)
                if it >= warmup:
                    ms[route].append(rk.kernel_ms())
                shape[route] = rk.launch_shape()
    for route in routes:
        t = float(np.median(ms[route])) * 1e-3
        users, groups = shape[route]
        kernel = "topn_wide_kernel" if (route == "wide" or k > 64) else "topn_kernel"
        tiles = (nu + users - 1) // users
        print(json.dumps(dict(kernel=kernel, route=route, dtype=dtype, k=k, n_top=n_top, nu=nu, n=n, ms=round(t * 1e3, 4),
                              ms_min=round(min(ms[route]), 4), ms_max=round(max(ms[route]), 4), runs=runs,
                              users_per_workgroup=users, workgroups=groups,
                              product_rate_tflops=round(2.0 * nu * n * k / t / 1e12, 3),
                              fraction_of_matrix_peak=round(2.0 * nu * n * k / t / PEAK[dtype], 4),
                              item_bytes_per_s=round(tiles * n * k * np.dtype(dt).itemsize / t, 1))), flush=True)


def handle_worker(nu, n):
    """Wall time of 8 batches of 2,048 users at k = 128, double precision: ops.topN_batch per batch (B uploaded 8 times)
    against one Ranker serving the 8 calls (B uploaded once; its creation is inside the timed region)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker, ops
    k, nb, per = 128, 8, 2048
    rng = np.random.default_rng(1)
    A = rng.standard_normal((nb * per, k)); B = rng.standard_normal((n, k))
    ops.topN_batch(A[:64], B[:4096], 10)                                   # library, device and kernels loaded
    out = {}
    for rep in range(3):
        t0 = time.perf_counter()
        a = [ops.topN_batch(A[i * per:(i + 1) * per], B, 10)[0] for i in range(nb)]
        t1 = time.perf_counter()
        with Ranker(B) as rk:
            b = [rk.topN(A[i * per:(i + 1) * per], n=10)[0] for i in range(nb)]
        t2 = time.perf_counter()
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        out.setdefault("topN_batch_s", []).append(round(t1 - t0, 4)); out.setdefault("ranker_s", []).append(round(t2 - t1, 4))
    print(json.dumps(dict(what="handle_end_to_end", dtype="float64", k=k, n=n, batches=nb, users_per_batch=per, n_top=10,
                          topN_batch_s=out["topN_batch_s"], ranker_s=out["ranker_s"],
                          gain=round(min(out["topN_batch_s"]) / min(out["ranker_s"]), 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn", "bench_topn.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--handle", action="store_true")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:128")
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "NTOP"))
    ap.add_argument("--handle-worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), int(a.worker[2]), a.nu, a.n, a.runs, a.warmup)
    if a.handle_worker:
        return handle_worker(a.nu, a.n)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), str(nt)] for dt, k in CONFIGS for nt in NTOPS if a.only in (None, "%s:%d" % (dt, k))]
    if a.handle:
        steps.append(["--handle-worker"])
    common = ["--nu", str(a.nu), "--n", str(a.n), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_topn: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
