#!/usr/bin/env python3
"""Times the stochastic top-N of a ranking handle (cmfrec_amd.Ranker.topN_sample) against the deterministic
ranking it is built on: 16,384 Gaussian users against 160,112 items at n = 10, k = 50 / 128 / 256 in double and k = 64 / 272 in
single precision, T = the standard deviation of the scores.

    python tools/bench_topn_sample.py           # every configuration, appended to profiles/topn_sample/bench_topn_sample.jsonl

Three routes on one handle in one process, alternating run by run: `topN` under CMFREC_HIP_TOPN=wide (topn_wide_kernel, the
yardstick), `sample` (topn_sample_kernel<LSE = false> and the score kernel behind it) and `sample_lse` (LSE = true).  Per route
the HIP-event time on the handle's stream (cmfrec_hip_ranker_kernel_ms): median, minimum and maximum of 10 runs after 3 warm-ups.

`log_share`: the share of pairs whose logarithms are evaluated -- an ARITHMETIC ESTIMATE, not a counter: for 64 users of the
batch the kernel's rule is replayed in NumPy round by round (128 items a round, the threshold is the n-th best key after the
previous round, a pair is evaluated when score + T * ((clz(~h) + 1) ln 2 + c) reaches it).  The kernel's threshold also rises
inside a round, so the estimate is an upper bound by a little.

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N, NTOP = 16384, 160112, 10
CONFIGS = [("float64", 50), ("float64", 128), ("float64", 256), ("float32", 64), ("float32", 272)]
SEED = 2026


def log_share(A, B, T, seed, n_top, dtype, users=64):
    """The estimate described above, over the first `users` rows of A."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sample_reference as sr
    S = A[:users].astype(np.float64) @ B.astype(np.float64).T
    h = sr.hashes(seed, users, B.shape[0])
    K, KB = S + T * sr.gumbel(h, dtype), S + T * sr.gumbel_bound(h)
    evaluated = 0
    best = np.full((users, n_top), -np.inf)
    for c0 in range(0, B.shape[0], 128):
        evaluated += int((KB[:, c0:c0 + 128] >= best[:, :1]).sum())
        best = -np.sort(-np.concatenate([best, K[:, c0:c0 + 128]], axis=1), axis=1)[:, :n_top][:, ::-1]
    return evaluated / S.size


def worker(dtype, k, nu, n, n_top, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    B = rng.standard_normal((n, k)).astype(dt); A = rng.standard_normal((nu, k)).astype(dt)
    T = float(dt(np.sqrt(k)))                                            # the standard deviation of a Gaussian dot product
    kernel = {"topN": [], "sample": [], "sample_lse": []}
    shape = {}
    os.environ["CMFREC_HIP_TOPN"] = "wide"
    with Ranker(B) as rk:
        for it in range(warmup + runs):
            for route in kernel:
                if route == "topN":
                    rk.topN(A, n=n_top)
                else:
                    rk.topN_sample(A, n_top, T, SEED, with_lse=route == "sample_lse")
                if it >= warmup:
                    kernel[route].append(rk.kernel_ms())
                shape[route] = rk.launch_shape()
    share = log_share(A, B, T, SEED, n_top, dt)
    base = float(np.median(kernel["topN"]))
    for route, ms in kernel.items():
        users, groups = shape[route]
        print(json.dumps(dict(what="bench_topn_sample", route=route, dtype=dtype, k=k, n_top=n_top, nu=nu, n=n, temperature=T, runs=runs,
                              kernel_ms=round(float(np.median(ms)), 4), kernel_ms_min=round(min(ms), 4), kernel_ms_max=round(max(ms), 4),
                              ratio_to_topN=round(float(np.median(ms)) / base, 4), users_per_workgroup=users, workgroups=groups,
                              log_share_estimate=None if route == "topN" else round(share, 6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_sample", "bench_topn_sample.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--n-top", type=int, default=NTOP)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:128")
    ap.add_argument("--worker", nargs=2, metavar=("DTYPE", "K"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.nu, a.n, a.n_top, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k)] for dt, k in CONFIGS if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--nu", str(a.nu), "--n", str(a.n), "--n-top", str(a.n_top), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_topn_sample: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
