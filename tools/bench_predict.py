#!/usr/bin/env python3
"""Times the prediction of chosen (user, item) pairs (cmfrec_amd.Scorer, cmfrec_hip_scorer_predict) against a model with random
factors of the flagship's shape: 358,858 users x 160,112 items, 10^7 uniformly random pairs, and the same pairs sorted by user.

    models     k = 50 in double precision, k = 64 in single precision; user and item biases, a global mean

One warm-up, then the median of `--runs` runs.  Reported per configuration and order:
    kernel_ms          HIP-event time of the scoring kernel (predict_kernels.hpp), summed over the blocks of a call
    wall_ms            Scorer.predict: the pairs up, the kernel, the predictions down
    gathered_TBps      n_pairs * (2 * kk * sizeof(T) + 8 + sizeof(T)) / kernel time -- two factor rows, two indices, one result
    vs_cached_gather   that rate over the 6.0 TB/s the project measured for cached row gathers
    numpy_wall_ms      CMF.predict on the same host for the same pairs: the NumPy gather and einsum a user ran before
Nothing is gated on these numbers.

    python tools/bench_predict.py               # every configuration, appended to profiles/predict/bench_predict.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("float64", 50), ("float32", 64)]
M, N, PAIRS = 358858, 160112, 10 ** 7
CACHED_GATHER_BYTES_PER_S = 6.0e12


def make_model(dtype, k):
    """A CMF that holds random factors and biases as if fitted."""
    import numpy as np
    from cmfrec_amd import CMF
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    mdl = CMF(k=k, lambda_=5., user_bias=True, item_bias=True, use_float=dt is np.float32)
    mdl.A_ = (0.1 * rng.standard_normal((M, k))).astype(dt)
    mdl.B_ = (0.1 * rng.standard_normal((N, k))).astype(dt)
    mdl.glob_mean_ = 3.1
    mdl.user_bias_ = (0.2 * rng.standard_normal(M)).astype(dt)
    mdl.item_bias_ = (0.2 * rng.standard_normal(N)).astype(dt)
    mdl.is_fitted_ = True
    return mdl


def worker(dtype, k, order, runs, warmup, n_pairs):
    import numpy as np
    sys.path.insert(0, ROOT)
    dt = np.dtype(dtype).type
    mdl = make_model(dtype, k)
    rng = np.random.default_rng(7)
    user = rng.integers(0, M, n_pairs).astype(np.int32); item = rng.integers(0, N, n_pairs).astype(np.int32)
    if order == "sorted":
        o = np.argsort(user, kind="stable")
        user, item = np.ascontiguousarray(user[o]), np.ascontiguousarray(item[o])
    wall, kern = [], []
    with mdl.scorer() as sc:
        for it in range(warmup + runs):
            s0 = time.perf_counter()
            out = sc.predict(user, item)
            s1 = time.perf_counter()
            if it >= warmup:
                wall.append((s1 - s0) * 1e3); kern.append(sc.kernel_ms())
    s0 = time.perf_counter()
    host = mdl.predict(user, item)
    numpy_ms = (time.perf_counter() - s0) * 1e3
    err = float(np.abs(out.astype(np.float64) - host.astype(np.float64)).max())
    assert err < (1e-10 if dt is np.float64 else 1e-3), err
    s = np.dtype(dt).itemsize
    med = lambda x: float(np.median(x))
    rate = n_pairs * (2 * k * s + 8 + s) / (med(kern) * 1e-3)
    print(json.dumps(dict(what="predict", dtype=dtype, k=k, order=order, m=M, n=N, n_pairs=n_pairs, runs=runs, warmup=warmup,
                          kernel_ms=round(med(kern), 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4),
                          wall_ms=round(med(wall), 2), gathered_TBps=round(rate / 1e12, 3),
                          vs_cached_gather=round(rate / CACHED_GATHER_BYTES_PER_S, 3), numpy_wall_ms=round(numpy_ms, 1),
                          max_abs_diff_to_numpy=err)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict", "bench_predict.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:50")
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "ORDER"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.worker[2], a.runs, a.warmup, a.pairs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), order] for dt, k in CONFIGS for order in ("random", "sorted") if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--runs", str(a.runs), "--warmup", str(a.warmup), "--pairs", str(a.pairs)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_predict: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
