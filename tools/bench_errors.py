#!/usr/bin/env python3
"""Times the error reduction on a resident held-out set (cmfrec_amd.EvalSet, Scorer.errors, AlsSession.errors) beside the path
it replaces, on the workload of tools/bench_predict.py: 358,858 users x 160,112 items, 10^7 uniformly random pairs with a value
each, as they come ("random") and reordered by user by EvalSet(sort=True) ("sorted").

    models     k = 50 in double precision, k = 64 in single precision; user and item biases, a global mean

One warm-up, then the median of `--runs` runs with the minimum and the maximum.  Per configuration and order:
    errors_kernel_ms    HIP-event time of score_errors_kernel + reduce_error_partials (EvalSet.kernel_ms)
    predict_kernel_ms   HIP-event time of the scoring kernel of Scorer.predict on the same pairs in the same order, same run
    errors_wall_ms      Scorer.errors on the resident set: two kernels, one record down
    predict_wall_ms     Scorer.predict (pairs up, kernel, predictions down) + the NumPy reduction of the same five sums
    upload_ms           EvalSet(...) itself, once: the sort on the host and the four arrays up
and one line "session": a resident AlsSession of the benchmark's shape (bench.py: the implicit model, k = 50, double precision,
17.3 M entries), milliseconds per iteration beside milliseconds per AlsSession.errors call on the resident set.
The base of every comparison is the prediction path (Scorer.predict and its scoring kernel) of the build the tool runs on, never
the error kernels against themselves.  That scoring kernel shares its loop with the error kernel since the latter exists, so it
is this commit's code, not its parent's: set its times beside the parent's own figures (profiles/predict/) before
reading a ratio -- DESIGN.md 3.11 does -- or run the tool on a parent build kept beside this one (CMFREC_HIP_LIBDIR) for the
predict columns.  Nothing is gated on these numbers.

    python tools/bench_errors.py               # every configuration, appended to profiles/errors/bench_errors.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CONFIGS = [("float64", 50), ("float32", 64)]
PAIRS = 10 ** 7


def _stats(name, v):
    import numpy as np
    return {name: round(float(np.median(v)), 4), name + "_min": round(min(v), 4), name + "_max": round(max(v), 4)}


def worker(dtype, k, order, runs, warmup, n_pairs):
    import numpy as np
    from bench_predict import M, N, make_model
    from cmfrec_amd import EvalSet
    from cmfrec_amd.metrics import error_metrics
    dt = np.dtype(dtype).type
    mdl = make_model(dtype, k)
    rng = np.random.default_rng(7)
    user = rng.integers(0, M, n_pairs).astype(np.int32); item = rng.integers(0, N, n_pairs).astype(np.int32)
    x = (3.1 + rng.standard_normal(n_pairs)).astype(dt)
    s0 = time.perf_counter()
    es = EvalSet(user, item, x, dtype=dt, sort=order == "sorted")
    upload_ms = (time.perf_counter() - s0) * 1e3
    if order == "sorted":
        o = np.argsort(user, kind="stable")
        user, item, x = np.ascontiguousarray(user[o]), np.ascontiguousarray(item[o]), np.ascontiguousarray(x[o])
    ew, ek, pw, pk = [], [], [], []
    with es, mdl.scorer() as sc:
        for it in range(warmup + runs):
            s0 = time.perf_counter()
            rec = sc.errors(es)
            s1 = time.perf_counter()
            p = sc.predict(user, item)
            e = p.astype(np.float64) - x
            host = dict(n=len(e), sum_we=e.sum(), sum_wabs=np.abs(e).sum(), sum_wsq=np.dot(e, e), max_abs=np.abs(e).max())
            s2 = time.perf_counter()
            if it >= warmup:
                ew.append((s1 - s0) * 1e3); ek.append(es.kernel_ms()); pw.append((s2 - s1) * 1e3); pk.append(sc.kernel_ms())
    got = error_metrics(rec)
    rmse_host = float(np.sqrt(host["sum_wsq"] / host["n"]))
    assert int(rec["n"][0]) == n_pairs and rec["max_abs"][0] == host["max_abs"], (rec, host)
    assert abs(got["rmse"] - rmse_host) < 1e-9 * rmse_host, (got["rmse"], rmse_host)
    line = dict(what="errors", dtype=dtype, k=k, order=order, m=M, n=N, n_pairs=n_pairs, runs=runs, warmup=warmup, upload_ms=round(upload_ms, 1),
                rmse=got["rmse"])
    for name, v in (("errors_kernel_ms", ek), ("predict_kernel_ms", pk), ("errors_wall_ms", ew), ("predict_wall_ms", pw)):
        line.update(_stats(name, v))
    line["kernel_ratio"] = round(line["errors_kernel_ms"] / line["predict_kernel_ms"], 3)
    line["wall_ratio"] = round(line["errors_wall_ms"] / line["predict_wall_ms"], 4)
    print(json.dumps(line), flush=True)


def session_worker(runs, warmup, n_pairs, scale):
    import numpy as np
    import bench
    from cmfrec_amd import AlsSession, EvalSet
    m, n, nnz, k = int(bench.M_USERS * scale), int(bench.N_ITEMS * scale), int(bench.NNZ * scale), bench.K
    row, col, val = bench.synth_block(m, n, nnz, seed=2)
    rng = np.random.default_rng(7)
    user = rng.integers(0, m, n_pairs).astype(np.int32); item = rng.integers(0, n, n_pairs).astype(np.int32)
    x = rng.integers(0, 2, n_pairs).astype(np.float64)
    sess = AlsSession(m, n, k, implicit=True, dtype=np.float64, lam=bench.LAM, use_cg=True, max_cg_steps=bench.MAX_CG_STEPS)
    sess.set_X(bench.to_csr(row, col, val, m), bench.to_csr(col, row, val, n))
    sess.set_factors(A=np.random.default_rng(100).random((m, k)) * 2.0 ** -7, B=np.zeros((n, k)))
    it_ms, ev_ms, ev_kernel, curve = [], [], [], []
    with EvalSet(user, item, x, sort=True) as es:
        for it in range(warmup + runs):
            s0 = time.perf_counter()
            sess.iterate(1, False); sess.sync()
            s1 = time.perf_counter()
            rec = sess.errors(es)
            s2 = time.perf_counter()
            curve.append(float(np.sqrt(rec["sum_wsq"][0] / rec["sum_w"][0])))
            if it >= warmup:
                it_ms.append((s1 - s0) * 1e3); ev_ms.append((s2 - s1) * 1e3); ev_kernel.append(es.kernel_ms())
    sess.close()
    line = dict(what="session", dtype="float64", k=k, m=m, n=n, nnz=nnz, n_pairs=n_pairs, order="sorted", runs=runs, warmup=warmup,
                rmse_curve=[round(v, 6) for v in curve])
    for name, v in (("iteration_ms", it_ms), ("errors_call_ms", ev_ms), ("errors_kernel_ms", ev_kernel)):
        line.update(_stats(name, v))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "errors", "bench_errors.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the session's workload (debug only)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:50, or 'session'")
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "ORDER"))
    ap.add_argument("--session-worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.worker[2], a.runs, a.warmup, a.pairs)
    if a.session_worker:
        return session_worker(a.runs, a.warmup, a.pairs, a.scale)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), order] for dt, k in CONFIGS for order in ("random", "sorted") if a.only in (None, "%s:%d" % (dt, k))]
    if a.only in (None, "session"):
        steps.append(["--session-worker", "--scale", str(a.scale)])
    common = ["--runs", str(a.runs), "--warmup", str(a.warmup), "--pairs", str(a.pairs)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_errors: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
