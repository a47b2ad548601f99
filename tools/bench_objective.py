#!/usr/bin/env python3
"""Times one evaluation of the training objective (AlsSession.objective: cmfrec_hip_session_objective) beside one ALS iteration of
the same resident session in the same process, on the benchmark's shape (bench.py: the implicit model on 358,858 x 160,112 with
17.3 M entries):

    float64 k = 50     the benchmark's own configuration
    float32 k = 128

Both are timed with HIP events recorded on the session's stream (the objective call ends with the download of its record, the
iteration with a synchronise), after `--warmup` rounds, `--runs` times, alternating; the median with the minimum and the maximum.
    objective_ms, iteration_ms
    gather_bytes        the bytes one gather pass needs: per entry its index, its value and one opposing row of k values, plus the
                        rows of A and B once and the two indptr arrays
    implied_gbps        gather_bytes / objective_ms -- the whole call (work items, row pass, both Gramians, reduction) over the
                        bytes of the row pass alone, so a lower bound of what the row kernel achieves
Nothing is gated on these numbers.

    python tools/bench_objective.py            # both configurations, appended to profiles/objective/bench_objective.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [("float64", 50), ("float32", 128)]


def worker(dtype, k, runs, warmup, scale):
    import numpy as np
    import torch
    import bench
    from cmfrec_amd import AlsSession
    from cmfrec_amd.metrics import objective_from_record
    dt = np.dtype(dtype).type
    m, n, nnz = int(bench.M_USERS * scale), int(bench.N_ITEMS * scale), int(bench.NNZ * scale)
    row, col, val = bench.synth_block(m, n, nnz, seed=2)
    sess = AlsSession(m, n, k, implicit=True, dtype=dt, lam=bench.LAM, use_cg=True, max_cg_steps=bench.MAX_CG_STEPS)
    sess.set_X(bench.to_csr(row, col, val.astype(dt), m), bench.to_csr(col, row, val.astype(dt), n))
    sess.set_factors(A=(np.random.default_rng(100).random((m, k)) * 2.0 ** -7).astype(dt), B=np.zeros((n, k), dt))
    stream = torch.cuda.ExternalStream(sess.stream())

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    it_ms, ob_ms, curve = [], [], []
    for r in range(warmup + runs):
        t_it, _ = timed(lambda: sess.iterate(1, False))
        t_ob, rec = timed(sess.objective)
        curve.append(objective_from_record(rec, lambda_=bench.LAM))
        if r >= warmup:
            it_ms.append(t_it); ob_ms.append(t_ob)
    sess.close()
    size = np.dtype(dt).itemsize
    gather_bytes = len(val) * (4 + size + k * size) + (m + n) * k * size + (m + n + 2) * 8
    line = dict(what="objective", dtype=dtype, k=k, m=m, n=n, nnz=int(len(val)), runs=runs, warmup=warmup, gather_bytes=int(gather_bytes),
                objective_curve=[float("%.9g" % v) for v in curve])
    for name, v in (("objective_ms", ob_ms), ("iteration_ms", it_ms)):
        line.update({name: round(float(np.median(v)), 4), name + "_min": round(min(v), 4), name + "_max": round(max(v), 4)})
    line["objective_over_iteration"] = round(line["objective_ms"] / line["iteration_ms"], 4)
    line["implied_gbps"] = round(gather_bytes / (line["objective_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective", "bench_objective.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workload (debug only)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--worker", nargs=2, metavar=("DTYPE", "K"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.runs, a.warmup, a.scale)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for dt, k in CONFIGS:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--warmup",
                   str(a.warmup), "--scale", str(a.scale), "--worker", dt, str(k)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_objective: %s k=%d ended with status %d; stopping\n" % (dt, k, r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
