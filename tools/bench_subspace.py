"""The subspace half-step against the Cholesky and CG routes at the benchmark's shape, implicit model, one session
per case:

  1. kernel time of one iteration (HIP events around the two half-steps, AlsSession.kernel_time) of each route -- subspace with one
     sweep, Cholesky, CG with max_cg_steps = 3 -- the routes alternating in one process from the same start values; median of
     --reps with minimum and maximum;
  2. objective against cumulative kernel time over --iters iterations of each route from the same start (one sweep is not one
     exact solve, so time per iteration alone does not rank the routes).

    python tools/bench_subspace.py [--cases 0,1,2,3,4] [--out profiles/subspace] [--scale 1]

One JSON line per case in <out>/lines.jsonl, the two tables in <out>/table.txt; both are written anew by every run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(64, "float64"), (128, "float64"), (256, "float64"), (128, "float32"), (256, "float32")]
ROUTES = ("subspace", "cholesky", "cg")


def iteration(s, route):
    """One iteration of `route`; returns its kernel time in ms (A-step + B-step)."""
    s.set_subspace(16 if route == "subspace" else 0, 1)
    s.sync(); s.reset_timers()
    s.update("B", use_cholesky=route == "cholesky"); s.update("A", use_cholesky=route == "cholesky")
    s.sync()
    return s.kernel_time("A")[0] + s.kernel_time("B")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1,2,3,4")
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="< 1: a toy shape, to rehearse the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subspace"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    from cmfrec_amd import AlsSession, metrics
    os.makedirs(args.out, exist_ok=True)
    for name in ("lines.jsonl", "table.txt"):                 # a run replaces the output of the one before it
        open(os.path.join(args.out, name), "w").close()
    m, n, nnz = (bench.M_USERS, bench.N_ITEMS, bench.NNZ) if args.scale >= 1 else (3000, 1500, 120000)
    row, col, val = bench.synth_block(m, n, nnz, seed=2)
    lam = 5.0
    for ci in [int(c) for c in args.cases.split(",")]:
        k, dt = CASES[ci]
        dtype = np.dtype(dt).type
        rng = np.random.default_rng(0)
        A0, B0 = (0.01 * rng.standard_normal((m, k))).astype(dtype), (0.01 * rng.standard_normal((n, k))).astype(dtype)
        s = AlsSession(m, n, k, implicit=True, dtype=dtype, lam=lam, use_cg=True, max_cg_steps=3)
        s.set_X_coo(row, col, val.astype(dtype))
        s.set_factors(A0, B0)
        for route in ROUTES:                                  # warm-up: every route once
            iteration(s, route)
        times = {r: [] for r in ROUTES}
        for _ in range(args.reps):
            for route in ROUTES:
                s.set_factors(A0, B0)
                times[route].append(iteration(s, route))
        curves = {}
        for route in ROUTES:
            s.set_factors(A0, B0)
            t, curve = 0.0, []
            for _ in range(args.iters):
                t += iteration(s, route)
                curve.append((t, metrics.objective_from_record(s.objective(), lam)))
            curves[route] = curve
        s.close()
        rec = dict(k=k, dtype=dt, m=m, n=n, nnz=nnz, reps=args.reps,
                   iteration_ms={r: dict(median=statistics.median(v), min=min(v), max=max(v)) for r, v in times.items()}, curves=curves)
        with open(os.path.join(args.out, "lines.jsonl"), "a") as log:
            log.write(json.dumps(rec) + "\n")
        with open(os.path.join(args.out, "table.txt"), "a") as tab:
            tab.write("k = %d, %s: kernel ms per iteration, median of %d (min .. max)\n" % (k, dt, args.reps))
            for r in ROUTES:
                v = rec["iteration_ms"][r]
                tab.write("  %-9s %9.2f (%.2f .. %.2f)\n" % (r, v["median"], v["min"], v["max"]))
            tab.write("  objective after each of %d iterations (cumulative ms: objective)\n" % args.iters)
            for r in ROUTES:
                tab.write("  %-9s %s\n" % (r, "  ".join("%.1f: %.8g" % c for c in curves[r])))
        print(json.dumps(rec["iteration_ms"]), flush=True)


if __name__ == "__main__":
    main()
