"""Implicit ALS-CG beyond 64 factors at the benchmark's shape: the A-step, the B-step (HIP events around the half-steps,
AlsSession.kernel_time) and the iteration (host clock around the loop, ended by a synchronise), for a comparison build and for
this build at several CMFREC_HIP_CG_WIDE_MIN -- each configuration in a child process of its own, the configurations of a case
interleaved over the rounds so that drift and neighbours on the machine hit them alike.

    python tools/bench_implicit_cg_wide.py [--parent-libdir cmfrec_amd/lib_parent] [--out profiles/implicit_cg_wide] [--rounds 3]

--parent-libdir: a build of the parent commit (make -C cmfrec_amd/csrc OUTDIR=... in a checkout of it), loaded through
CMFREC_HIP_LIBDIR; left out, only this build is measured.  One JSON line per child in <out>/lines.jsonl, the table in <out>/table.txt:
per configuration the median over the rounds and the spread (max - min) / median; a configuration differs from the parent where the
medians differ by more than the larger of the two spreads."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(100, "float64"), (128, "float64"), (128, "float32")]
WIDE_MIN = [128, 256, 512, 1024]


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    from cmfrec_amd.session import AlsSession
    dtype = np.dtype(args.dtype).type
    m, n, nnz = (bench.M_USERS, bench.N_ITEMS, bench.NNZ) if args.scale >= 1 else (3000, 1500, 120000)
    row, col, val = bench.synth_block(m, n, nnz, seed=2)
    rng = np.random.default_rng(0)
    s = AlsSession(m, n, args.k, implicit=True, dtype=dtype, lam=5.0, use_cg=True, max_cg_steps=3)
    s.set_X_coo(row, col, val.astype(dtype))
    s.set_factors(A=(0.01 * rng.standard_normal((m, args.k))).astype(dtype), B=np.zeros((n, args.k), dtype))
    for _ in range(args.warmup):
        s.update("B"); s.update("A")
    s.sync(); s.reset_timers()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        s.update("B"); s.update("A")
    s.sync()
    it_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    (a_ms, a_n), (b_ms, b_n) = s.kernel_time("A"), s.kernel_time("B")
    wide = [s.cg_wide_rows(w) if hasattr(s.lib, "cmfrec_hip_session_cg_wide_rows") else None for w in (0, 1)]
    f = s.get_factors()
    print(json.dumps(dict(label=args.label, k=args.k, dtype=args.dtype, round=args.round, a_step_ms=a_ms / a_n, b_step_ms=b_ms / b_n,
                          iteration_ms=it_ms, wide_rows=wide, checksum=[float(np.abs(f["A"]).sum()), float(np.abs(f["B"]).sum())])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--k", type=int); ap.add_argument("--dtype"); ap.add_argument("--label"); ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="< 1: a toy shape, to rehearse the tool")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="0,1,2")
    ap.add_argument("--parent-libdir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "implicit_cg_wide"))
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    configs = [("this_min%d" % w, {"CMFREC_HIP_CG_WIDE_MIN": str(w)}) for w in WIDE_MIN]
    if args.parent_libdir:
        configs.insert(0, ("parent", {"CMFREC_HIP_LIBDIR": os.path.abspath(args.parent_libdir)}))
    lines = []
    with open(os.path.join(args.out, "lines.jsonl"), "a") as log:
        for ci in [int(c) for c in args.cases.split(",")]:
            k, dt = CASES[ci]
            for rnd in range(args.rounds):
                for label, env in configs:
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--k", str(k), "--dtype", dt, "--label", label, "--round", str(rnd),
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--scale", str(args.scale)]
                    out = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=args.timeout)
                    if out.returncode != 0:      # a child that fails ends the measurement: nothing more is started on the device
                        sys.exit("child %s k=%d %s failed (%d):\n%s" % (label, k, dt, out.returncode, out.stderr[-2000:]))
                    rec = json.loads(out.stdout.strip().splitlines()[-1])
                    lines.append(rec); log.write(json.dumps(rec) + "\n"); log.flush()
                    print(rec, flush=True)
    with open(os.path.join(args.out, "table.txt"), "a") as tab:
        for ci in [int(c) for c in args.cases.split(",")]:
            k, dt = CASES[ci]
            tab.write("k = %d, %s: median ms over %d rounds (spread = (max - min) / median)\n" % (k, dt, args.rounds))
            for label, _ in configs:
                rs = [r for r in lines if r["label"] == label and r["k"] == k and r["dtype"] == dt]
                cell = lambda key: "%8.2f (%4.1f %%)" % (statistics.median(r[key] for r in rs),
                                                        100 * (max(r[key] for r in rs) - min(r[key] for r in rs)) / statistics.median(r[key] for r in rs))
                tab.write("  %-14s A-step %s  B-step %s  iteration %s  rows on the Gramian CG (A, B) %s\n" %
                          (label, cell("a_step_ms"), cell("b_step_ms"), cell("iteration_ms"), rs[0]["wide_rows"]))
    print(open(os.path.join(args.out, "table.txt")).read())


if __name__ == "__main__":
    main()
