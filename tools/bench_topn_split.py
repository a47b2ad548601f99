#!/usr/bin/env python3
"""Times the full ranking of a FEW users with the items cut into slices (Ranker(split=...)) against the
unsplit route on the same ranker in the same run: n = 160,112 items, nu = 1 .. 4096 users, k = 50 / 128 / 256 in double and 272
in single precision, n_top = 10 and 128.

    python tools/bench_topn_split.py                # every configuration, appended to profiles/topn_split/bench_topn_split.jsonl
    python tools/bench_topn_split.py --e2e          # plus model.topN(user) / model.topN_warm(...) per request, end to end
    python tools/bench_topn_split.py --trace        # plus the two kernels' own times (rocprofv3 --kernel-trace --stats): the merge's share

Per point and route: 2 warm-up calls, then 3 repetitions of 5 calls; a repetition's figure is the median HIP-event time of its
calls (cmfrec_hip_ranker_kernel_ms: the slice pass and the merge).  `ms` is the median of the three, `spread_ms` their range;
`wall_ms` the median wall time of a call (uploads, launch, download).  Routes: "unsplit" (split=None, the code path of a ranker
that never heard of the setting -- the yardstick), "auto" (the planner), and forced slice counts around the planner's choice.
`auto_wins` on an "auto" line: it chose more than one slice and its time is below the unsplit time by more than both spreads.

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 160112
CONFIGS = [("float64", 50), ("float64", 128), ("float64", 256), ("float32", 272)]
NTOPS = (10, 128)
USERS = (1, 4, 16, 64, 256, 1024, 4096)
REPS, CALLS, WARMUP = 3, 5, 2


def measure(rk, A, n_top, split):
    import numpy as np
    rk.split = split
    for _ in range(WARMUP):
        rk.topN(A, n=n_top)
    reps, wall = [], []
    for _ in range(REPS):
        ms = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            rk.topN(A, n=n_top)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(rk.kernel_ms())
        reps.append(float(np.median(ms)))
    users, groups = rk.launch_shape()
    return dict(ms=round(float(np.median(reps)), 4), reps_ms=[round(x, 4) for x in reps], spread_ms=round(max(reps) - min(reps), 4),
                wall_ms=round(float(np.median(wall)), 4), slices=rk.slices(), users_per_workgroup=users, workgroups=groups)


def worker(dtype, k, n, users, forced):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    os.environ.pop("CMFREC_HIP_TOPN", None)
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    B = rng.standard_normal((n, k)).astype(dt)
    Aall = rng.standard_normal((max(users), k)).astype(dt)
    with Ranker(B) as rk:
        for n_top in NTOPS:
            for nu in users:
                A = Aall[:nu]
                base = dict(dtype=dtype, k=k, n=n, n_top=n_top, nu=nu)
                un = measure(rk, A, n_top, None)
                print(json.dumps(dict(base, route="unsplit", **un)), flush=True)
                au = measure(rk, A, n_top, "auto")
                wins = au["slices"] > 1 and au["ms"] + au["spread_ms"] + un["spread_ms"] < un["ms"]
                print(json.dumps(dict(base, route="auto", speedup=round(un["ms"] / au["ms"], 3), auto_wins=bool(wins), **au)), flush=True)
                s = au["slices"]
                around = sorted({max(2, s // 4), max(2, s // 2), s * 2, s * 4} | set(forced))
                done = {1, s}
                for f in around:
                    r = measure(rk, A, n_top, f)
                    if r["slices"] in done:
                        continue
                    done.add(r["slices"])
                    print(json.dumps(dict(base, route="forced", asked=f, speedup=round(un["ms"] / r["ms"], 3), **r)), flush=True)


def e2e_worker(n, k, use_float):
    """model.topN(user) and model.topN_warm(...) per request on a CMF_implicit fitted on n items; the one-row solve's part (HIP
    events of NewUsers.kernel_ms) beside the ranking's."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import CMF_implicit
    m, nnz = 2000, 400000
    rng = np.random.default_rng(0)
    lin = rng.choice(m * n, size=nnz, replace=False)
    row, col = (lin // n).astype(np.int32), (lin % n).astype(np.int32)
    val = np.ceil(rng.lognormal(1, 1, nnz))
    mdl = CMF_implicit(k=k, lambda_=5., niter=1, use_float=use_float, nthreads=1).fit((row, col, val), shape=(m, n))
    xc = np.sort(rng.choice(n, 60, replace=False)); xv = np.ceil(rng.lognormal(1, 1, 60))
    out = dict(what="one_user_end_to_end", dtype="float32" if use_float else "float64", k=k, n=n, n_top=10, x_entries=60)
    for name, call in (("topN", lambda: mdl.topN(7, 10)), ("topN_warm", lambda: mdl.topN_warm(10, X_col=xc, X_val=xv)),
                       ("topN_batch_one", lambda: mdl.topN_batch([7], 10)),
                       ("topN_new_batch_one", lambda: mdl.topN_new_batch(X=(np.zeros(60, np.int32), xc, xv), n=10, exclude_seen=False))):
        reps = 60 if name in ("topN", "topN_warm") else 5
        for _ in range(3):
            call()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter(); call(); t.append((time.perf_counter() - t0) * 1e6)
        out[name + "_us"] = round(float(np.median(t)), 1)
    out["topN_kernel_us"] = round(mdl._one_user_ranker.kernel_ms() * 1e3, 1)
    out["topN_slices"] = mdl._one_user_ranker.slices()
    solve, rank = mdl._one_user_new.kernel_ms()
    out["topN_warm_solve_us"] = round(solve * 1e3, 1); out["topN_warm_rank_us"] = round(rank * 1e3, 1)
    print(json.dumps(out), flush=True)


def trace_worker(dtype, k, n, n_top, nu):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    B = rng.standard_normal((n, k)).astype(dt); A = rng.standard_normal((nu, k)).astype(dt)
    with Ranker(B, split="auto") as rk:
        for _ in range(20):
            rk.topN(A, n=n_top)


def trace(dtype, k, n, n_top, nu, outdir, timeout):
    """The slice pass's and the merge's own times: the trace worker alone under rocprofv3 --kernel-trace --stats."""
    d = os.path.join(outdir, "trace_%s_k%d_top%d_nu%d" % (dtype, k, n_top, nu))
    cmd = ["timeout", "-k", "10", str(timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "split", "--",
           sys.executable, os.path.abspath(__file__), "--n", str(n), "--trace-worker", dtype, str(k), str(n_top), str(nu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        return r.returncode, None
    t = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(f)):
            name = rec.get("Name", "")
            for key in ("topn_split_kernel", "topn_split_merge_kernel"):
                if key + "<" in name or name.startswith(key):
                    t[key] = t.get(key, 0.0) + float(rec.get("AverageNs") or 0) / 1e3
    row = dict(what="kernel_events", dtype=dtype, k=k, n=n, n_top=n_top, nu=nu, slice_pass_us=round(t.get("topn_split_kernel", 0.0), 2),
               merge_us=round(t.get("topn_split_merge_kernel", 0.0), 2))
    tot = row["slice_pass_us"] + row["merge_us"]
    row["merge_share"] = round(row["merge_us"] / tot, 4) if tot else None
    return 0, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_split", "bench_topn_split.jsonl"))
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--users", default=",".join(str(u) for u in USERS))
    ap.add_argument("--forced", default="", help="further slice counts to time at every point, comma separated")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:128")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--worker", nargs=2, metavar=("DTYPE", "K"))
    ap.add_argument("--e2e-worker", nargs=2, metavar=("K", "USE_FLOAT"))
    ap.add_argument("--trace-worker", nargs=4, metavar=("DTYPE", "K", "NTOP", "NU"))
    a = ap.parse_args()
    users = [int(u) for u in a.users.split(",") if u]
    forced = [int(f) for f in a.forced.split(",") if f]
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.n, users, forced)
    if a.e2e_worker:
        return e2e_worker(a.n, int(a.e2e_worker[0]), bool(int(a.e2e_worker[1])))
    if a.trace_worker:
        return trace_worker(a.trace_worker[0], int(a.trace_worker[1]), a.n, int(a.trace_worker[2]), int(a.trace_worker[3]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k)] for dt, k in CONFIGS if a.only in (None, "%s:%d" % (dt, k))]
    if a.e2e:
        steps += [["--e2e-worker", "50", "0"], ["--e2e-worker", "128", "0"]]
    common = ["--n", str(a.n), "--users", a.users, "--forced", a.forced]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            f.write(r.stdout); f.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_topn_split: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
        if a.trace:
            for dt, k, n_top, nu in (("float64", 128, 10, 1), ("float64", 128, 128, 1), ("float64", 128, 128, 64), ("float32", 272, 128, 1)):
                rc, row = trace(dt, k, a.n, n_top, nu, os.path.dirname(a.out), a.timeout)
                if rc != 0:
                    sys.stderr.write("\nbench_topn_split: the trace ended with status %d; stopping\n" % rc)
                    return rc
                line = json.dumps(row) + "\n"
                sys.stdout.write(line); sys.stdout.flush(); f.write(line); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
