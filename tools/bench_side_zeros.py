#!/usr/bin/env python3
"""Times one ALS iteration of the implicit model with sparse side information whose absent entries are zeros (NA_as_zero_user) on
its two routes: the zero-filled dense matrix (up to CMFREC_HIP_ZEROFILL_MAX_GB) and the triplets themselves (beyond it;
cmfrec_amd/csrc/side_zeros_kernels.hpp).  Synthetic model at the C2 shape of bench.py (358,858 x 160,112, 17.3 M entries, k = 50,
double precision, CG), 16 attributes per user (one flag nearly every user carries, the others 1 / rank^0.8), k_user = 0.

    python tools/bench_side_zeros.py                 # p = 2,000 both routes, p = 20,000 sparse route beside the plain model
    python tools/bench_side_zeros.py --trace         # plus the kernels' event times from rocprofv3 --kernel-trace --stats

The routes are timed as the two sessions a fit creates on either side of the limit (cmfrec_hip_session_set_sideinfo on the
zero-filled centred matrix / cmfrec_hip_session_set_sideinfo_sparse_zeros), alive in ONE process and advanced in turn, iteration by
iteration: 3 warm-up and 10 timed iterations each, every one ended by a device synchronise; median and min - max.  Each
measurement runs in a child process of its own under `timeout`; the first that fails ends the run.  JSON lines are appended to
profiles/side_zeros/bench_side_zeros.jsonl.

Bytes per product, from the shapes: nnz_U (sizeof(real_t) + 4) for the triplets, nnz_U kc sizeof(real_t) for the gathered rows of M
(p x kc: cache-resident) / F (rows x kc), and the output; the column-sum pass of the attribute side reads F once more."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
ATTRS_PER_USER = 16


def synth_side(m, p, seed):
    """Triplets of [m, p]: attribute 0 for 95 % of the rows, 15 more per row drawn 1 / rank^0.8 (a repeated draw adds up)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, p) ** 0.8
    cdf = np.cumsum(w / w.sum())
    rest = 1 + np.minimum(np.searchsorted(cdf, rng.random(m * (ATTRS_PER_USER - 1))), p - 2)
    flag = np.nonzero(rng.random(m) < 0.95)[0]
    row = np.concatenate([np.repeat(np.arange(m), ATTRS_PER_USER - 1), flag]).astype(np.int32)
    col = np.concatenate([rest, np.zeros(len(flag), np.int64)]).astype(np.int32)
    perm = rng.permutation(len(row))
    return row[perm], col[perm], np.ones(len(row))


def make_sessions(p, routes, m, n, nnz, k):
    import numpy as np
    sys.path.insert(0, ROOT)
    from bench import synth_block, LAM, MAX_CG_STEPS
    from cmfrec_amd.session import AlsSession
    row, col, val = synth_block(m, n, nnz, 0)
    rng = np.random.default_rng(1)
    A0 = rng.standard_normal((m, k)) * 0.01
    ur, uc, uv = synth_side(m, p, 2) if p else (None, None, None)
    mu = np.bincount(uc, weights=uv, minlength=p) / m if p else None
    out = {}
    for route in routes:
        side = dict(p=p, m_u=m) if route != "plain" else {}
        s = AlsSession(m, n, k, True, np.float64, lam=LAM, use_cg=True, max_cg_steps=MAX_CG_STEPS, **side)
        s.set_X_coo(row, col, val)
        if route == "dense":
            U = np.zeros((m, p)); np.add.at(U, (ur, uc), uv); U -= mu[None, :]
            s.set_sideinfo(U=U); del U
        elif route == "sparse":
            s.set_sideinfo_sparse_zeros("U", ur, uc, uv, colmeans=mu)
        s.set_factors(A=A0, B=np.zeros((n, k)), Cm=np.zeros((p, k)) if route != "plain" else None)
        out[route] = s
    return out, (0 if not p else len(uv))


def worker(p, routes, m, n, nnz, k, runs, warmup):
    import numpy as np
    sessions, nnz_u = make_sessions(p, routes, m, n, nnz, k)
    ms = {r: [] for r in routes}
    for it in range(warmup + runs):
        for route in routes:                      # the routes in turn, iteration by iteration
            s = sessions[route]
            s.sync()
            t0 = time.perf_counter()
            s.iterate(1)
            s.sync()
            if it >= warmup:
                ms[route].append((time.perf_counter() - t0) * 1e3)
    # the two products of one iteration: U~^T A (C update) and U~ C (right-hand sides of the A-step)
    sz = 8
    by_rows = nnz_u * (sz + 4) + nnz_u * k * sz + m * k * sz
    by_cols = nnz_u * (sz + 4) + nnz_u * k * sz + p * k * sz + m * k * sz
    for route in routes:
        print(json.dumps(dict(what="iteration", route=route, dtype="float64", m=m, n=n, nnz=nnz, k=k, p=p, nnz_U=nnz_u,
                              ms_median=round(float(np.median(ms[route])), 4), ms_min=round(min(ms[route]), 4),
                              ms_max=round(max(ms[route]), 4), runs=runs, warmup=warmup,
                              bytes_row_product=by_rows, bytes_attribute_product=by_cols,
                              dense_gemm_flop_each=2.0 * m * p * k)), flush=True)
    for s in sessions.values():
        s.close()


def trace(p, route, a, outdir):
    """Event times of one route's kernels: this tool's worker alone under rocprofv3 --kernel-trace --stats, nothing else traced."""
    d = os.path.join(outdir, "trace_p%d_%s" % (p, route))
    cmd = ["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "sz", "--",
           sys.executable, os.path.abspath(__file__), "--worker", str(p), route] + common_args(a)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        return r.returncode, []
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(f)):
            name = rec.get("Name", "")
            if "sz_" in name or "gemm_mfma_kernel" in name:
                rows.append(dict(what="kernel_events", route=route, p=p, kernel=name.split("(")[0][:120], calls=rec.get("Calls"),
                                 total_ns=rec.get("TotalDurationNs"), average_ns=rec.get("AverageNs"), min_ns=rec.get("MinNs"),
                                 max_ns=rec.get("MaxNs")))
    return 0, rows


def common_args(a):
    return ["--m", str(a.m), "--n", str(a.n), "--nnz", str(a.nnz), "--k", str(a.k), "--runs", str(a.runs), "--warmup", str(a.warmup)]


def main():
    sys.path.insert(0, ROOT)
    from bench import M_USERS, N_ITEMS, NNZ, K
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "side_zeros", "bench_side_zeros.jsonl"))
    ap.add_argument("--m", type=int, default=M_USERS)
    ap.add_argument("--n", type=int, default=N_ITEMS)
    ap.add_argument("--nnz", type=int, default=NNZ)
    ap.add_argument("--k", type=int, default=K)
    ap.add_argument("--p-both", type=int, default=2000, help="attributes where both routes run")
    ap.add_argument("--p-sparse", type=int, default=20000, help="attributes where the dense route is out of reach")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per measurement")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--worker", nargs=2, metavar=("P", "ROUTES"))
    a = ap.parse_args()
    if a.worker:
        return worker(int(a.worker[0]), a.worker[1].split(","), a.m, a.n, a.nnz, a.k, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [(a.p_both, "dense,sparse"), (a.p_sparse, "sparse,plain")]
    with open(a.out, "a") as f:
        for p, routes in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", str(p), routes] + common_args(a)
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_side_zeros: p = %d ended with status %d; stopping\n" % (p, r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
        if a.trace:
            for route in ("dense", "sparse"):
                rc, rows = trace(a.p_both, route, a, os.path.dirname(a.out))
                if rc != 0:
                    sys.stderr.write("\nbench_side_zeros: the trace of the %s route ended with status %d; stopping\n" % (route, rc))
                    return rc
                for rec in rows:
                    line = json.dumps(rec)
                    print(line, flush=True); f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
