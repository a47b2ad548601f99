#!/usr/bin/env python3
"""Times validation while fitting (fit(..., validation=), cmfrec_hip_fit_set_monitor) on bench.py's C2 shape: the implicit
model, 358,858 users x 160,112 items, 17.3 M entries, k = 50, double precision, three CG steps.  1 % of the entries are held out
(their value in the set is 1: the implicit model predicts a preference) and the fit runs on the rest.

    session   on a resident AlsSession: milliseconds per iteration, per AlsSession.errors call on the held-out set and per
              AlsSession.ranking call (NDCG@10 and its kin) on 16,384 of the users with held-out items, their training items
              excluded (what the monitor adds to an evaluated iteration), per snapshot() and per restore() (device-to-device
              copies of A and B, synchronised for the measurement; the monitor itself does not wait for them)
    fit       CMF_implicit.fit end to end with `--niter` and with three times as many iterations: plain, watched by RMSE after every
              iteration without a snapshot (restore_best=False), with restore_best=True (a snapshot at every improvement), and
              watched by NDCG@10 on the 16,384 users.
              The two iteration counts split each fit's time into a fixed part (upload and conversion of X; with a watch also
              the set's sort and upload and the monitor's checks) and a part per iteration, as a user meets them

One warm-up, then the median of `--runs` runs with the minimum and the maximum.  Nothing is gated on these numbers.

    python tools/bench_fit_validation.py       # appended to profiles/fit_validation/bench_fit_validation.jsonl

Every part runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is started on a
device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HELD_OUT = 0.01
RANK_USERS = 16384


def _stats(name, v):
    import numpy as np
    return {name: round(float(np.median(v)), 4), name + "_min": round(min(v), 4), name + "_max": round(max(v), 4)}


def _problem(scale):
    import numpy as np
    import bench
    m, n, nnz = int(bench.M_USERS * scale), int(bench.N_ITEMS * scale), int(bench.NNZ * scale)
    row, col, val = bench.synth_block(m, n, nnz, seed=2)
    held = np.random.default_rng(7).random(len(val)) < HELD_OUT
    tr = ~held
    train = (np.ascontiguousarray(row[tr]), np.ascontiguousarray(col[tr]), np.ascontiguousarray(val[tr]))
    heldout = (np.ascontiguousarray(row[held]), np.ascontiguousarray(col[held]), np.ones(int(held.sum())))
    return m, n, bench.K, train, heldout


def _rank_users(heldout, scale):
    """The users of the ranking watch: RANK_USERS of those with held-out items, seeded."""
    import numpy as np
    have = np.unique(heldout[0])
    return np.sort(np.random.default_rng(11).choice(have, size=min(len(have), max(1, int(RANK_USERS * scale))), replace=False))


def session_worker(runs, warmup, scale):
    import numpy as np
    import bench
    from cmfrec_amd import AlsSession, EvalSet
    m, n, k, (row, col, val), (hr, hc, hx) = _problem(scale)
    sess = AlsSession(m, n, k, implicit=True, dtype=np.float64, lam=bench.LAM, use_cg=True, max_cg_steps=bench.MAX_CG_STEPS)
    sess.set_X(bench.to_csr(row, col, val, m), bench.to_csr(col, row, val, n))
    sess.set_factors(A=np.random.default_rng(100).random((m, k)) * 2.0 ** -7, B=np.zeros((n, k)))
    import scipy.sparse as sp
    from cmfrec_amd import RankSet
    ru = _rank_users((hr, hc, hx), scale)
    held_csr = sp.csr_matrix((np.ones(len(hr), np.int8), (hr, hc)), shape=(m, n))[ru]
    train_csr = sp.csr_matrix((np.ones(len(row), np.int8), (row, col)), shape=(m, n))[ru]
    train_csr.sort_indices()
    it_ms, ev_ms, ev_kernel, snap_ms, rest_ms, rank_ms, curve, ndcg = [], [], [], [], [], [], [], []
    with EvalSet(hr, hc, hx, sort=True) as es, RankSet(ru, held_csr, train_csr) as rs:
        for it in range(warmup + runs):
            t = [time.perf_counter()]
            sess.iterate(1, False); sess.sync(); t.append(time.perf_counter())
            rec = sess.errors(es); t.append(time.perf_counter())
            sess.snapshot(); sess.sync(); t.append(time.perf_counter())
            sess.restore(); sess.sync(); t.append(time.perf_counter())
            rk = sess.ranking(rs, 10); t.append(time.perf_counter())
            ndcg.append(float(rk["sum"][4] / rk["count"][4]))
            curve.append(float(np.sqrt(rec["sum_wsq"][0] / rec["sum_w"][0])))
            if it >= warmup:
                d = [(b - a) * 1e3 for a, b in zip(t, t[1:])]
                it_ms.append(d[0]); ev_ms.append(d[1]); ev_kernel.append(es.kernel_ms()); snap_ms.append(d[2]); rest_ms.append(d[3]); rank_ms.append(d[4])
    sess.close()
    line = dict(what="session", dtype="float64", k=k, m=m, n=n, nnz=len(val), n_heldout=len(hx), runs=runs, warmup=warmup,
                snapshot_bytes=(m + n) * k * 8, rank_users=len(ru), rank_heldout=int(held_csr.nnz), rmse_curve=[round(v, 6) for v in curve],
                ndcg_curve=[round(v, 6) for v in ndcg])
    for name, v in (("iteration_ms", it_ms), ("errors_call_ms", ev_ms), ("errors_kernel_ms", ev_kernel), ("snapshot_ms", snap_ms),
                    ("restore_ms", rest_ms), ("ranking_call_ms", rank_ms)):
        line.update(_stats(name, v))
    line["errors_over_iteration"] = round(line["errors_call_ms"] / line["iteration_ms"], 5)
    line["ranking_over_iteration"] = round(line["ranking_call_ms"] / line["iteration_ms"], 5)
    print(json.dumps(line), flush=True)


def fit_worker(runs, warmup, scale, niter):
    import numpy as np
    import bench
    from cmfrec_amd import CMF_implicit, Validation
    m, n, k, train, heldout = _problem(scale)
    A0 = np.random.default_rng(100).random((m, k)) * 2.0 ** -7
    B0 = np.zeros((n, k))
    watches = {"plain": lambda: None,
               "watched": lambda: Validation(heldout, metric="rmse", restore_best=False),
               "watched_restore_best": lambda: Validation(heldout, metric="rmse", restore_best=True),
               "watched_ndcg": lambda: Validation(heldout, metric="ndcg", k=10, users=_rank_users(heldout, scale), restore_best=False)}
    line = dict(what="fit", dtype="float64", k=k, m=m, n=n, nnz=len(train[2]), n_heldout=len(heldout[2]), niter=[niter, 3 * niter], runs=runs,
                warmup=warmup)
    med = {}
    for its in (niter, 3 * niter):
        ms = {name: [] for name in watches}
        last = {}
        for it in range(warmup + runs):
            for name, make in watches.items():
                mdl = CMF_implicit(k=k, lambda_=bench.LAM, use_cg=True, max_cg_steps=bench.MAX_CG_STEPS, niter=its, use_float=False,
                                   precompute_for_predictions=False)
                s0 = time.perf_counter()
                mdl.fit(train, shape=(m, n), A0=A0, B0=B0, validation=make())
                if it >= warmup:
                    ms[name].append((time.perf_counter() - s0) * 1e3)
                last[name] = mdl
        assert np.array_equal(last["plain"].A_, last["watched"].A_), "a monitor-only watch changed the fit"
        for name, v in ms.items():
            line.update(_stats("fit%d_%s_ms" % (its, name), v))
            med[its, name] = float(np.median(v))
        line["rmse_curve"] = [round(h["rmse"], 6) for h in last["watched"].validation_history_]
        line["best_iteration"] = last["watched_restore_best"].best_iteration_
    # a fit's time is a fixed part (upload, COO -> CSR / CSC; with a watch the set's sort and upload and the monitor's checks) plus a
    # part per iteration: the two iteration counts separate them
    for name in watches:
        per_it = (med[3 * niter, name] - med[niter, name]) / (2 * niter)
        line["%s_ms_per_iteration" % name] = round(per_it, 4)
        line["%s_fixed_ms" % name] = round(med[niter, name] - niter * per_it, 3)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_validation", "bench_fit_validation.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--niter", type=int, default=4, help="iterations of the fits of the 'fit' part")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workload (debug only)")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per part")
    ap.add_argument("--only", default=None, choices=["session", "fit"])
    ap.add_argument("--session-worker", action="store_true")
    ap.add_argument("--fit-worker", action="store_true")
    a = ap.parse_args()
    if a.session_worker:
        return session_worker(a.runs, a.warmup, a.scale)
    if a.fit_worker:
        return fit_worker(a.runs, a.warmup, a.scale, a.niter)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--%s-worker" % part] for part in ("session", "fit") if a.only in (None, part)]
    common = ["--runs", str(a.runs), "--warmup", str(a.warmup), "--scale", str(a.scale), "--niter", str(a.niter)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_fit_validation: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
