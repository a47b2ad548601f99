#!/usr/bin/env python3
"""Times the ranking over per-user candidate lists (Ranker.topN(include=), topn_cand_kernel) on the ranking benchmark's shape:
nu = 16,384 random users against n = 160,112 items, n_top = 10, and about 1,000 candidates per user --

    uniform   1,000 random items per user (a few less where the draw repeats an item);
    heavy     lengths from a truncated power law on [10, 20,000], p(L) ~ L^-a, with a chosen so that the mean is 1,000 (a = 1
              would be log-uniform, whose mean on that range is 2,630; the exponent used is in the output line).

Per configuration and kind of list, medians and the spread (min, max) over the timed runs after the warm-ups:

    cand_kernel_ms        HIP-event time of topn_cand_kernel (cmfrec_hip_ranker_kernel_ms), gathered_bytes_per_s = the bytes of
                          the 16-byte pieces of the listed rows / that time
    cand_end_to_end_s     wall clock of Ranker.topN(A, n, include=(indptr, indices)) -- the lists are handed over sorted
    pairs_*               the route without candidate lists: flatten the lists into (user, item) pairs, Scorer.predict, download
                          one score per candidate, top-N per user in NumPy (argpartition on the [nu, L] matrix where all lists
                          have one length, else user by user): the scorer's kernel time and the wall clock of the whole route
    full_*                Ranker.topN over all n items for the same users, for context

The ids of the first two routes are compared once (they must be equal: the candidate kernel states the scorer's arithmetic).

    python tools/bench_topn_candidates.py            # every configuration, appended to profiles/topn_candidates/bench.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N, NTOP, MEAN, LO, HI = 16384, 160112, 10, 1000, 10, 20000
CONFIGS = [("float64", 50), ("float64", 128), ("float32", 272)]
KINDS = ("uniform", "heavy")


def power_law_lengths(rng, nu, lo, hi, mean):
    """Lengths with density ~ L^-a on [lo, hi], a found by bisection so that the mean is `mean`."""
    import numpy as np

    def mean_of(a):
        return (1 - a) / (2 - a) * (hi ** (2 - a) - lo ** (2 - a)) / (hi ** (1 - a) - lo ** (1 - a))
    a0, a1 = 1.0001, 1.9999
    for _ in range(60):
        a = 0.5 * (a0 + a1)
        if mean_of(a) > mean:
            a0 = a
        else:
            a1 = a
    u = rng.random(nu)
    L = (lo ** (1 - a) + u * (hi ** (1 - a) - lo ** (1 - a))) ** (1 / (1 - a))
    return np.clip(np.rint(L), lo, hi).astype(np.int64), a


def top_n_numpy(cp, ci, s, n_top):
    """The n_top best of every user's scored list, ties to the lower id (the lists are ascending)."""
    import numpy as np
    nu = len(cp) - 1
    lens = np.diff(cp.astype(np.int64))
    ids = np.full((nu, n_top), -1, np.int32)
    if lens.min() == lens.max() and lens[0] >= n_top:
        L = int(lens[0])
        S = s.reshape(nu, L); I = ci.reshape(nu, L)
        part = np.argpartition(-S, n_top - 1, axis=1)[:, :n_top]
        ps = np.take_along_axis(S, part, 1); pi = np.take_along_axis(I, part, 1)
        o = np.lexsort((pi, -ps), axis=1)
        return np.take_along_axis(pi, o, 1)
    for u in range(nu):
        lo, hi = int(cp[u]), int(cp[u + 1])
        su, cu = s[lo:hi], ci[lo:hi]
        if hi - lo > n_top:
            part = np.argpartition(-su, n_top - 1)[:n_top]
            su, cu = su[part], cu[part]
        o = np.lexsort((cu, -su))
        ids[u, :len(o)] = cu[o]
    return ids


def med(x):
    import numpy as np
    return dict(median=round(float(np.median(x)), 4), min=round(float(min(x)), 4), max=round(float(max(x)), 4))


def worker(dtype, k, kind, nu, n, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker, Scorer
    from cmfrec_amd.ops import _sorted_include
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    A = rng.standard_normal((nu, k)).astype(dt); B = rng.standard_normal((n, k)).astype(dt)
    exponent = None
    if kind == "uniform":
        lens = np.full(nu, MEAN, np.int64)
    else:
        lens, exponent = power_law_lengths(rng, nu, LO, min(HI, n), MEAN)
    ip = np.concatenate([[0], np.cumsum(lens)])
    cp, ci = _sorted_include((ip, rng.integers(0, n, int(ip[-1]), dtype=np.int64)), nu)       # sorted, the repeats dropped
    if kind == "uniform":                                    # one length for all (the [nu, L] form of the NumPy route): cut to the shortest
        L = int(np.diff(cp.astype(np.int64)).min())
        keep = (np.arange(len(ci)) - np.repeat(cp[:-1].astype(np.int64), np.diff(cp.astype(np.int64)))) < L
        ci = np.ascontiguousarray(ci[keep]); cp = (np.arange(nu + 1) * L).astype(np.uint64)
    total = int(cp[-1])
    piece = 16 // np.dtype(dt).itemsize
    row_bytes = (k + piece - 1) // piece * 16
    t_cand, ms_cand, t_pairs, ms_pairs, t_full, ms_full = [], [], [], [], [], []
    with Ranker(B) as rk, Scorer(A, B, glob_mean=0.0) as sc:
        for it in range(warmup + runs):
            t0 = time.perf_counter()
            ids, _ = rk.topN(A, n=NTOP, include=(cp, ci))
            t1 = time.perf_counter()
            ms = rk.kernel_ms(); shape = rk.launch_shape()
            t2 = time.perf_counter()
            row = np.repeat(np.arange(nu, dtype=np.int32), np.diff(cp.astype(np.int64)))
            s = sc.predict(row, ci)
            ids_p = top_n_numpy(cp, ci, s, NTOP)
            t3 = time.perf_counter()
            if it == 0:
                assert np.array_equal(ids, ids_p), "the two routes disagree"
            if it >= warmup:
                t_cand.append(t1 - t0); ms_cand.append(ms); t_pairs.append(t3 - t2); ms_pairs.append(sc.kernel_ms())
        for it in range(1 + min(runs, 3)):
            t0 = time.perf_counter()
            rk.topN(A, n=NTOP)
            t1 = time.perf_counter()
            if it >= 1:
                t_full.append(t1 - t0); ms_full.append(rk.kernel_ms())
    k_ms = float(np.median(ms_cand))
    print(json.dumps(dict(what="topn_candidates", dtype=dtype, k=k, n_top=NTOP, nu=nu, n=n, lists=kind, exponent=exponent,
                          candidates=total, longest=int(np.diff(cp.astype(np.int64)).max()), runs=runs, warmup=warmup,
                          wavefronts_per_workgroup=shape[0], workgroups=shape[1],
                          cand_kernel_ms=med(ms_cand), gathered_bytes_per_s=round(total * row_bytes / (k_ms * 1e-3), 1),
                          cand_end_to_end_s=med(t_cand), pairs_kernel_ms=med(ms_pairs), pairs_end_to_end_s=med(t_pairs),
                          end_to_end_gain=round(float(np.median(t_pairs)) / float(np.median(t_cand)), 3),
                          worst_case_gain=round(min(t_pairs) / max(t_cand), 3),
                          full_kernel_ms=med(ms_full), full_end_to_end_s=med(t_full))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_candidates", "bench.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:128")
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "KIND"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.worker[2], a.nu, a.n, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), kind] for dt, k in CONFIGS for kind in KINDS if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--nu", str(a.nu), "--n", str(a.n), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_topn_candidates: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
