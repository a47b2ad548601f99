#!/usr/bin/env python3
"""Times the factors of new users under NA_as_zero on the headline shape: 16,384 users against 160,112 items, about 50 entries
per user, k = 50 in double and k = 64 in single precision, with a user bias, with and without a dense U of 64 attributes.

    (naz)   model.new_users().factors(X, U) of a model with NA_as_zero=True: the shared-matrix route -- one gather-sum over the
            triplets (newrows_naz_kernels.hpp) and one product with the inverse the handle keeps;
    (plain) the same handle call on the same batch for the same model with the option off: the per-row Cholesky route, the
            nearest thing the library had before.  It solves another model; it is here as the yardstick of cost only.

Per configuration: HIP-event time of the solve phase as the handle reports it (NewUsers.kernel_ms: from the uploads of the batch
to the last solve kernel), `--warmup` calls per handle (3), then `--runs` repetitions (30) alternating between the two handles in one
process; median, minimum and maximum are reported.  `share_of_8TBps`: the algorithmic bytes of the batch -- the triplets, the
gathered item rows, the factors written -- over the median time, as a share of 8 TB/s.

    python tools/bench_new_users_naz.py          # every configuration, appended to profiles/new_users_naz/bench_new_users_naz.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 160112
USERS = 16384
P = 64
CONFIGS = [("float64", 50), ("float32", 64)]


def make_model(dtype, k, n, p):
    """A CMF that holds random factors as if fitted with NA_as_zero=True (nothing precomputed: the handle builds its own)."""
    import numpy as np
    from cmfrec_amd import CMF
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    mdl = CMF(k=k, lambda_=5., user_bias=True, item_bias=True, NA_as_zero=True, precompute_for_predictions=False,
              use_float=dt is np.float32)
    e = np.empty((0, 0), dt)
    mdl.B_ = (0.1 * rng.standard_normal((n, k))).astype(dt)
    mdl.C_ = (0.1 * rng.standard_normal((p, k))).astype(dt) if p else e
    mdl.A_ = e; mdl.D_ = e; mdl.Bi_ = e
    mdl.item_bias_ = (0.1 * rng.standard_normal(n)).astype(dt)
    mdl.user_bias_ = np.empty(0, dt)
    mdl.glob_mean_ = 3.5
    mdl._U_colmeans = (0.1 * rng.standard_normal(p)).astype(dt)
    mdl._I_colmeans = np.empty(0, dt)
    mdl._scaling_biasA = 1.
    mdl._TransBtBinvBt = e; mdl._TransCtCinvCt = e
    mdl.is_fitted_ = True
    return mdl


def make_users(seed, rows, n, dt, per_user=50):
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = np.maximum(rng.poisson(per_user, rows), 1)
    r = np.repeat(np.arange(rows), lens).astype(np.int32)
    c = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.int32)
    v = (0.5 * rng.integers(1, 11, len(r))).astype(dt)
    perm = rng.permutation(len(r))
    return r[perm], c[perm], v[perm]


def worker(dtype, k, p, rows, n, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    dt = np.dtype(dtype).type
    mdl = make_model(dtype, k, n, p)
    off = copy.copy(mdl)
    off.NA_as_zero = False
    X = make_users(rows, rows, n, dt)
    U = np.random.default_rng(3).standard_normal((rows, p)).astype(dt) if p else None
    ms = {"naz": [], "plain": []}
    with mdl.new_users() as h_naz, off.new_users() as h_plain:
        for it in range(warmup + runs):
            for tag, h in (("naz", h_naz), ("plain", h_plain)):
                A, bias = h.factors(X, U=U, return_bias=True)
                assert np.isfinite(A).all() and np.isfinite(bias).all()
                if it >= warmup:
                    ms[tag].append(h.kernel_ms()[0])
    real = np.dtype(dt).itemsize
    nnz, kx = len(X[2]), k + 1
    algo_bytes = nnz * (8 + real) + nnz * kx * real + rows * kx * real + (rows * p * real if p else 0)
    med = lambda x: float(np.median(x))
    out = dict(what="new_users_naz", dtype=dtype, k=k, p=p, n=n, users=rows, entries=nnz, runs=runs, warmup=warmup,
               algorithmic_bytes=int(algo_bytes))
    for tag in ("naz", "plain"):
        out["%s_solve_ms" % tag] = round(med(ms[tag]), 3)
        out["%s_solve_ms_min" % tag] = round(min(ms[tag]), 3)
        out["%s_solve_ms_max" % tag] = round(max(ms[tag]), 3)
    out["naz_share_of_8TBps"] = round(algo_bytes / (med(ms["naz"]) * 1e-3) / 8e12, 4)
    out["plain_over_naz"] = round(med(ms["plain"]) / med(ms["naz"]), 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_users_naz", "bench_new_users_naz.jsonl"))
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--users", type=int, default=USERS)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "P"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), int(a.worker[2]), a.users, a.n, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), str(p)] for dt, k in CONFIGS for p in (0, P)]
    common = ["--n", str(a.n), "--users", str(a.users), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_new_users_naz: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
