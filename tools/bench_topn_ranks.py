#!/usr/bin/env python3
"""Times the rank kernel (Ranker.ranks, topn_rank_kernel) on the ranking benchmark's shape: nu = 16,384 random users against
n = 160,112 items, 10 held-out and about 50 excluded items per user.  The yardstick is topn_wide_kernel at n_top = 10 on the same
batch, exclusion lists and handle in the same process (CMFREC_HIP_TOPN=wide, so that k = 50 takes it too): it reads the same
bytes and does the same products.

Per configuration, medians and the spread (min, max) of the HIP-event kernel times over the timed runs after the warm-ups:

    topn_wide_ms          topn_wide_kernel, n_top = 10, with the exclusion lists
    ranks_ms              topn_rank_kernel, 10 held-out items per user, with the exclusion lists (thresholds and exclusion steps
                          included: they are part of the kernel)
    ranks_no_excl_ms      the same without exclusion lists: what the exclusion step costs
    ranks_own_best_ms     each user's own 10 best items held out: every other score beats none of the thresholds (the first exit)
    ranks_own_worst_ms    each user's own 10 worst items held out: every other score beats all of them (the second exit, a
                          per-lane register); random held-out items lie between the two -- most scores take the binary search and
                          an LDS atomic
    ranks_1000_ms         1,000 held-out items per user, with the exclusion lists: the sort and the binary search grow, and where
                          1,000 thresholds do not fit the LDS beside the factors the items are streamed once per slice
    ratio                 ranks_ms / topn_wide_ms (medians); ratio_1000 likewise
    *_end_to_end_s        wall clock of the Python call, uploads and downloads included

The ranks below 10 are compared once with the top-N result (they must name the same items).

    python tools/bench_topn_ranks.py            # every configuration, appended to profiles/topn_ranks/bench.jsonl

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N, NTOP, HELD, EXCL, LONG = 16384, 160112, 10, 10, 50, 1000
CONFIGS = [("float64", 50), ("float64", 128), ("float32", 272)]


def med(x):
    import numpy as np
    return dict(median=round(float(np.median(x)), 4), min=round(float(min(x)), 4), max=round(float(max(x)), 4))


def lists(rng, nu, n, length):
    """(indptr, indices): `length` random items per user, sorted, the repeats of a draw dropped."""
    import numpy as np
    from cmfrec_amd.ops import _sorted_include
    ip = np.arange(nu + 1, dtype=np.int64) * length
    return _sorted_include((ip, rng.integers(0, n, int(ip[-1]), dtype=np.int64)), nu)


def worker(dtype, k, nu, n, runs, warmup, commit):
    import numpy as np
    os.environ["CMFREC_HIP_TOPN"] = "wide"
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    A = rng.standard_normal((nu, k)).astype(dt); B = rng.standard_normal((n, k)).astype(dt)
    held, excl, held_long = lists(rng, nu, n, HELD), lists(rng, nu, n, EXCL), lists(rng, nu, n, LONG)
    res = {}
    with Ranker(B) as rk:
        def timed(name, call):
            ms, wall, shape = [], [], None
            for it in range(warmup + runs):
                t0 = time.perf_counter()
                out = call()
                t1 = time.perf_counter()
                if it >= warmup:
                    ms.append(rk.kernel_ms()); wall.append(t1 - t0)
                shape = rk.launch_shape()
            res[name + "_ms"] = med(ms); res[name + "_end_to_end_s"] = med(wall); res[name + "_launch"] = list(shape)
            return out, float(np.median(ms))
        (ids, _), t_top = timed("topn_wide", lambda: rk.topN(A, n=NTOP, exclude=excl))
        (hp, hi, ranks, pool), t_rank = timed("ranks", lambda: rk.ranks(A, held, exclude=excl))
        _, t_plain = timed("ranks_no_excl", lambda: rk.ranks(A, held))
        _, t_long = timed("ranks_1000", lambda: rk.ranks(A, held_long, exclude=excl))
        # the two exits on their own: each user's own 10 best items held out (every other score beats none of the thresholds) and
        # its 10 worst (every other score beats all of them)
        ip10 = np.arange(nu + 1, dtype=np.int64) * NTOP
        worst_ids, _ = rk.topN(-A, n=NTOP, exclude=excl)
        (_, _, r_best, _), t_best = timed("ranks_own_best", lambda: rk.ranks(A, (ip10, np.sort(ids, axis=1).ravel()), exclude=excl))
        (_, _, r_worst, pool_w), t_worst = timed("ranks_own_worst", lambda: rk.ranks(A, (ip10, np.sort(worst_ids, axis=1).ravel()), exclude=excl))
    assert np.array_equal(np.sort(r_best.reshape(nu, NTOP), axis=1), np.tile(np.arange(NTOP), (nu, 1))), "the 10 best are not places 0 .. 9"
    assert np.array_equal(np.sort(r_worst.reshape(nu, NTOP), axis=1), pool_w[:, None] - NTOP + np.arange(NTOP)), "the 10 worst are not the last places"
    # the held-out items ranked below n_top are the items the top-N call returned at those places
    owner = np.repeat(np.arange(nu), np.diff(hp))
    low = (ranks >= 0) & (ranks < NTOP)
    assert np.array_equal(ids[owner[low], ranks[low]], hi[low]), "ranks and top-N disagree"
    print(json.dumps(dict(what="topn_ranks", commit=commit, dtype=dtype, k=k, nu=nu, n=n, held=int(hp[-1]), excluded=int(excl[0][-1]),
                          held_long=int(held_long[0][-1]), runs=runs, warmup=warmup, ranked_below_10=int(low.sum()),
                          ratio=round(t_rank / t_top, 3), ratio_no_excl=round(t_plain / t_top, 3), ratio_1000=round(t_long / t_top, 3),
                          ratio_own_best=round(t_best / t_top, 3), ratio_own_worst=round(t_worst / t_top, 3),
                          **res)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_ranks", "bench.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:128")
    ap.add_argument("--commit", default="", help="what the numbers were measured on (recorded in every line)")
    ap.add_argument("--worker", nargs=2, metavar=("DTYPE", "K"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.nu, a.n, a.runs, a.warmup, a.commit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k)] for dt, k in CONFIGS if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--nu", str(a.nu), "--n", str(a.n), "--runs", str(a.runs), "--warmup", str(a.warmup), "--commit", a.commit]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_topn_ranks: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
