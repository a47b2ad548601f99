#!/usr/bin/env python3
"""Times the exact top-N through the certified fp16 filter (Ranker(filter="fp16")) against the exact route on
the same ranker in the same process, alternating call by call: nu = 16,384 users against n = 160,112 items, n_top = 10 and 50,
k = 50 / 128 / 256 in double and 64 / 272 in single precision, medians of `--runs` calls after `--warmup`.

    python tools/bench_topn_filter.py                 # every configuration, appended to profiles/topn_filter/bench_topn_filter.jsonl
    python tools/bench_topn_filter.py --model-like    # factors with a decaying spectrum instead of Gaussian ones

Every configuration runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is started
on a device that has just faulted).  Each line: HIP-event times of the three stages of the filtered call (filter, refinement,
certificate), the image build, the exact route's kernel, both routes end to end (host clock around the call, which ends in a
synchronise), the certified share, and whether the two routes returned the same ids."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N = 16384, 160112
CONFIGS = [("float64", 50), ("float64", 128), ("float64", 256), ("float32", 64), ("float32", 272)]
NTOPS = (10, 50)


def worker(dtype, k, n_top, nu, n, runs, warmup, model_like):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    A = rng.standard_normal((nu, k)); B = rng.standard_normal((n, k))
    if model_like:                                            # a decaying spectrum: a few strong directions, a long tail
        w = 1.0 / np.sqrt(1.0 + np.arange(k))
        A, B = A * w, B * w
    A, B = A.astype(dt), B.astype(dt)
    ms = {"filter": [], "refine": [], "certify": [], "exact_kernel": []}
    e2e = {"on": [], "off": []}
    with Ranker(B) as rk:
        rk.filter = "fp16"
        image_ms = rk.filter_ms()["image"]
        for it in range(warmup + runs):
            for route in ("on", "off"):
                rk.filter = "fp16" if route == "on" else None     # (switching it on again rebuilds the image: outside the timing)
                t0 = time.perf_counter()
                ids, _ = rk.topN(A, n=n_top)
                t1 = time.perf_counter()
                if it < warmup:
                    continue
                e2e[route].append((t1 - t0) * 1e3)
                if route == "on":
                    stats, stage = rk.filter_stats(), rk.filter_ms()
                    for s in ("filter", "refine", "certify"):
                        ms[s].append(stage[s])
                    ids_on = ids
                else:
                    ms["exact_kernel"].append(rk.kernel_ms())
                    same = bool(np.array_equal(ids, ids_on))
    med = lambda v: round(float(np.median(v)), 4)
    print(json.dumps(dict(what="topn_filter", factors="model-like" if model_like else "gaussian", dtype=dtype, k=k, n_top=n_top, nu=nu, n=n,
                          runs=runs, image_build_ms=round(image_ms, 4), filter_ms=med(ms["filter"]), refine_ms=med(ms["refine"]),
                          certify_ms=med(ms["certify"]), exact_kernel_ms=med(ms["exact_kernel"]),
                          e2e_filter_ms=med(e2e["on"]), e2e_filter_ms_min=round(min(e2e["on"]), 4), e2e_filter_ms_max=round(max(e2e["on"]), 4),
                          e2e_exact_ms=med(e2e["off"]), e2e_exact_ms_min=round(min(e2e["off"]), 4), e2e_exact_ms_max=round(max(e2e["off"]), 4),
                          certified_share=round(stats["certified"] / max(stats["users"], 1), 6), filtered=stats["filtered"],
                          same_ids=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_filter", "bench_topn_filter.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--model-like", action="store_true")
    ap.add_argument("--only", default=None, help="dtype:k, e.g. float64:128")
    ap.add_argument("--worker", nargs=3, metavar=("DTYPE", "K", "NTOP"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), int(a.worker[2]), a.nu, a.n, a.runs, a.warmup, a.model_like)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    steps = [["--worker", dt, str(k), str(nt)] for dt, k in CONFIGS for nt in NTOPS if a.only in (None, "%s:%d" % (dt, k))]
    common = ["--nu", str(a.nu), "--n", str(a.n), "--runs", str(a.runs), "--warmup", str(a.warmup)] + (["--model-like"] if a.model_like else [])
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_topn_filter: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
