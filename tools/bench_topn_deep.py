#!/usr/bin/env python3
"""Times deep top-N lists (Ranker.topN_deep: pages of topn_after_kernel chained on the device) by the protocol of
tools/bench_topn.py: nu = 16,384 random users against n = 160,112 items, the HIP-event time around all the pages of a call
(cmfrec_hip_ranker_kernel_ms), median of 10 runs after 3 warm-ups.

    python tools/bench_topn_deep.py             # every configuration, appended to profiles/topn_deep/bench.jsonl
    python tools/bench_topn_deep.py --only float64:96,float32:128     # other widths, e.g. between two page-length ranges

Every (precision, k) runs in a child process of its own under `timeout`; the first that fails ends the run (nothing more is
started on a device that has just faulted).  Within a child, for n_top = 128, 500 and 1000 the page lengths 128, 256 and 512
(CMFREC_HIP_TOPN_PAGE, re-read on every call) are timed alternating run by run; at n_top = 128 the same batch also goes through
Ranker.topN under CMFREC_HIP_TOPN=wide -- topn_wide_kernel, one list of 128 -- which is what one page of 128 is held against.

Each line: milliseconds of the call, launches and page length (Ranker.pages), milliseconds per page, the users per workgroup of
the last page."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, N = 16384, 160112
CONFIGS = [("float64", 50), ("float64", 128), ("float64", 256), ("float32", 272)]
NTOPS = (128, 500, 1000)
PAGES = (128, 256, 512)


def worker(dtype, k, nu, n, runs, warmup):
    import numpy as np
    sys.path.insert(0, ROOT)
    from cmfrec_amd import Ranker
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(k)
    A = rng.standard_normal((nu, k)).astype(dt); B = rng.standard_normal((n, k)).astype(dt)
    with Ranker(B) as rk:
        for n_top in NTOPS:
            routes = [("deep", p) for p in PAGES if p == 128 or p < 2 * n_top] + ([("wide_topN", 0)] if n_top == 128 else [])
            ms = {r: [] for r in routes}
            info = {}
            for it in range(warmup + runs):
                for route in routes:
                    what, page = route
                    if what == "deep":
                        os.environ["CMFREC_HIP_TOPN_PAGE"] = str(page)
                        rk.topN_deep(A, n_top)
                        info[route] = rk.pages() + rk.launch_shape()
                    else:
                        os.environ["CMFREC_HIP_TOPN"] = "wide"
                        rk.topN(A, n=n_top)
                        os.environ.pop("CMFREC_HIP_TOPN")
                        info[route] = (1, n_top) + rk.launch_shape()
                    if it >= warmup:
                        ms[route].append(rk.kernel_ms())
            for route in routes:
                t = float(np.median(ms[route]))
                launches, page_len, users, groups = info[route]
                print(json.dumps(dict(kernel="topn_after_kernel" if route[0] == "deep" else "topn_wide_kernel", route=route[0],
                                      dtype=dtype, k=k, n_top=n_top, nu=nu, n=n, page_asked=route[1], page_len=page_len, pages=launches,
                                      ms=round(t, 4), ms_min=round(min(ms[route]), 4), ms_max=round(max(ms[route]), 4),
                                      ms_per_page=round(t / launches, 4), runs=runs, users_per_workgroup=users, workgroups=groups)),
                      flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_deep", "bench.jsonl"))
    ap.add_argument("--nu", type=int, default=NU)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--only", default=None, help="dtype:k[,dtype:k ...] in place of the standard four, e.g. float64:96,float32:128")
    ap.add_argument("--worker", nargs=2, metavar=("DTYPE", "K"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), a.nu, a.n, a.runs, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    configs = CONFIGS if a.only is None else [(c.split(":")[0], int(c.split(":")[1])) for c in a.only.split(",")]
    steps = [["--worker", dt, str(k)] for dt, k in configs]
    common = ["--nu", str(a.nu), "--n", str(a.n), "--runs", str(a.runs), "--warmup", str(a.warmup)]
    with open(a.out, "a") as f:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + step
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.stderr.write("\nbench_topn_deep: %s ended with status %d; stopping\n" % (" ".join(step), r.returncode))
                return r.returncode
            f.write(r.stdout); f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
