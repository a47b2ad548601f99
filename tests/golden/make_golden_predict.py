"""Records tests/golden/g42_predict_{f64,f32}.npz: the compiled reference's predict_X_old_collective_explicit / _implicit on
predict_reference.old_problem (k_main = 0 and 2) and its predict_X_new_collective_explicit / _implicit on the cases of
predict_reference.new_cases, both precisions, ONE CASE PER CHILD PROCESS (a case on which the reference dies must not take the
others with it).  Needs oracle/_ref (built by __graft_entry__.build() where the reference's sources are).

    python tests/golden/make_golden_predict.py

A case is left out of the fixture -- and reported -- when the child dies or returns non-zero.  Data only: one vector of
predictions per case (300 values for predict_X_old, 200 for predict_X_new).  No negative index is given to the reference (its
fallback reads biasA[row] / biasB[col] for one)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import new_rows_options as nro  # noqa: E402
import predict_reference as pr  # noqa: E402

DT = {"f64": np.float64, "f32": np.float32}


def jobs(dtype):
    """(key, callable(lib) -> (rc, predicted)) of every recorded case."""
    out = []
    for km in pr.OLD_KMS:
        d = pr.old_problem(dtype, km)
        for implicit in (False, True):
            out.append(("old_%s_km%d" % ("imp" if implicit else "exp", km),
                        lambda lib, d=d, implicit=implicit: pr.call_old(lib, dtype, d, implicit)))
    for k in nro.KS:
        for name, kind, kw in pr.new_cases(dtype, k):
            prow, pcol = pr.new_pairs(kw)
            out.append((pr.key_of(k, name), lambda lib, kind=kind, kw=kw, prow=prow, pcol=pcol: pr.call_new(lib, dtype, kind, prow, pcol, **kw)))
    return out


def child(tag, index, out):
    from oracle.bindings import Reference
    dtype = DT[tag]
    rc, pred = jobs(dtype)[index][1](Reference(dtype).lib)
    if rc != 0:
        sys.exit(10 + rc)
    np.savez(out, pred=pred)


def main():
    tmp = os.path.join(HERE, "_g42_child.npz")
    left_out = []
    for tag, dtype in DT.items():
        store = {}
        for index, (key, _) in enumerate(jobs(dtype)):
            if os.path.exists(tmp):
                os.remove(tmp)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tag, str(index), tmp])
            if r.returncode != 0 or not os.path.exists(tmp):
                left_out.append("%s %s: the reference died or returned non-zero (exit status %d)" % (tag, key, r.returncode))
                continue
            store[key] = np.load(tmp)["pred"]
        np.savez_compressed(os.path.join(HERE, "%s_%s.npz" % (pr.FIXTURE, tag)), **store)
        print("%s: %d arrays" % (tag, len(store)))
    if os.path.exists(tmp):
        os.remove(tmp)
    print("left out:\n  " + "\n  ".join(left_out or ["nothing"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        main()
