"""Records tests/golden/g43_new_rows_naz_{f64,f32}.npz: the compiled reference's factors_collective_explicit_multiple with
NA_as_zero_X / NA_as_zero_U on the cases of tests/new_rows_naz.py, both precisions, ONE CASE PER CHILD PROCESS (a case on which
the reference dies must not take the others with it).  Needs oracle/_ref (built by __graft_entry__.build() where the
reference's sources are).

    python tests/golden/make_golden_new_rows_naz.py

A case is left out of the fixture -- and reported -- when the child dies, returns non-zero, returns non-finite values, or
disagrees with the float64 normal equations of tests/new_rows_naz.normal_equations by more than 1e-8.  The cases of
new_rows_naz.numpy_only_cases are run too and reported with their error against the normal equations; they are never stored."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import new_rows_naz as nrz  # noqa: E402
import new_rows_options as nro  # noqa: E402

DT = {"f64": np.float64, "f32": np.float32}


def every(d):
    return nrz.cases(d) + nrz.numpy_only_cases(d)


def child(tag, k, index, out):
    from oracle.bindings import Reference
    dtype = DT[tag]
    name, kw = every(nrz.problem(dtype, k))[index]
    rc, A, bA = nro.call_multiple(Reference(dtype).lib, dtype, k=k, **kw)
    if rc != 0:
        sys.exit(10 + rc)
    np.savez(out, A=A, **({} if bA is None else {"biasA": bA}))


def main():
    tmp = os.path.join(HERE, "_g43_child.npz")
    left_out, drop = [], set()
    for tag, dtype in DT.items():           # (float64 first: what it leaves out is left out in float32 too)
        store = {}
        for k in nrz.KS:
            d = nrz.problem(dtype, k)
            for index, (name, kw) in enumerate(every(d)):
                if os.path.exists(tmp):
                    os.remove(tmp)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tag, str(k), str(index), tmp])
                why = None
                if r.returncode != 0 or not os.path.exists(tmp):
                    why = "the reference died or returned non-zero (exit status %d)" % r.returncode
                else:
                    g = np.load(tmp)
                    if not all(np.isfinite(g[f]).all() for f in g.files):
                        why = "non-finite values"
                    elif tag == "f64":
                        A, bA = nrz.normal_equations(dict(kw, k=k))
                        err = np.abs(g["A"] - A).max() / np.abs(A).max()
                        if bA is not None:
                            err = max(err, np.abs(g["biasA"] - bA).max() / max(np.abs(bA).max(), 1e-300))
                        print("%s k=%d %s: %.1e against the normal equations" % (tag, k, name, err))
                        if err > 1e-8:
                            why = "disagrees with the float64 normal equations (%.1e)" % err
                if index >= len(nrz.cases(d)):
                    left_out.append("%s k=%d %s: not stored (%s)" % (tag, k, name, why or ("agrees" if tag == "f64" else "not compared in this precision")))
                    continue
                if why is None and (k, name) in drop:
                    continue
                if why:
                    drop.add((k, name))
                    left_out.append("%s k=%d %s: %s" % (tag, k, name, why))
                    continue
                for f in g.files:
                    store["%s_%s" % (f, nrz.key_of(k, name))] = g[f]
        np.savez_compressed(os.path.join(HERE, "%s_%s.npz" % (nrz.FIXTURE, tag)), **store)
        print("%s: %d arrays" % (tag, len(store)))
    if os.path.exists(tmp):
        os.remove(tmp)
    print("left out:\n  " + "\n  ".join(left_out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        main()
