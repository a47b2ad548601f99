"""Records tests/golden/g41_impute_{f64,f32}.npz: the compiled reference's impute_X_collective_explicit on the cases i0-i6 of
tests/impute_reference.py, both precisions and both k, ONE CASE PER CHILD PROCESS (a case on which the reference dies must not
take the others with it).  Needs oracle/_ref (built by __graft_entry__.build() where the reference's sources are).

    python tests/golden/make_golden_impute.py

A case is left out of the fixture -- and reported -- when the child dies, returns non-zero or returns non-finite values.  Data
only: the outputs, [48, 70] per case.  Afterwards the script asserts the condition the float32 tolerance of the GPU test rests
on: the reference's own float32 result lies within a quarter of new_rows_options.TOL32 of its float64 result on every case."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import impute_reference as ir  # noqa: E402
import new_rows_options as nro  # noqa: E402

DT = {"f64": np.float64, "f32": np.float32}


def child(tag, k, index, out):
    from oracle.bindings import Reference
    dtype = DT[tag]
    name, kw = ir.impute_cases(nro.problem(dtype, k))[index]
    rc, X = ir.call_impute(Reference(dtype).lib, dtype, k=k, **kw)
    if rc != 0:
        sys.exit(10 + rc)
    np.savez(out, X=X)


def main():
    tmp = os.path.join(HERE, "_g41_child.npz")
    left_out, drop = [], set()
    for tag, dtype in DT.items():           # (float64 first: what it leaves out is left out in float32 too)
        store = {}
        for k in nro.KS:
            for index, (name, kw) in enumerate(ir.impute_cases(nro.problem(dtype, k))):
                if os.path.exists(tmp):
                    os.remove(tmp)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tag, str(k), str(index), tmp])
                why = None
                if r.returncode != 0 or not os.path.exists(tmp):
                    why = "the reference died or returned non-zero (exit status %d)" % r.returncode
                elif not np.isfinite(np.load(tmp)["X"]).all():
                    why = "non-finite values"
                if why or (k, name) in drop:
                    if why:
                        drop.add((k, name)); left_out.append("%s k=%d %s: %s" % (tag, k, name, why))
                    continue
                store[ir.key_of(k, name)] = np.load(tmp)["X"]
        np.savez_compressed(os.path.join(HERE, "%s_%s.npz" % (ir.FIXTURE, tag)), **store)
        print("%s: %d arrays" % (tag, len(store)))
    if os.path.exists(tmp):
        os.remove(tmp)
    print("left out:\n  " + "\n  ".join(left_out or ["nothing"]))
    g64, g32 = ir.load_fixture(np.float64), ir.load_fixture(np.float32)
    for k in nro.KS:
        for name, kw in ir.impute_cases(nro.problem(np.float64, k)):
            key = ir.key_of(k, name)
            if key in g64.files and key in g32.files:
                e = ir.imputed_row_err(g32[key], g64[key], kw["Xfull"])
                print("%s: float32 against float64 %.2e" % (key, e))
                assert e < nro.TOL32 / 4, (key, e)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        main()
