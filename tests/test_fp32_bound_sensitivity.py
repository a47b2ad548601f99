"""The float64 criteria of tests/test_gpu_single_precision.py can see a subtly wrong kernel (CPU, oracles only).

For every case the GPU file runs: (a) the float32 oracle itself passes the forward and, on closed-form routes, the backward
criterion of tests/fp32_reference.py; (b) what a wrong kernel would compute -- a row's last entry lost, the first entry of a
slice counted twice, B rounded to fp16 before the gather, the shared matrix solved by its explicit inverse without the
refinement step -- is rejected with the margin fp32_reference.MARGIN asks for; (c) the margins are printed (pytest -s)."""
import numpy as np
import pytest

import fp32_reference as F


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_oracle_passes_and_mutations_fail(name):
    c = F.case(name)
    a64, ao, system = F.references(name)
    fwd, bwd = F.check_case(name, ao)                                    # (a)
    line = "%-20s float32 oracle: fwd %.3f%s" % (name, fwd, "" if bwd is None else ", bwd %.3f" % bwd)
    muts = F.mutations(name)
    assert "drop last entry" in muts or c.get("csr") is None
    assert "B through fp16" in muts
    if c["route"] in ("naz", "impfeat"):
        assert "explicit inverse" in muts
    lens = np.diff(c["csr"][0].astype(np.int64)) if c.get("csr") is not None else None
    if lens is not None and lens.max() >= F.VH_MIN_F32:
        assert "slice start twice" in muts
    for mname, (am, rows) in muts.items():                                # (b)
        assert len(rows) > 0, mname
        r = F.rejection_ratios(name, am, rows)
        margin = F.rejection(mname, r)
        line += " | %s %.1f (rows %d, min %.1f, median %.1f)" % (mname, margin, len(rows), r.min(), np.median(r))
        assert margin >= F.MARGIN[mname], "%s: %s rejected only %.2fx (min row %.2f, median %.2f)" % (
            name, mname, margin, r.min(), np.median(r))
        F._log("reject-" + mname.replace(" ", "-"), margin)
    print(line)                                                           # (c)


def test_production_case_takes_2048_entry_slices():
    """The production-slicing case crosses device.hpp's threshold (split rows holding >= 2048 * 1024 entries); the ladder's
    split rows stay on 256-entry slices."""
    lens = F.case("prod-cg")["lens"]
    assert sum(int(l) for l in lens if l >= F.VH_MIN_F32) >= F.GRAM_SLICE * 1024
    assert F.slice_len(lens) == 2048
    assert F.slice_len(F.LADDER) == 256
