"""Device time of the compaction of a dense batch of new rows (dense_rows_device.hpp: count pass, write pass) for 4,096 rows of
10,000 items, half of them present -- cmfrec_hip_dense_rows_probe, HIP events, one warm-up run and 200 timed runs per kernel,
the whole measurement three times."""
import ctypes as C
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from cmfrec_amd import _lib

rows, n, present, reps = 4096, 10000, 0.5, 200
for dt in (np.float64, np.float32):
    lib = _lib.load(dt)
    item = np.dtype(dt).itemsize
    for rep in range(3):
        a, b, nz = C.c_double(0), C.c_double(0), C.c_size_t(0)
        rc = lib.cmfrec_hip_dense_rows_probe(C.c_int(rows), C.c_int(n), C.c_double(present), C.c_int(reps), C.byref(a), C.byref(b), C.byref(nz))
        rd = rows * n * item
        wr = nz.value * (8 + item)
        print("%-7s run %d: count %.4f ms (%.2f TB/s read)  write %.4f ms (%.2f TB/s read + written)  nnz %d  rc %d"
              % (np.dtype(dt).name, rep, a.value, rd / a.value / 1e9, b.value, (rd + wr) / b.value / 1e9, nz.value, rc))
