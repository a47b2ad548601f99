"""A compiled C caller of predict_X_old_collective_explicit / _implicit: include/cmfrec_hip.h as C99 (-pedantic -Werror), linked
against libcmfrec_hip_double.so, on a 5 x 7 model with k_user, k_item and k_main non-zero; the printed values are checked against
the exact ones (tests/predict_reference.py)."""
import os
import subprocess

import numpy as np
import pytest

import predict_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_caller", "predict_caller.c")
M, N, K, K_USER, K_ITEM, K_MAIN = 5, 7, 3, 2, 1, 2


def build_caller(tmp_path):
    exe = str(tmp_path / "predict_caller")
    libdir = os.path.join(ROOT, "cmfrec_amd", "lib")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", libdir, "-lcmfrec_hip_double", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def model():
    """The caller's model, restated: exact multiples of 1/8, 1/4 and 1/16."""
    lda, ldb = K_USER + K + K_MAIN, K_ITEM + K + K_MAIN
    i, j = np.arange(M)[:, None], np.arange(lda)[None, :]
    A = (((i * 7 + j * 3) % 11) - 5) / 8.0
    i, j = np.arange(N)[:, None], np.arange(ldb)[None, :]
    B = (((i * 5 + j * 2) % 13) - 6) / 8.0
    biasA, biasB = (np.arange(M) - 2) / 4.0, (3 - np.arange(N)) / 16.0
    row = np.array([0, 4, 2, 2, 1, 3, 5, 0, 4, 3], np.int32); col = np.array([0, 6, 3, 3, 5, 1, 2, 7, 0, 4], np.int32)
    return A, B, biasA, biasB, 1.5, row, col


def test_predict_caller_compiles_and_links(tmp_path):
    assert os.path.exists(build_caller(tmp_path))


@pytest.mark.gpu
def test_c_caller_predicts(tmp_path):
    exe = build_caller(tmp_path)
    lines = subprocess.check_output([exe]).decode().strip().splitlines()
    assert len(lines) == 2
    A, B, bA, bB, gm, row, col = model()
    As, Bs = np.ascontiguousarray(A[:, K_USER:]), np.ascontiguousarray(B[:, K_ITEM:])
    for line, implicit in zip(lines, (False, True)):
        f = line.split()
        assert int(f[0]) == 0
        got = np.array([float(x) for x in f[1:]], np.float64)
        ops = (As, Bs, None, None, 0.0) if implicit else (As, Bs, bA, bB, gm)
        scored = pr.exact(*ops, row, col, implicit)[2]
        assert (~scored).sum() == 2
        pr.check(got, *ops, row, col, implicit=implicit, what="C caller")
