"""Builds tests/ecg_hostmath/ecg_hostmath.cpp (the host restatement of houv_knn_feat) with g++ and loads it through ctypes.
Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    out = os.path.join(_HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libecg_hostmath.so")
    src = os.path.join(_HERE, "ecg_hostmath.cpp")
    if (not os.path.exists(so)) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


def knn_feat(x, k, C=None):
    """x[B,N,ld] fp32 (the first C columns of a row are the features; C defaults to ld) -> (idx[B,N,k] int32, dist2[B,N,k] fp32)
    of hm_knn_feat."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, N, ld = x.shape
    C = ld if C is None else C
    assert 1 <= k <= N and 1 <= C <= ld
    idx = np.zeros((B, N, k), np.int32)
    dist = np.zeros((B, N, k), np.float32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    load().hm_knn_feat(x.ctypes.data_as(fp), B, N, C, ld, k, idx.ctypes.data_as(ip), dist.ctypes.data_as(fp))
    return idx, dist
