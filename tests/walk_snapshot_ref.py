"""Numpy restatement of the walk snapshot (include/cmpc.h, cmpc_walk_snapshot) for the tests: the arrays of one snapshot as host buffers with random bits in
them, the C struct over them, and the copy as fancy indexing."""
import ctypes as C

import numpy as np

import cmpc_amd as cm

# (key, per-problem shape as a function of (nx, np, M), dtype) in the order of the struct's pointer fields
FIELDS = (
    ("dState", lambda nx, n_p, M: (9,), np.float32), ("dP", lambda nx, n_p, M: (n_p,), np.float32), ("dX", lambda nx, n_p, M: (nx,), np.float32),
    ("dX0", lambda nx, n_p, M: (nx,), np.float32), ("dInfo", lambda nx, n_p, M: (8,), np.float32), ("dZmp", lambda nx, n_p, M: (2,), np.float32),
    ("dOk", lambda nx, n_p, M: (), np.int32), ("dLand", lambda nx, n_p, M: (2,), np.int32),
    ("dListT", lambda nx, n_p, M: (2, M, 2), np.float64), ("dListPose", lambda nx, n_p, M: (2, M, 7), np.float32), ("dListN", lambda nx, n_p, M: (2,), np.int32),
    ("dListTB", lambda nx, n_p, M: (2, M, 2), np.float64), ("dListPoseB", lambda nx, n_p, M: (2, M, 7), np.float32), ("dListNB", lambda nx, n_p, M: (2,), np.int32),
    ("dEndTick", lambda nx, n_p, M: (), np.int32), ("dEndCode", lambda nx, n_p, M: (), np.int32), ("dIterationsSum", lambda nx, n_p, M: (), np.int32),
    ("dIterationsMax", lambda nx, n_p, M: (), np.int32), ("dFinalState", lambda nx, n_p, M: (9,), np.float32), ("dBoxSlackMin", lambda nx, n_p, M: (), np.float32),
)
OPTIONAL = ("dX0", "dInfo", "dZmp")


def bits(a):
    """the array as unsigned words, so that NaN payloads and the sign of zero take part in a comparison"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def arrays(N, M, batch, rng=None, fill=None):
    """{field: array[batch, ...]}: random bits with NaN, -0.0 and infinities planted (rng), or every word the byte pattern `fill`"""
    L = cm.Layout(N)
    out = {}
    for k, shape, dt in FIELDS:
        shp = (batch,) + shape(L.nx, L.np, M)
        if rng is None:
            a = np.empty(shp, dt)
            a.view(np.uint8).reshape(-1)[:] = fill
        elif dt == np.int32:
            a = rng.integers(-5, 50, shp).astype(np.int32)
        else:
            a = rng.standard_normal(shp).astype(dt)
            flat = a.reshape(-1)
            pick = rng.integers(0, flat.size, max(3, flat.size // 17))
            flat[pick[0::3]] = np.nan
            flat[pick[1::3]] = -0.0
            flat[pick[2::3]] = np.inf
        out[k] = a
    return out


def struct(arr, tick=0, lists_in=0, without=()):
    """the cmpc_walk_snapshot over the arrays; the fields named in `without` are NULL"""
    s = cm._capi.CmpcWalkSnapshot()
    s.tick, s.lists_in = tick, lists_in
    for k, _, _ in FIELDS:
        setattr(s, k, None if k in without else arr[k].ctypes.data_as(C.c_void_p))
    return s


def expected(src, dst, index, src_batch, without=()):
    """(arrays of dst after the copy, ok): numpy fancy indexing where the index is valid, dst as it was elsewhere"""
    B = dst["dState"].shape[0]
    idx = np.arange(B) if index is None else np.asarray(index)
    good = (idx >= 0) & (idx < src_batch)
    out = {k: v.copy() for k, v in dst.items()}
    for k in out:
        if k not in without:
            out[k][good] = src[k][idx[good]]
    return out, good.astype(np.int32)
