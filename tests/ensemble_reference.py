"""Test-side restatement of K13's merge of root tables (include/gomoku_hip.h, "K13"), in numpy: what tests/test_ensemble.py holds the host
function to and tests/test_ensemble_gpu.py the device kernels, bit for bit."""
import numpy as np

LIMIT = 1 << 24


def numpy_merge(group, visits, values, root_visits=None, root_values=None):
    """The merge of include/gomoku_hip.h (K13) restated: int64 sums of np.rint(n * q * 2^24) in float64, one float64 division chain, a cast
    to float32.  A replica with a count of 2^24 or more adds nothing and sets status bit 1; a uint32 output whose sum passed 2^32 - 1 holds
    2^32 - 1 and sets status bit 2 (the sums themselves stay exact)."""
    n = np.asarray(visits, np.uint32).reshape(-1, group, 225).astype(np.int64)
    q = np.asarray(values, np.float32).reshape(-1, group, 225).astype(np.float64)
    E = n.shape[0]
    rn = np.zeros((E, group), np.int64) if root_visits is None else np.asarray(root_visits, np.uint32).reshape(E, group).astype(np.int64)
    rq = np.zeros((E, group), np.float64) if root_values is None else np.asarray(root_values, np.float32).reshape(E, group).astype(np.float64)
    bad = (n >= LIMIT).any(axis=2) | (rn >= LIMIT)
    keep = ~bad
    n = n * keep[:, :, None]
    rn = rn * keep
    N = n.sum(axis=1)
    S = np.rint(n.astype(np.float64) * q * 2.0 ** 24).astype(np.int64).sum(axis=1)
    RN = rn.sum(axis=1)
    RS = np.rint(rn.astype(np.float64) * rq * 2.0 ** 24).astype(np.int64).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(N > 0, (S.astype(np.float64) / 2.0 ** 24 / N.astype(np.float64)), 0.0).astype(np.float32)
        rval = np.where(RN > 0, (RS.astype(np.float64) / 2.0 ** 24 / RN.astype(np.float64)), 0.0).astype(np.float32)
    cells = np.where(N.max(axis=1) > 0, N.argmax(axis=1), -1).astype(np.int16)          # argmax: the first maximum
    top = 0xFFFFFFFF
    status = bad.any(axis=1) * 2 + ((N > top).any(axis=1) | (RN > top)) * 4
    return {"visits": np.minimum(N, top).astype(np.uint32), "values": val, "cells": cells, "root_visits": np.minimum(RN, top).astype(np.uint32),
            "root_value": rval, "status": status.astype(np.int32)}


def assert_same(got, want, where=""):
    for k in ("visits", "cells", "root_visits", "status"):
        np.testing.assert_array_equal(got[k], want[k], "%s %s" % (where, k))
    for k in ("values", "root_value"):
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), "%s %s (bits)" % (where, k))
