"""The trainer's C-ABI (include/gomoku_hip.h, K11): the symbols exist, and without a device every entry returns GMK_ERR_STATE."""
import ctypes as C
import os
import re

import pytest

from gomokuai_amd import lib as G

TRAIN_SYMBOLS = ("gmk_train_create", "gmk_train_destroy", "gmk_train_forward", "gmk_train_grads", "gmk_train_step", "gmk_train_params",
                 "gmk_train_set_params", "gmk_train_get_block", "gmk_train_set_block", "gmk_train_set_step_count", "gmk_train_export", "gmk_train_info",
                 "gmk_train_kernel_gemm", "gmk_train_kernel_reduce", "gmk_train_kernel_im2col", "gmk_train_kernel_col2im")


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "..", "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\bint (gmk_train_\w+)\(", header))
    assert declared == set(TRAIN_SYMBOLS)
    L = G.load()
    for name in TRAIN_SYMBOLS:
        assert name in G.EXPORTS and getattr(L, name) is not None
    assert G.TRAIN_PARAMS == 326540 and sorted(G.TRAIN_BLOCK_ORDER) == sorted(name for name, _ in G.TRAIN_TENSORS)


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_init(0) == -1                                                  # GMK_ERR_NO_DEVICE
    h = C.c_void_p()
    assert L.gmk_train_create(*([None] * 16), 8, C.byref(h)) == -4              # GMK_ERR_STATE
    assert not h.value
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_train_forward(None, None, 1, None, None, None) == -4
    assert L.gmk_train_grads(None, None, None, None, 1, None, None, None) == -4
    assert L.gmk_train_step(None, None, None, None, 1, 1e-3, None, None, None, None) == -4
    assert L.gmk_train_params(*([None] * 17)) == -4
    assert L.gmk_train_set_params(*([None] * 17)) == -4
    assert L.gmk_train_get_block(None, 0, None) == -4
    assert L.gmk_train_set_block(None, 0, None) == -4
    assert L.gmk_train_set_step_count(None, 0) == -4
    assert L.gmk_train_export(None, None, None) == -4
    assert L.gmk_train_info(None, None, None, None, None) == -4
    assert L.gmk_train_kernel_gemm(C.byref(G.train_gemm_desc(M=1, N=1, K=1)), None) == -4
    assert L.gmk_train_kernel_gemm(None, None) == -4
    assert L.gmk_train_kernel_reduce(None, 1, 1, None, None) == -4
    assert L.gmk_train_kernel_im2col(None, 0, 0, 0, 0, 1, 1, None, None) == -4
    assert L.gmk_train_kernel_col2im(None, 1, 1, None, None, None) == -4
    assert L.gmk_train_destroy(None) == 0
    with pytest.raises(G.GmkError):
        G.TrainerHandle({name: __import__("numpy").zeros(shape, "float32") for name, shape in G.TRAIN_TENSORS}, 8)
