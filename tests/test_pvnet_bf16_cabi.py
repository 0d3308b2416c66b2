""""K9 in bf16" at the C-ABI, without a device: the three entries exist and are declared, and their argument errors come back before anything
touches a GPU."""
import ctypes as C
import os
import re

import numpy as np

from gomokuai_amd import lib as G

_NEW = ("gmk_pvnet_set_precision", "gmk_pvnet_get_precision", "gmk_bf16_round_host")
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gomoku_hip.h")


def test_exports_exist_and_are_declared():
    lib = G.load()
    text = open(_HEADER).read()
    for name in _NEW:
        assert name in G.EXPORTS
        assert getattr(lib, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"GMK_PVNET_F32\s*=\s*0\b", text) and re.search(r"GMK_PVNET_BF16\s*=\s*1\b", text)
    assert (G.PVNET_F32, G.PVNET_BF16) == (0, 1) and G.PVNET_PRECISIONS == {"f32": 0, "bf16": 1}
    assert "K9 in bf16" in text


def test_argument_errors_without_a_device():
    lib = G.load()
    err_arg = -3
    out = C.c_int(77)
    assert lib.gmk_pvnet_set_precision(None, G.PVNET_BF16) == err_arg
    assert b"gmk_pvnet_set_precision" in lib.gmk_last_error()
    assert lib.gmk_pvnet_set_precision(None, G.PVNET_F32) == err_arg
    assert lib.gmk_pvnet_set_precision(None, 2) == err_arg
    assert lib.gmk_pvnet_get_precision(None, C.byref(out)) == err_arg and out.value == 77
    assert b"gmk_pvnet_get_precision" in lib.gmk_last_error()
    src, dst = np.ones(4, np.float32), np.zeros(4, np.uint16)
    assert lib.gmk_bf16_round_host(None, 4, dst.ctypes.data) == err_arg
    assert lib.gmk_bf16_round_host(src.ctypes.data, 4, None) == err_arg
    assert b"gmk_bf16_round_host" in lib.gmk_last_error()
    assert (dst == 0).all()
    assert lib.gmk_bf16_round_host(src.ctypes.data, 4, dst.ctypes.data) == 0 and (dst == 0x3F80).all()


def test_fused_network_rejects_an_unknown_precision_before_the_device():
    """FusedPolicyValueNetwork(precision=) is checked before gmk_init: a typo is a ValueError on any machine"""
    import pytest
    from gomokuai_amd.network import FusedPolicyValueNetwork, PolicyValueNetwork
    with pytest.raises(ValueError):
        FusedPolicyValueNetwork(PolicyValueNetwork(seed=0), precision="fp16")
