"""The wire-form entries of the C-ABI (gmk_records_scan / _packed_bytes / _pack / _unpack, gmk_samples_from_packed) are declared,
exported and refuse to run without a device: no CPU fallback."""
import ctypes as C
import os
import re

import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIRE = ["gmk_records_scan", "gmk_records_packed_bytes", "gmk_records_pack", "gmk_records_unpack", "gmk_samples_from_packed"]


def test_wire_entries_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in WIRE:
        assert name in declared, name
        assert name in G.EXPORTS, name
        assert hasattr(L, name), name


def test_wire_entries_refuse_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_init(0) == -1                      # GMK_ERR_NO_DEVICE
    refused = (-1, -4)                              # GMK_ERR_NO_DEVICE, GMK_ERR_STATE
    b = C.c_uint64(12345)
    assert L.gmk_records_scan(None, 4, None, None) in refused
    assert L.gmk_records_packed_bytes(None, 4, 1, C.byref(b), None) in refused
    assert b.value == 12345
    assert L.gmk_records_pack(None, None, None, None, 4, None, None, 0, None, None) in refused
    assert L.gmk_records_unpack(None, 0, 4, 1, None, None, None, None, None, None, None) in refused
    assert L.gmk_samples_from_packed(None, 4, None, None, None, 4, 0, None, None, None, None) in refused
    assert b"no CPU fallback" in L.gmk_last_error()
    with pytest.raises(G.GmkError):
        G.records_packed_bytes(None, 4, True)
