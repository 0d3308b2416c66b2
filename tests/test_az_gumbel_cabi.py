"""K21 at the C boundary.  Without a GPU: the new entries are declared, exported and bound, the host forms refuse bad arguments, the Python layers
take the new arguments with defaults that reproduce the calls without them, and nothing falls back to the CPU.  With one (marked gpu): the
option's ranges, and its refusals against GMK_OPT_AZ_LEAVES and GMK_OPT_AZ_PROOF in both orders."""
import inspect
import os
import re

import numpy as np
import pytest

from gomokuai_amd import lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gmk_az_set_gumbel", "gmk_az_advance_gumbel", "gmk_az_root_choice_gumbel", "gmk_gumbel_sequence_host", "gmk_gumbel_setup_host",
         "gmk_gumbel_pick_host", "gmk_gumbel_move_host", "gmk_gumbel_row_host", "gmk_samples_from_records_target", "gmk_samples_from_packed_target",
         "gmk_replay_sample_target")
ERR_ARG, ERR_STATE = -3, -4


def test_entries_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "gomoku_hip.h")).read()
    declared = set(re.findall(r"\b(gmk_[a-z0-9_]+)\s*\(", text))
    L = G.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in G.EXPORTS, name
    assert "K21" in text and re.search(r"\bGMK_TARGET_VISITS = 0\b", text) and re.search(r"\bGMK_TARGET_POLICY = 1\b", text)
    assert (G.TARGET_VISITS, G.TARGET_POLICY) == (0, 1)
    rule = open(os.path.join(ROOT, "include", "gomoku_gumbel.h")).read()
    for name in ("gmk_gumbel_setup225", "gmk_gumbel_pick225", "gmk_gumbel_move225", "gmk_gumbel_row225", "gmk_gumbel_sequence", "gmk_gumbel_sum225"):
        assert re.search(r"\b%s\(" % name, rule), name
    assert "0x676d626cu" in rule                                 # 'gmbl'


def test_host_forms_refuse_bad_arguments():
    L = G.load()
    f32, u32, f64, u8, i32, i16, u16 = (np.zeros(225, t) for t in (np.float32, np.uint32, np.float64, np.uint8, np.int32, np.int16, np.uint16))
    p = lambda a: a.ctypes.data
    one = np.ones(1, np.int32)
    assert L.gmk_gumbel_setup_host(p(f32), p(u32), p(i32), p(u32), 1, 0, 1, None, p(f64), p(u32), p(u8), p(i32)) == ERR_ARG        # max_considered
    assert L.gmk_gumbel_setup_host(p(f32), p(u32), p(i32), p(u32), 1, 226, 1, None, p(f64), p(u32), p(u8), p(i32)) == ERR_ARG
    assert L.gmk_gumbel_setup_host(None, p(u32), p(i32), p(u32), 1, 4, 1, None, p(f64), p(u32), p(u8), p(i32)) == ERR_ARG           # a NULL row
    assert L.gmk_gumbel_setup_host(p(f32), p(u32), p(np.full(1, 226, np.int32)), p(u32), 1, 4, 1, None, p(f64), p(u32), p(u8), p(i32)) == ERR_ARG
    assert L.gmk_gumbel_setup_host(None, None, None, None, 0, 4, 1, None, None, None, None, None) == 0                                   # n = 0
    assert L.gmk_gumbel_pick_host(p(f32), p(u32), p(f32), p(f32), p(f64), p(u32), p(u8), p(one), 1, 0, 50.0, 1.0, p(i16)) == ERR_ARG   # n_sims
    assert L.gmk_gumbel_pick_host(p(f32), p(u32), p(f32), p(f32), p(f64), p(u32), p(u8), p(one), 1, 4097, 50.0, 1.0, p(i16)) == ERR_ARG
    assert L.gmk_gumbel_pick_host(p(f32), p(u32), p(f32), p(f32), p(f64), p(u32), p(u8), p(one), 1, 8, float("nan"), 1.0, p(i16)) == ERR_ARG
    assert L.gmk_gumbel_move_host(p(f32), p(u32), p(f32), p(f32), p(f64), p(u32), p(u8), 1, 50.0, float("inf"), p(i16)) == ERR_ARG
    assert L.gmk_gumbel_move_host(p(f32), p(u32), p(f32), p(f32), p(f64), p(u32), p(u8), -1, 50.0, 1.0, p(i16)) == ERR_ARG
    assert L.gmk_gumbel_row_host(p(f32), p(u32), p(f32), p(f32), 1, -1.0, 1.0, p(u16)) == ERR_ARG
    assert L.gmk_gumbel_row_host(p(f32), p(u32), p(f32), p(f32), 1, 50.0, 1.0, None) == ERR_ARG
    assert b"gmk_gumbel_row_host" in L.gmk_last_error()
    assert L.gmk_az_set_gumbel(None, 4, 16, 50.0, 1.0, 1, 0) == ERR_ARG
    assert L.gmk_az_root_choice_gumbel(None, None, None, None) == ERR_ARG
    assert L.gmk_az_advance_gumbel(None, None, None, None, None, 1, None, None) == ERR_ARG


def test_python_layer_is_there():
    from gomokuai_amd import selfplay
    assert inspect.signature(G.AlphaZeroMCTS.__init__).parameters["gumbel"].default is None
    assert inspect.signature(G.AlphaZeroMCTS.advance).parameters["gumbel"].default is False
    assert inspect.signature(G.AlphaZeroMCTS.root_choice).parameters["gumbel"].default is False
    assert callable(G.AlphaZeroMCTS.set_gumbel)
    for fn in (G.samples_from_records, G.samples_from_packed, G.ReplayHandle.sample, selfplay.GameRecords.to_samples):
        assert inspect.signature(fn).parameters["target"].default is None
    assert inspect.signature(selfplay.ReplayBuffer.__init__).parameters["target"].default == "visits"
    assert inspect.signature(selfplay.play_network_games).parameters["gumbel"].default is None


def test_play_network_games_refuses_what_does_not_go_with_gumbel():
    from gomokuai_amd import selfplay
    ok = dict(gumbel=(16, 50.0, 1.0), root_noise=None)
    for bad in (dict(leaves=2), dict(proof=True), dict(vcf_defend=True), dict(sample_plies=4)):
        with pytest.raises(ValueError, match="gumbel does not go with"):
            selfplay.play_network_games(4, None, 8, **dict(ok, **bad))
    with pytest.raises(ValueError, match="root_noise=None"):
        selfplay.play_network_games(4, None, 8, gumbel=(16, 50.0, 1.0))          # the default root noise
    with pytest.raises(ValueError, match="target"):
        selfplay.ReplayBuffer(4096, target="rows")


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = G.load()
    assert L.gmk_samples_from_records_target(None, None, None, None, None, None, 0, 0, 1, None, None, None, None) == ERR_STATE
    assert b"no CPU fallback" in L.gmk_last_error()
    assert L.gmk_replay_sample_target(None, 0, 0, 0, 1, 0, None, None, None, None, None, None) == ERR_STATE
    with pytest.raises(G.GmkError) as err:
        G.AlphaZeroMCTS(2, gumbel=(4, 16, 50.0, 1.0, 1, 0))
    assert "no CPU fallback" in str(err.value)


@pytest.mark.gpu
def test_option_ranges_and_refusals_in_both_orders():
    G.init()
    L = G.load()
    tree = G.AlphaZeroMCTS(2, node_capacity=256)
    for args in ((-1, 16, 50.0, 1.0), (226, 16, 50.0, 1.0), (4, 0, 50.0, 1.0), (4, 4097, 50.0, 1.0), (4, 16, float("nan"), 1.0), (4, 16, 50.0, -1.0), (4, 16, float("inf"), 1.0)):
        assert L.gmk_az_set_gumbel(tree.h, args[0], args[1], args[2], args[3], 1, 0) == ERR_ARG, args
    assert L.gmk_az_set_gumbel(tree.h, 0, -5, float("nan"), 0.0, 1, 0) == 0      # off: nothing else is read
    # the options first
    tree.set_option(G.OPT_AZ_LEAVES, 2)
    assert L.gmk_az_set_gumbel(tree.h, 4, 16, 50.0, 1.0, 1, 0) == ERR_STATE and b"GMK_OPT_AZ_LEAVES" in L.gmk_last_error()
    tree.set_option(G.OPT_AZ_LEAVES, 1)
    tree.set_option(G.OPT_AZ_PROOF, 1)
    assert L.gmk_az_set_gumbel(tree.h, 4, 16, 50.0, 1.0, 1, 0) == ERR_STATE and b"GMK_OPT_AZ_PROOF" in L.gmk_last_error()
    tree.set_option(G.OPT_AZ_PROOF, 0)
    # Gumbel first
    tree.set_gumbel(225, 4096)
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_LEAVES, 2) == ERR_STATE and b"gmk_az_set_gumbel" in L.gmk_last_error()
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_PROOF, 1) == ERR_STATE
    assert L.gmk_az_set_option(tree.h, G.OPT_AZ_LEAVES, 9) == ERR_ARG            # out of range stays an argument error
    tree.set_option(G.OPT_AZ_VCF_DEPTH, 8)                                       # composes
    tree.set_option(G.OPT_AZ_VCF_DEPTH, 0)
    tree.set_gumbel(0)
    tree.set_option(G.OPT_AZ_LEAVES, 2)                                          # off again: the options are free
    tree.set_option(G.OPT_AZ_LEAVES, 1)
    with pytest.raises(G.GmkError):
        G.AlphaZeroMCTS(2, node_capacity=256, proof=True, gumbel=(4, 16, 50.0, 1.0, 1, 0))
    tree.close()
