"""CPU tier: the inputs of tests/test_gpu_trees.py reach the conditions they are there for.  tests/model/trees_model.c runs the oracle's
compress_advanced through the oracle's test hook, unchanged in what it codes (its stream must be the oracle's), and counts the records a
way out hands to the tree wavefront; the figures in test_gpu_trees.py's docstring are these counters for each case's own input."""
import ctypes as C
import os

import pytest

import trees_cases
from csc_amd.capi import CscLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counted():
    """name -> the counters of the case's three inputs; every model stream compared with the oracle's"""
    mod = CscLib(trees_cases.build_model())
    orc = CscLib(os.path.join(ROOT, "oracle", "liborc.so"))
    mod.lib.orc_zero_alloc.restype = C.c_void_p
    orc.lib.orc_zero_alloc.restype = C.c_void_p
    zm, zo = mod.lib.orc_zero_alloc(), orc.lib.orc_zero_alloc()
    out = {}
    for name, (_, dict_size) in trees_cases.CASES.items():
        rows = []
        for data in trees_cases.streams_of(name):
            s, c = trees_cases.counts(mod, data, dict_size, zm)
            assert orc.encode(data, 3, dict_size, alloc=zo) == (0, s), f"{name}: the counting model's stream is not the oracle's"
            rows.append(c)
        out[name] = rows
    return out


def test_inputs_are_small():
    for name in trees_cases.CASES:
        n = len(trees_cases.CASES[name][0]())
        # (b) needs a distance beyond 2 MiB for its two-piece direct bits: the one input above 256 KB
        assert n <= (256 << 10) or name == "b_distance_classes", (name, n)
        assert n <= (2 << 20) + (128 << 10)


def test_a_many_records_on_the_same_cells(counted):
    c = counted["a_short_blocks"][0]
    assert c["wo_match_gt8"] >= 20 and c["most_match"] > 64, c
    assert c["same_len_cells"] > 1000 and c["same_slot_cells"] > 500 and c["same_low_cells"] > 100, c


def test_b_every_distance_class_in_one_run_of_eight(counted):
    c = counted["b_distance_classes"][0]
    assert c["dir0"] > 500 and c["dir1"] > 500 and c["dir2"] > 500, c
    assert c["runs8_all_classes"] > 100, c


def test_c_both_rings_wrap_inside_a_way_out(counted):
    c = counted["c_ring_wraps"][0]
    assert c["match_records"] > 64 and c["lit_records"] > 128, c
    assert c["lring_wraps_inside"] > 20 and c["mring_wraps_inside"] > 20, c
    assert c["exit_lit_on_ring_edge"] > 20, c


def test_d_more_literals_than_a_pass_with_repeated_pairs(counted):
    c = counted["d_literal_runs"][0]
    assert c["wo_lit_gt8"] > 100 and c["wo_lit_gt16"] > 100, c
    assert c["pair_repeats_in_eight"] > 1000 and c["pair_repeats_across_halves"] > 1000, c


def test_e_positions_without_a_window_between_windows(counted):
    name = "e_small_dictionary"
    assert trees_cases.CASES[name][1] < len(trees_cases.CASES[name][0]())          # the dictionary is smaller than the input
    c = counted[name][0]
    assert c["no_window"] > 5000 and c["no_window_runs_ge8"] > 100 and c["windows"] > 1000, c
    assert c["exit_lit_same_row"] > 100 and c["exit_lit_after_gt64"] > 10, c


def test_f_room_requests_and_refreshes_with_records_outstanding(counted):
    c = counted["f_long_stream"][0]
    assert c["queue_entries"] > 100 * 4096, c                                       # the coder's queue holds 4 096 entries
    assert c["refreshes"] > 20 and c["refreshes_early_after_records"] > 5, c
    assert c["exit_lit_after_gt64"] > 100, c
