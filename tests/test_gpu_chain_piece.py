"""-m gpu: chains of different lengths verified in passes of equal pieces, on the GPU -- mp_verify_shuffle_chain_ragged[_dev],
mp_set_chain_pieces, mp_chain_ragged_stats.  The cases are those of tests/chain_piece_cases.py, which tests/test_chain_piece_emu.py runs
through the emulator, and the rows of a 52-card deck (6 656 and 6 368 bytes: many waves per row) on top.  The _dev cases matter here:
only asynchronous copies and launches can show a missing ordering between the gather, the pass, the final scatter and mp_sync."""
import pytest

import chain_piece_cases as cp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(mp):
    cache = {}

    def get(curve):
        if curve not in cache:
            cache[curve] = mp._native.Engine(curve, 0)
        return cache[curve]
    yield get
    for e in cache.values():
        e.close()


def _run(fn, *args, **kw):
    fails, checks = fn(*args, **kw)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


@pytest.mark.parametrize("keyed", [False, True], ids=["own key", "keys per link"])
def test_honest_chains_in_both_modes_from_host_and_device_buffers(engines, coracle, keyed):
    """the first case: fails without mp_verify_shuffle_chain_ragged_dev, mp_set_chain_pieces and mp_chain_ragged_stats"""
    import torch
    _run(cp.run_honest, engines("stark"), coracle, keyed, torch, "cuda")


def test_the_cases_reach_their_edges_and_the_model_restates_the_source():
    assert not cp.edge_failures()


@pytest.mark.parametrize("name", cp.DEFECTS)
def test_defects_at_piece_boundaries_fail_their_links_alone(engines, coracle, name):
    import torch
    _run(cp.run_defect, engines("stark"), coracle, name, True, torch, "cuda", settings=name == cp.DEFECTS[0])


def test_defects_on_a_table_with_its_own_key(engines, coracle):
    import torch
    _run(cp.run_defect, engines("stark"), coracle, cp.DEFECTS[1], False, torch, "cuda")


@pytest.mark.parametrize("keyed", [False, True], ids=["own key", "keys per link"])
def test_equal_lengths_give_the_words_of_the_uniform_call(engines, coracle, keyed):
    _run(cp.run_equal, engines("stark"), coracle, keyed)


def test_rows_of_96_byte_points(engines, coracle):
    import torch
    _run(cp.run_width, engines("bls12_377"), coracle, "bls12_377", cp.MN, cp.BLS_LINKS, torch, "cuda")


def test_rows_of_a_52_card_deck(engines, coracle):
    import torch
    _run(cp.run_width, engines("stark"), coracle, "stark", cp.WIDE_MN, cp.WIDE_LINKS, torch, "cuda")


def test_refused_calls_touch_nothing(engines, coracle):
    import torch
    _run(cp.run_refusals, engines("stark"), coracle, torch, "cuda")
