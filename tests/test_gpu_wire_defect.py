"""-m gpu: malformed wire inputs to the shuffle calls on the GPU -- the cases of tests/wire_defect_cases.py, which
tests/test_wire_defect_emu.py runs in part through the emulator.  The verifier with a defect at every point and scalar of a proof, at
every point of both decks and in the per-proof key on all four base fields; every one of those lanes again under merged and
per-equation verification, group equations of 3 and 65 with and without refinement and the pipelined lane, chains, and mp_set_validated
on BLS12-377; the prover's masking factors, deck points, permutations and keys with N on both sides of the 64-lane stride of
k_prove_init_w, and in one call of 32 769 proofs on k_prove_init.  Every expectation is the C++ oracle's (or, for points outside the
subgroup, the header's, checked in Python integers) and is made before the device is asked."""
import pytest

import wire_defect_cases as wd

pytestmark = pytest.mark.gpu

_ids = lambda s: "%s-%dx%d" % s


def _run(mp, curve, want, fn, *args, **kw):
    eng = mp._native.Engine(curve, 0)
    try:
        fails, checks = fn(eng, *args, **kw)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks == want


@pytest.mark.parametrize("shape", wd.VERIFIER_SHAPES, ids=_ids)
def test_verifier_refuses_a_defect_at_every_position(mp, coracle, shape):
    _run(mp, shape[0], wd.positions_count(*shape), wd.run_verifier_positions, coracle, *shape)


@pytest.mark.parametrize("shape", wd.VERIFIER_SHAPES, ids=_ids)
def test_verifier_refuses_bad_keys(mp, coracle, shape):
    import torch
    _run(mp, shape[0], wd.keys_count(shape[0]), wd.run_verifier_keys, coracle, *shape, torch, "cuda:0")


@pytest.mark.parametrize("shape", wd.STRATEGY_SHAPES, ids=_ids)
def test_strategies_keep_the_words(mp, coracle, shape):
    import torch
    _run(mp, shape[0], wd.strategies_count(*shape), wd.run_strategies, coracle, *shape, torch, "cuda:0")


@pytest.mark.parametrize("shape", wd.STRATEGY_SHAPES, ids=_ids)
def test_chains_keep_the_words(mp, coracle, shape):
    _run(mp, shape[0], wd.chain_count(), wd.run_chain, coracle, *shape)


def test_validated_ranges_end_where_they_should(mp, coracle):
    import torch
    _run(mp, "bls12_377", wd.validated_count(), wd.run_validated, coracle, torch, "cuda:0")


@pytest.mark.parametrize("shape", wd.PROVER_SHAPES, ids=_ids)
def test_prover_refuses_malformed_witnesses_and_decks(mp, coracle, shape):
    _run(mp, shape[0], wd.prover_count(*shape), wd.run_prover, coracle, *shape)


def test_lone_lane_permutation_check(mp, coracle):
    _run(mp, "stark", wd.lone_lane_count(), wd.run_prover_lone_lane, coracle)


@pytest.mark.parametrize("shape", [("stark", 2, 3), ("bls12_377", 2, 3)], ids=_ids)
def test_prover_refuses_bad_keys(mp, coracle, shape):
    _run(mp, shape[0], wd.prover_keys_count(shape[0]), wd.run_prover_keys, coracle, *shape)
