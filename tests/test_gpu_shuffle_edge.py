"""-m gpu: shuffle proofs on degenerate decks, witnesses and keys on the GPU -- the cases of tests/shuffle_edge_cases.py, which
tests/test_shuffle_edge_emu.py runs through the emulator: every class in one batch next to generic lanes, the prover under every plan
(latency batch, the six work splits with one and four lanes per group operation, Toom-Cook on and off, both transcript modes, the bucket
kernel forced) and the verifier under every strategy (merged and per equation, group equations on the wave kernel and on the split
pipeline, pipelined device pointers, explicit keys and key sets, chains), byte for byte and word for word against the C++ oracle -- on
every Toom-Cook node set, the Karatsuba path and m = 2 on the STARK curve, and on the other three base fields."""
import pytest

import shuffle_edge_cases as sec

pytestmark = pytest.mark.gpu


def _run(fn, *args):
    fails, checks = fn(*args)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


_ids = lambda s: "%s-%dx%d" % s


@pytest.mark.parametrize("shape", sec.SHAPES, ids=_ids)
def test_prover_matches_the_oracle_on_degenerate_inputs(mp, coracle, shape):
    import torch
    eng = mp._native.Engine(shape[0], 0)
    try:
        _run(sec.run_prover, eng, coracle, *shape, torch, "cuda:0")
    finally:
        eng.close()


@pytest.mark.parametrize("shape", sec.SHAPES, ids=_ids)
def test_verifier_matches_the_oracle_on_degenerate_inputs(mp, coracle, shape):
    import torch
    eng = mp._native.Engine(shape[0], 0)
    try:
        _run(sec.run_verifier, eng, coracle, *shape, torch, "cuda:0")
    finally:
        eng.close()
