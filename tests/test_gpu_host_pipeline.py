"""-m gpu: the chunked host-buffer calls on the GPU -- the cases of tests/host_pipeline_cases.py, which tests/test_host_pipeline_emu.py
runs at tiny sizes through the emulator.  Only here are the copies asynchronous (with buffers from mp_host_alloc), so only here can a
missing wait between the upload, kernel and download streams corrupt a staging buffer; and only here do the sizes reach the ramp of a
1 024-proof chunk, the verifier's rounding to 1 024, its "two halves" and "what is left" branches and the 52-card offsets.  Every
expectation is one device-resident call's, held to the C++ oracle at the chunk edges, and is made before the call under test."""
import pytest

import host_pipeline_cases as hp

pytestmark = pytest.mark.gpu

STARK = ("stark", 2, 3)
CARDS52 = ("stark", 2, 26)
TINY = [(4, 11), (8, 16), (8, 20), (8, 27), (9, 19)]
_cb = lambda v: "C%d-B%d" % v
_kind = lambda p: "page-locked" if p else "pageable"


def _run(mp, curve, want, fn, coracle, *args, **kw):
    import torch
    eng = mp._native.Engine(curve, 0)
    try:
        fails, checks = fn(eng, coracle, *(((torch, "cuda:0") if fn is not hp.run_schedule else ()) + args), **kw)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks == want


def test_schedule_model_is_the_librarys(mp, coracle):
    _run(mp, "stark", hp.schedule_count(), hp.run_schedule, coracle)


@pytest.mark.parametrize("cb", TINY + [(1024, 2047)], ids=_cb)
def test_prover_returns_every_row_under_every_schedule(mp, coracle, cb):
    """the even cut (C = 4; C = 1 024 with B = 2 047, the last B before the ramp) and the ramp at tiny sizes"""
    _run(mp, "stark", hp.prover_count(*cb), hp.run_prover, coracle, *STARK, *cb)


@pytest.mark.parametrize("pinned", [False, True], ids=_kind)
def test_prover_ramp_of_twelve_chunks(mp, coracle, pinned):
    """9 216 proofs of 52 cards in chunks of 1 024: 128 384 1 024 x 8 384 128.  With page-locked buffers this is the case meant to be
    sensitive to a missing wait: the kernels of a 1 024-proof chunk should outlast the upload of the next chunk by a wide margin (173 k
    proofs/s at 1 024 in flight against ~13 KB uploaded per proof: ~6 ms of kernels, well under 1 ms of copies), so an upload that
    does not wait for `done` lands in buffers the kernels still read.  Nobody has measured that margin for this purpose; the test asserts
    bytes, never times."""
    assert len(hp.model_schedule(9216, 1024, False)) == 12
    _run(mp, "stark", hp.prover_count(1024, 9216, pinned=(pinned,)), hp.run_prover, coracle, *CARDS52, 1024, 9216, pinned=(pinned,))


def test_prover_and_verifier_on_96_byte_points(mp, coracle):
    _run(mp, "bls12_377", hp.prover_count(8, 20), hp.run_prover, coracle, "bls12_377", 2, 3, 8, 20)


@pytest.mark.parametrize("shape,cb", [(STARK, (8, 27)), (CARDS52, (1024, 2048))], ids=["6-cards-C8-B27", "52-cards-C1024-B2048"])
def test_keyed_batches_across_chunks(mp, coracle, shape, cb):
    _run(mp, shape[0], hp.prover_count(*cb, keyed=True), hp.run_prover, coracle, *shape, *cb, keyed=True)


def test_seeded_witnesses_across_chunks_tiny(mp, coracle):
    _run(mp, "stark", hp.prover_count(8, 27, seeded=True), hp.run_prover, coracle, *STARK, 8, 27, seeded=True)


def test_seeded_witnesses_across_nine_chunks_page_locked(mp, coracle):
    """the permutations and factors go back from st.perm / st.in1, which the sampler of the next-but-one chunk overwrites"""
    assert len(hp.model_schedule(6144, 1024, False)) >= 5
    _run(mp, "stark", hp.prover_count(1024, 6144, seeded=True, pinned=(True,)), hp.run_prover, coracle, *CARDS52, 1024, 6144, seeded=True,
         pinned=(True,))


def test_bad_witnesses_at_every_chunk_edge(mp, coracle):
    _run(mp, "stark", hp.bad_witness_count(8, 27), hp.run_bad_witness, coracle, *STARK, 8, 27)


@pytest.mark.parametrize("cb", TINY, ids=_cb)
def test_verifier_defects_at_every_chunk_edge(mp, coracle, cb):
    modes = hp.MODES if cb == (8, 20) else hp.MODES[:2]       # (20, 8): 1 8 6 5 -- the chunk of 1 takes no group, the others do
    _run(mp, "stark", hp.verifier_count(*cb, modes=modes), hp.run_verifier, coracle, *STARK, *cb, modes=modes)


@pytest.mark.parametrize("B", [37648, 16384])
def test_verifier_schedule_that_grows_by_half(mp, coracle, B):
    """C = 8 192: 1 024 2 048 3 072 5 120 8 192 8 192 5 000 5 000 (the rounding to 1 024 and the two halves) and 1 024 2 048 3 072 5 120
    5 120 (what is left)"""
    _run(mp, "stark", hp.verifier_count(8192, B, modes=hp.MODES[:2]), hp.run_verifier, coracle, *STARK, 8192, B, modes=hp.MODES[:2])


def test_verifier_on_the_52_card_ramp(mp, coracle):
    _run(mp, "stark", hp.verifier_count(1024, 9216, modes=hp.MODES[:1]), hp.run_verifier, coracle, *CARDS52, 1024, 9216, modes=hp.MODES[:1])


def test_pipeline_setting_leaves_the_host_calls_alone(mp, coracle):
    _run(mp, "stark", hp.pipeline_count(20), hp.run_pipeline_setting, coracle, *STARK, 8, 20)


def test_staging_buffers_shared_with_chain_slices(mp, coracle):
    _run(mp, "stark", hp.staging_count(), hp.run_shared_staging, coracle, *STARK)
