"""The device Fiat-Shamir layer as the GPU runs it: the cases of tests/fs_cases.py through the gfx950 build of tools/fscheck (compiled by
the package's build() with the library's own flags) against hashlib and the Python oracle, exact equality -- the only place where the
device BLAKE2s (one lane and the DPP quad form), StageWriter, ChaCha20, the rejection sampler and the verifier-only weights meet a
reference directly -- and black-box tests through the C ABI that a weight is APPLIED at every position of a group equation, of a chain
equation and to every element of a proof.  The probe cases also run under the emulator in tests/test_fs_emu.py."""
import pytest

import fs_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(mp):      # (mp: the package is imported first, so that torch's HIP runtime is in the process before the probe's)
    p = fc.Probe(fc.GPU_LIB)      # a missing probe library is an error, not a skip
    assert p.rt_name == "hip-gfx950", p.rt_name
    return p


def _report(result):
    fails, count = result
    assert count > 0
    assert not fails, "\n" + "\n".join(fails[:9])


def test_array_chacha_is_the_oracles():
    _report(fc.check_chacha_reference())


@pytest.mark.parametrize("mode", [0, 1], ids=["one-lane", "four-lane"])
def test_staged_blake2s_matches_hashlib(probe, mode):
    _report(fc.run_blake2s(probe, mode))


@pytest.mark.parametrize("lpp", fc.LPPS)
@pytest.mark.parametrize("curve", fc.CURVES)
def test_fsq_absorb_matches_hashlib(probe, curve, lpp):
    _report(fc.run_fsq_absorb(probe, curve, lpp))


def test_chacha20_block_matches_oracle(probe):
    _report(fc.run_chacha(probe))


@pytest.mark.parametrize("curve", fc.CURVES)
def test_rejection_classes_were_found(curve):
    _, found = fc.frstream_keys(curve)
    assert len(found) == (3 if curve in fc.REJECT_RUN else 0), found      # (secp256k1 rejects with probability ~2^-128: no such key exists)


@pytest.mark.parametrize("curve", fc.CURVES)
def test_fr_rand_matches_oracle(probe, curve):
    _report(fc.run_frstream(probe, curve))


@pytest.mark.parametrize("T", fc.CHAIN_T)
@pytest.mark.parametrize("curve", fc.CURVES)
def test_chain_weights_match_their_derivation(probe, curve, T):
    _report(fc.run_chain_weights(probe, curve, T))


@pytest.mark.parametrize("curve", fc.CURVES)
def test_chain_weights_depend_on_every_seed_of_their_table_only(probe, curve):
    _report(fc.run_chain_bit_flip(probe, curve))


@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("curve", fc.CURVES)
def test_screen_digests_and_weights(probe, curve, nw):
    _report(fc.run_screen_digest(probe, curve, nw))


@pytest.mark.parametrize("n", fc.MERGE_N)
@pytest.mark.parametrize("curve", fc.CURVES)
def test_merge_weights_match_on_one_and_four_lanes(probe, curve, n):
    _report(fc.run_merge_weights(probe, curve, n))


@pytest.mark.parametrize("mode,lpp", [(0, 0), (1, 4), (1, 16)], ids=["one-lane", "lpp4", "lpp16"])
@pytest.mark.parametrize("curve", fc.CURVES)
def test_merge_weights_depend_on_every_response_scalar(probe, curve, mode, lpp):
    _report(fc.run_merge_scalar_flips(probe, curve, mode, lpp))


# ---- black box: a weight is applied at every position ------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,m,n", fc.ELEMENT_SHAPES)
def test_every_proof_element_is_enforced_under_both_transcript_kernels(mp, coracle, curve, m, n):
    eng = mp._native.Engine(curve, 0)
    try:
        _report(fc.run_element_tamper(eng, coracle, curve, m, n))
    finally:
        eng.close()


@pytest.mark.parametrize("L", fc.GROUP_L)
def test_every_member_of_a_group_equation_is_enforced(mp, coracle, L):
    import torch
    eng = mp._native.Engine(fc.BB_CURVE, 0)
    try:
        _report(fc.run_group_members(eng, coracle, torch, torch.device("cuda", 0), L))
    finally:
        eng.close()


def test_every_link_of_a_chain_equation_is_enforced(mp, coracle):
    import torch
    eng = mp._native.Engine(fc.BB_CURVE, 0)
    try:
        _report(fc.run_chain_links(eng, coracle, torch, torch.device("cuda", 0), 65, 65))
    finally:
        eng.close()
