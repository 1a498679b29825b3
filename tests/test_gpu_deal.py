"""-m gpu: dealing and seating on the GPU -- mp_mask_batch, mp_verify_mask_batch, mp_verify_mask_batch_dev, mp_aggregate_keys_batch and
their mirrors -- on all four curves.  The cases are those of tests/deal_cases.py, which tests/test_deal_emu.py runs through the emulator:
(cards, keys) = (1, 1), (63, 3), (64, 3), (65, 7), (257, 16) and, on the STARK curve, (52, 1), masking and remasking, with edge factors and
edge cards spread over the lanes; (tables, players) = (1, 1), (7, 9), (8, 8), (13, 5), (257, 1) with edge keys; one defect per lane;
points outside the subgroup (BLS12-377); agreement with mp_msm, mp_remask_batch, mp_sigma_prove_batch and mp_sigma_verify_batch; the
device-pointer form on the output of a shuffle prover; DLCards.deal / verify_deal / compute_aggregate_keys against the single-element
members; two host threads on one table; examples/deal.py."""
import os
import subprocess
import sys
import threading

import pytest

import deal_cases as dc
from conftest import ROOT

pytestmark = pytest.mark.gpu

CURVES = dc.CURVES


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


def _run(fn, *args):
    fails, checks = fn(*args)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


@pytest.mark.parametrize("curve", CURVES)
def test_mask_and_verify_match_the_oracle(engines, coracle, curve):
    _run(dc.run_honest, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_aggregate_keys_match_the_oracle(engines, coracle, curve):
    _run(dc.run_seating, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_tiny_batch_matches_the_python_oracle(engines, coracle, curve):
    _run(dc.run_python_oracle, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_one_defect_per_lane_and_call_level_refusals(engines, coracle, curve):
    _run(dc.run_defects, engines(curve), coracle, curve)


def test_points_outside_the_subgroup_bls12_377(engines, coracle):
    _run(dc.run_subgroup, engines("bls12_377"), coracle)


@pytest.mark.parametrize("curve", CURVES)
def test_agreement_with_the_composed_calls(engines, coracle, curve):
    _run(dc.run_agreement, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_device_pointer_form_on_a_prover_s_output_deck(engines, coracle, curve):
    import torch
    _run(dc.run_dev, engines(curve), coracle, curve, torch, "cuda")


def test_two_host_threads_verify_on_one_table(engines, coracle):
    _run(dc.run_threads, engines("stark"), coracle, "stark", threading)


@pytest.mark.parametrize("curve", CURVES)
def test_dlcards_batched_dealing_against_the_single_element_members(mp, curve):
    """10 players at two tables of five and 4 cards: compute_aggregate_keys, deal / verify_deal and deal_remask / verify_deal_remask give,
    element by element, what compute_aggregate_key, mask / verify_mask and remask / verify_remask give; one bad element has the member's
    error and leaves the others intact"""
    M, N_ = (4, 13) if curve == "stark" else (2, 3)
    cards = mp.DLCards(curve, device=0)
    pp = cards.setup(bytes(range(32)), M, N_)
    rng = mp.ChaCha20Rng(b"\x12" * 32)
    players = [cards.player_keygen(rng, pp) for _ in range(10)]
    rows = [(pk, cards.prove_key_ownership(bytes([i]) * 32, pp, pk, sk, b"info %d" % i), b"info %d" % i) for i, (pk, sk) in enumerate(players)]
    tables = [rows[:5], rows[5:]]
    joint = cards.compute_aggregate_keys(pp, tables)
    assert joint == [cards.compute_aggregate_key(pp, t) for t in tables]
    bad = [rows[:5], rows[5:7] + [(rows[7][0], rows[7][1], b"somebody else")] + rows[8:]]
    got = cards.compute_aggregate_keys(pp, bad)
    assert got[0] == joint[0] and got[1] == mp.CardProtocolError("ProofVerificationError", mp.CryptoError("Schnorr Identification"))
    with pytest.raises(mp.CardProtocolError) as e:
        cards.compute_aggregate_key(pp, bad[1])
    assert e.value == got[1]

    G = pp.enc_parameters
    t = cards.table(pp, G)
    plain = [t.msm(1, 1, mp.fr_rand(curve, rng).to_bytes(32, "little"), G) for _ in range(4)]
    key_index = [0, 1, 1, 0]
    factors = [mp.fr_rand(curve, rng) for _ in range(4)]
    seeds = [bytes([0x60 + i]) * 32 for i in range(4)]
    dealt = cards.deal(seeds, pp, joint, key_index, plain, factors)
    assert dealt == [cards.mask(seeds[i], pp, joint[key_index[i]], plain[i], factors[i]) for i in range(4)]
    masked, proofs = [d[0] for d in dealt], [d[1] for d in dealt]
    assert cards.verify_deal(pp, joint, key_index, plain, masked, proofs) == [None] * 4
    for i in range(4):
        assert cards.verify_mask(pp, joint[key_index[i]], plain[i], masked[i], proofs[i]) is None
    swapped = [plain[0], plain[2], plain[1], plain[3]]
    verdicts = cards.verify_deal(pp, joint, key_index, swapped, masked, proofs)
    assert verdicts == [None, mp.CryptoError("Chaum-Pedersen"), mp.CryptoError("Chaum-Pedersen"), None]
    with pytest.raises(mp.CryptoError) as e:
        cards.verify_mask(pp, joint[1], plain[2], masked[1], proofs[1])
    assert e.value == verdicts[1]

    alphas = [mp.fr_rand(curve, rng) for _ in range(4)]
    seeds2 = [bytes([0x70 + i]) * 32 for i in range(4)]
    again = cards.deal_remask(seeds2, pp, joint, key_index, masked, alphas)
    assert again == [cards.remask(seeds2[i], pp, joint[key_index[i]], masked[i], alphas[i]) for i in range(4)]
    remasked, proofs2 = [d[0] for d in again], [d[1] for d in again]
    assert cards.verify_deal_remask(pp, joint, key_index, masked, remasked, proofs2) == [None] * 4
    for i in range(4):
        assert cards.verify_remask(pp, joint[key_index[i]], masked[i], remasked[i], proofs2[i]) is None
    verdicts = cards.verify_deal_remask(pp, joint, [0, 1, 0, 0], masked, remasked, proofs2)
    assert verdicts == [None, None, mp.CryptoError("Chaum-Pedersen"), None]
    with pytest.raises(mp.CryptoError) as e:
        cards.verify_remask(pp, joint[0], masked[2], remasked[2], proofs2[2])
    assert e.value == verdicts[2]


def test_deal_example_runs_end_to_end():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "deal.py")], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    text = out.stdout.decode()
    assert "32 players seated at 8 tables" in text and "416 cards dealt" in text and text.strip().endswith("deal ok"), text
