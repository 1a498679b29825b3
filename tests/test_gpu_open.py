"""-m gpu: the opening phase on the GPU -- mp_reveal_batch, mp_unmask_batch, mp_unmask_batch_dev and their mirrors -- on all four curves.
The cases are those of tests/open_cases.py, which tests/test_open_emu.py runs through the emulator: (C cards, T tokens) = (1, 1), (7, 9),
(8, 8), (13, 5), (257, 1) and, on the STARK curve, (52, 4), with edge keys and edge cards spread over the lanes; one defect per card;
points outside the subgroup (BLS12-377); agreement with mp_msm, mp_sigma_prove_batch and mp_sigma_verify_batch; the device-pointer form;
DLCards.compute_reveal_tokens / open_cards against the single-card members; two host threads on one table; examples/showdown.py."""
import os
import subprocess
import sys
import threading

import pytest

import open_cases as oc
from conftest import ROOT

pytestmark = pytest.mark.gpu

CURVES = oc.CURVES


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
def test_reveal_and_unmask_match_the_oracle(engines, coracle, curve):
    _run(oc.run_honest, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_tiny_batch_matches_the_python_oracle(engines, coracle, curve):
    _run(oc.run_python_oracle, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_one_defect_per_card_and_call_level_refusals(engines, coracle, curve):
    _run(oc.run_defects, engines(curve), coracle, curve)


def test_points_outside_the_subgroup_bls12_377(engines, coracle):
    _run(oc.run_subgroup, engines("bls12_377"), coracle)


@pytest.mark.parametrize("curve", CURVES)
def test_agreement_with_the_sigma_calls(engines, coracle, curve):
    _run(oc.run_agreement, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_device_pointer_form_gives_the_same_outputs(engines, coracle, curve):
    import torch
    _run(oc.run_dev, engines(curve), coracle, curve, torch, "cuda")


@pytest.mark.parametrize("curve", CURVES)
def test_dlcards_batched_opening_against_the_single_card_members(mp, curve):
    """the flow of test_gpu_protocol.py::test_verify_masking_remasking_reveal_unmask with 10 players and 4 cards: the batched members
    give the tokens, proofs and plaintexts of compute_reveal_token / unmask, and a bad token fails its card alone, with unmask's error"""
    M, N_ = (4, 13) if curve == "stark" else (2, 3)
    cards = mp.DLCards(curve, device=0)
    pp = cards.setup(bytes(range(32)), M, N_)
    rng = mp.ChaCha20Rng(b"\x11" * 32)
    players = [cards.player_keygen(rng, pp) for _ in range(10)]
    agg = cards.compute_aggregate_key(pp, [(pk, cards.prove_key_ownership(bytes([i]) * 32, pp, pk, sk, b"info"), b"info")
                                           for i, (pk, sk) in enumerate(players)])
    rng = mp.ChaCha20Rng(b"\x31" * 32)
    G = pp.enc_parameters
    t = cards.table(pp, G)
    plain = [t.msm(1, 1, mp.fr_rand(curve, rng).to_bytes(32, "little"), G) for _ in range(4)]
    masked = [cards.remask(bytes([0x42 + i]) * 32, pp, agg, cards.mask(bytes([0x41 + i]) * 32, pp, agg, p, mp.fr_rand(curve, rng))[0],
                           mp.fr_rand(curve, rng))[0] for i, p in enumerate(plain)]
    T = len(players)
    signer = [j for _ in masked for j in range(T)]
    seeds = [bytes([0x50 + l]) * 32 for l in range(len(signer))]
    got = cards.compute_reveal_tokens(seeds, pp, players, masked, signer)
    single = [cards.compute_reveal_token(seeds[c * T + j], pp, players[j][1], players[j][0], masked[c]) for c in range(4) for j in range(T)]
    assert got == single
    keys = [pk for pk, _ in players]
    card_list = [plain[2], plain[0], plain[3]]
    opened = cards.open_cards(pp, keys, masked, signer, [g[0] for g in got], [g[1] for g in got], card_list)
    assert opened == [(plain[0], 1), (plain[1], None), (plain[2], 0), (plain[3], 2)]
    for c in range(4):
        assert cards.unmask(pp, [(got[c * T + j][0], got[c * T + j][1], keys[j]) for j in range(T)], masked[c]) == plain[c]
    toks = [g[0] for g in got]
    toks[1 * T + 4] = t.msm(1, 1, (7).to_bytes(32, "little"), G)
    opened = cards.open_cards(pp, keys, masked, signer, toks, [g[1] for g in got], card_list)
    assert opened[1] == mp.CardProtocolError("ProofVerificationError", mp.CryptoError("Chaum-Pedersen"))
    assert [opened[0], opened[2], opened[3]] == [(plain[0], 1), (plain[2], 0), (plain[3], 2)]
    with pytest.raises(mp.CardProtocolError) as e:
        cards.unmask(pp, [(toks[T + j], got[T + j][1], keys[j]) for j in range(T)], masked[1])
    assert e.value == opened[1]


def test_two_host_threads_unmask_on_one_table(engines, coracle):
    """two host threads on ONE table, each opening a batch of its own several times: the context's lock runs the calls one after the
    other, and every result equals the single-threaded one"""
    curve = "stark"
    c = oc.Ctx(engines(curve), coracle, curve)
    batches = [oc.Batch(c, 13, 5, salt=51), oc.Batch(c, 8, 8, salt=52)]
    for b in batches:
        b.tokens[len(b.tokens) // 2] = c.pool[0]      # one bad token each
    lists = [b.card_list(True) for b in batches]
    want = [b.unmask(c.t, lst) for b, lst in zip(batches, lists)]
    assert [sum(1 for v in w[3] if v) for w in want] == [1, 1]
    got, errors = [[], []], []

    def work(k):
        try:
            for _ in range(4):
                got[k].append(batches[k].unmask(c.t, lists[k]))
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(2):
        assert got[k] == [want[k]] * 4
    c.close()


def test_showdown_example_runs_end_to_end():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "showdown.py")], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    text = out.stdout.decode()
    assert "208 reveal tokens" in text and "52 cards opened" in text and text.strip().endswith("showdown ok"), text

