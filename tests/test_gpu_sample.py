"""-m gpu: secrets drawn on the device from seeds -- mp_sample_secrets_batch[_dev], mp_shuffle_and_remask_batch_seeded[_dev],
mp_keygen_batch and their mirrors.  The cases are those of tests/sample_cases.py: the stream word for word at 1, 63, 64, 65 and 257 lanes
for every (S, P) on all four curves, with all-zero, all-0xFF and searched seeds (first candidate rejected, three rejections in a row,
permutation draws that start in the middle of a block and at a block boundary, a next_u64 whose high word changes j); (1024, 1024) and
(1, 4096) on STARK; the seeded prover against the unseeded one, the oracle and the verifier, with the table's key and with a key per
proof, host form and device-pointer form; key generation against the oracle, mp_msm, mp_sigma_prove_batch and mp_aggregate_keys_batch;
refusals; two host threads; DLCards' mirrors; examples/seeded_shuffle.py."""
import os
import subprocess
import sys
import threading

import pytest

import sample_cases as sc
from conftest import ROOT

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


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("curve", sc.CURVES)
def test_stream_word_for_word(engines, coracle, mp, curve, shape):
    _run(sc.run_stream, engines(curve), coracle, curve, shape, mp)


def test_long_streams_stark(engines, coracle):
    _run(sc.run_long, engines("stark"), coracle)


PROVE = [(curve, mn, B) for curve in ("stark", "bn254") for mn, B in sc.PROVE_SHAPES[curve]]


@pytest.mark.parametrize("keyed", [False, True], ids=["table key", "key per proof"])
@pytest.mark.parametrize("curve,mn,B", PROVE)
def test_seeded_prove_equals_unseeded_prove(engines, coracle, curve, mn, B, keyed):
    _run(sc.run_seeded, engines(curve), coracle, curve, mn, B, keyed, python_oracle=B == 1)


@pytest.mark.parametrize("keyed", [False, True], ids=["table key", "key per proof"])
@pytest.mark.parametrize("curve,mn,B", PROVE)
def test_device_pointer_form_equals_host_form(engines, coracle, curve, mn, B, keyed):
    import torch
    _run(sc.run_seeded_dev, engines(curve), coracle, curve, mn, B, keyed, torch, "cuda")


@pytest.mark.parametrize("K", sc.KEYGEN)
@pytest.mark.parametrize("curve", sc.CURVES)
def test_keygen_matches_the_oracle_and_seats(engines, coracle, curve, K):
    _run(sc.run_keygen, engines(curve), coracle, curve, K)


@pytest.mark.parametrize("curve", sc.CURVES)
def test_refusals(engines, coracle, curve):
    _run(sc.run_refusals, engines(curve), coracle, curve)


def test_two_host_threads_sample_on_one_table(engines, coracle):
    _run(sc.run_threads, engines("stark"), coracle, "stark", threading)


def test_dlcards_mirrors(mp, coracle):
    """sample_shuffle_witnesses, shuffle_and_remask_batch_seeded and player_keygen_batch against secret_stream and the single-element
    members"""
    cards = mp.DLCards("stark", device=0)
    pp = cards.setup(bytes(range(32)), 2, 3)
    seeds = list(sc.seeds_for("stark", 6, 6)[:5])
    players = cards.player_keygen_batch(seeds[:3], pp, infos=[b"seat %d" % i for i in range(3)])
    for i, (pk, sk, proof) in enumerate(players):
        assert sk == mp.secret_stream("stark", seeds[i], 1, 0)[0][0]
        assert pk == cards._mul(cards._t(pp), [(sk, pp.enc_parameters)])
        assert proof == cards.prove_key_ownership(seeds[i], pp, pk, sk, b"seat %d" % i)
    assert cards.player_keygen_batch(seeds[:3], pp) == [p[:2] for p in players]
    joint = cards.compute_aggregate_key(pp, [(pk, proof, b"seat %d" % i) for i, (pk, _, proof) in enumerate(players)])
    perms, factors = cards.sample_shuffle_witnesses(seeds, pp)
    for b, s in enumerate(seeds):
        assert (factors[b], perms[b].mapping) == mp.secret_stream("stark", s, 6, 6)
    g = coracle.gen_inputs("stark", 2, 3, 9)
    deck = [g["deck"][i * 128:(i + 1) * 128] for i in range(6)]
    out = cards.shuffle_and_remask_batch_seeded(seeds, pp, joint, [deck] * 5)
    assert out == cards.shuffle_and_remask_batch(seeds, pp, joint, [deck] * 5, factors, perms)
    assert out[0] == cards.shuffle_and_remask(seeds[0], pp, joint, deck, factors[0], perms[0])
    assert cards.verify_shuffle_batch(pp, joint, [deck] * 5, [o[0] for o in out], [o[1] for o in out]) == [None] * 5
    keys = [joint, players[0][0], players[1][0], joint, players[2][0]]
    keyed = cards.shuffle_and_remask_batch_seeded(seeds, pp, keys, [deck] * 5)
    assert keyed == cards.shuffle_and_remask_batch_keys(seeds, pp, keys, [deck] * 5, factors, perms)
    assert keyed[0] == out[0] and keyed[1] != out[1]


def test_seeded_shuffle_example_runs_end_to_end():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "seeded_shuffle.py")], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    text = out.stdout.decode()
    assert "4 shuffles from 4 seeds" in text and text.strip().endswith("seeded shuffle ok"), text
