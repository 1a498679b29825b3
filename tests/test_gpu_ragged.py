"""-m gpu: the ragged calls on the GPU -- mp_reveal_ragged_batch, mp_unmask_ragged_batch[_dev], mp_aggregate_keys_ragged_batch,
mp_verify_shuffle_chain_ragged and their mirrors.  The cases are those of tests/ragged_cases.py, which tests/test_ragged_emu.py runs
through the emulator, here on all four curves (BLS12-377 with its subgroup test on, the default): items of 1 to 257 lanes whose runs end
at, start at and straddle a wave and a workgroup edge, against the C++ oracle and against the uniform calls on the regrouped items;
defects at the first and the last lane of an item and in one-lane items; the screened verifiers; malformed offsets; the device-pointer
form; the Python oracle; chains of 3, 1, 2, 3 and 1 links; the C++ mirror; DLCards with tables of 2, 3 and 5 players against its
single-call members; examples/mixed_tables.py."""
import os
import subprocess
import sys

import pytest

import ragged_cases as rc
from conftest import ROOT

pytestmark = pytest.mark.gpu

CURVES = rc.CURVES
_ids = [c[0] for c in rc.CASES]


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


def test_every_case_hits_the_edge_it_names():
    assert rc.workgroup_size() == rc.WORKGROUP
    assert not rc.edge_failures()


@pytest.mark.parametrize("case", rc.CASES, ids=_ids)
@pytest.mark.parametrize("curve", CURVES)
def test_opening_matches_the_oracle_and_the_regrouped_uniform_calls(engines, coracle, curve, case):
    _run(rc.run_open_case, engines(curve), coracle, curve, case)


@pytest.mark.parametrize("case", rc.CASES, ids=_ids)
@pytest.mark.parametrize("curve", CURVES)
def test_seating_matches_the_oracle_and_the_regrouped_uniform_calls(engines, coracle, curve, case):
    _run(rc.run_seating_case, engines(curve), coracle, curve, case)


@pytest.mark.parametrize("shape", rc.EQUAL, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("curve", CURVES)
def test_equal_counts_give_the_bytes_of_the_uniform_calls(engines, coracle, curve, shape):
    _run(rc.run_open_equal, engines(curve), coracle, curve, shape)
    _run(rc.run_seating_equal, engines(curve), coracle, curve, shape)


@pytest.mark.parametrize("curve", CURVES)
def test_defects_stay_with_their_lanes_and_items(engines, coracle, curve):
    _run(rc.run_open_defects, engines(curve), coracle, curve)
    _run(rc.run_seating_defects, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_screened_calls_give_the_same_words_and_bytes(engines, coracle, curve):
    _run(rc.run_screen, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors_leave_the_outputs_alone(engines, coracle, curve):
    _run(rc.run_argument_errors, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_device_pointer_form_gives_the_same_outputs(engines, coracle, curve):
    import torch
    _run(rc.run_open_dev, engines(curve), coracle, curve, torch, "cuda")


@pytest.mark.parametrize("curve", CURVES)
def test_tiny_batch_matches_the_python_oracle(engines, coracle, curve):
    _run(rc.run_open_python_oracle, engines(curve), coracle, curve)


@pytest.mark.parametrize("keyed", [False, True], ids=["own key", "keys per link"])
def test_chains_of_different_lengths(engines, coracle, keyed):
    _run(rc.run_chains, engines("stark"), coracle, keyed)


@pytest.mark.parametrize("curve", CURVES)
def test_dlcards_mixed_tables_against_the_single_call_members(mp, curve):
    """tables of 2, 3 and 5 players: compute_aggregate_keys gives the key of compute_aggregate_key table by table, and a bad proof fails
    its table alone; two cards per table opened with counts=...: the tokens and proofs of compute_reveal_token, the plaintexts of unmask,
    and a bad token fails its card alone with unmask's error.  Without counts the uneven signer list is refused as before."""
    M, N_ = 2, 3
    seats = [2, 3, 5]
    cards = mp.DLCards(curve, device=0)
    pp = cards.setup(bytes(range(32)), M, N_)
    rng = mp.ChaCha20Rng(b"\x12" * 32)
    players, tables = [], []
    for k, n in enumerate(seats):
        row = []
        for j in range(n):
            pk, sk = cards.player_keygen(rng, pp)
            info = b"table %d seat %d" % (k, j)
            players.append((pk, sk))
            row.append((pk, cards.prove_key_ownership(bytes([16 * k + j]) * 32, pp, pk, sk, info), info))
        tables.append(row)
    joint = cards.compute_aggregate_keys(pp, tables)
    assert joint == [cards.compute_aggregate_key(pp, row) for row in tables]
    bad = [list(row) for row in tables]
    bad[1][2] = (bad[1][2][0], bad[1][0][1], bad[1][2][2])
    got = cards.compute_aggregate_keys(pp, bad)
    assert got[1] == mp.CardProtocolError("ProofVerificationError", mp.CryptoError("Schnorr Identification"))
    assert [got[0], got[2]] == [joint[0], joint[2]]
    with pytest.raises(mp.CardProtocolError):
        cards.compute_aggregate_keys(pp, [tables[0], []])
    G = pp.enc_parameters
    t = cards.table(pp, G)
    rng = mp.ChaCha20Rng(b"\x32" * 32)
    plain = [t.msm(1, 1, mp.fr_rand(curve, rng).to_bytes(32, "little"), G) for _ in range(6)]
    masked = [cards.mask(bytes([0x41 + i]) * 32, pp, joint[i // 2], p, mp.fr_rand(curve, rng))[0] for i, p in enumerate(plain)]
    counts = [seats[i // 2] for i in range(6)]
    start = [0, 2, 5]
    signer = [start[i // 2] + j for i in range(6) for j in range(counts[i])]
    first = [sum(counts[:i]) for i in range(7)]
    seeds = [bytes([0x50 + l]) * 32 for l in range(len(signer))]
    got = cards.compute_reveal_tokens(seeds, pp, players, masked, signer, counts=counts)
    assert got == [cards.compute_reveal_token(seeds[l], pp, players[signer[l]][1], players[signer[l]][0], masked[i])
                   for i in range(6) for l in range(first[i], first[i + 1])]
    keys = [pk for pk, _ in players]
    card_list = [plain[2], plain[0], plain[5]]
    toks, prfs = [g[0] for g in got], [g[1] for g in got]
    opened = cards.open_cards(pp, keys, masked, signer, toks, prfs, card_list, counts=counts)
    assert opened == [(plain[0], 1), (plain[1], None), (plain[2], 0), (plain[3], None), (plain[4], None), (plain[5], 2)]
    for i in range(6):
        assert cards.unmask(pp, [(toks[l], prfs[l], keys[signer[l]]) for l in range(first[i], first[i + 1])], masked[i]) == plain[i]
    toks[first[3] - 1] = t.msm(1, 1, (7).to_bytes(32, "little"), G)          # the last token of card 2: card 3's first one is next to it
    opened = cards.open_cards(pp, keys, masked, signer, toks, prfs, card_list, counts=counts)
    assert opened[2] == mp.CardProtocolError("ProofVerificationError", mp.CryptoError("Chaum-Pedersen"))
    assert opened[:2] + opened[3:] == [(plain[0], 1), (plain[1], None), (plain[3], None), (plain[4], None), (plain[5], 2)]
    with pytest.raises(mp.CardProtocolError) as e:
        cards.unmask(pp, [(toks[l], prfs[l], keys[signer[l]]) for l in range(first[2], first[3])], masked[2])
    assert e.value == opened[2]
    with pytest.raises(mp.CardProtocolError) as e:                          # 20 signers for 6 cards, and no counts
        cards.open_cards(pp, keys, masked, signer, toks, prfs, card_list)
    assert "same number of players" in str(e.value)
    with pytest.raises(mp.CardProtocolError):
        cards.open_cards(pp, keys, masked, signer, toks, prfs, card_list, counts=counts[:-1] + [counts[-1] + 1])


def test_dlcards_verify_shuffle_chains_against_verify_shuffle(mp):
    """chains of 2, 1 and 3 links under three keys: verify_shuffle_chains says link by link what verify_shuffle says, for honest chains
    and with one proof swapped"""
    M, N_ = 2, 3
    cards = mp.DLCards("stark", device=0)
    pp = cards.setup(bytes(range(32)), M, N_)
    rng = mp.ChaCha20Rng(b"\x13" * 32)
    G = pp.enc_parameters
    t = cards.table(pp, G)
    chains = []
    for k, links in enumerate([2, 1, 3]):
        key = t.msm(1, 1, mp.fr_rand("stark", rng).to_bytes(32, "little"), G)
        deck = [cards.mask(bytes([0x60 + i]) * 32, pp, key, t.msm(1, 1, mp.fr_rand("stark", rng).to_bytes(32, "little"), G),
                           mp.fr_rand("stark", rng))[0] for i in range(M * N_)]
        decks, proofs = [deck], []
        for j in range(links):
            d, p = cards.shuffle_and_remask(bytes([0x70 + 8 * k + j]) * 32, pp, key, decks[-1], [mp.fr_rand("stark", rng) for _ in range(M * N_)],
                                            mp.Permutation.new(rng, M * N_))
            decks.append(d)
            proofs.append(p)
        chains.append((key, decks, proofs))
    assert cards.verify_shuffle_chains(pp, chains) == [[None] * 2, [None], [None] * 3]
    swapped = list(chains)
    swapped[2] = (chains[2][0], chains[2][1], [chains[2][2][0], chains[0][2][1], chains[2][2][2]])
    got = cards.verify_shuffle_chains(pp, swapped)
    want = []
    for key, decks, proofs in swapped:
        row = []
        for j, p in enumerate(proofs):
            try:
                row.append(cards.verify_shuffle(pp, key, decks[j], decks[j + 1], p))
            except mp.CryptoError as e:
                row.append(e)
        want.append(row)
    assert got == want and isinstance(got[2][1], mp.CryptoError) and sum(v is None for row in got for v in row) == 5
    with pytest.raises(mp.CardProtocolError):
        cards.verify_shuffle_chains(pp, [(chains[0][0], chains[0][1][:1], [])])


def test_cpp_mirror_ragged_members(mp, tmp_path):
    """the ragged overloads of include/barnett_smart.hpp, compiled with g++ against libmpshuffle.so"""
    libdir = os.path.join(ROOT, "mental-poker_amd")
    exe = tmp_path / "mirror_ragged"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mirror_ragged.cpp"),
                           "-L", libdir, "-lmpshuffle", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mirror_ragged ok" in out.stdout, out.stdout + out.stderr


def test_mixed_tables_example_runs_end_to_end():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mixed_tables.py")], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    text = out.stdout.decode()
    assert "22 players seated at 5 tables" in text and "22 shuffle links in 5 chains" in text and "15 cards opened" in text and \
        text.strip().endswith("mixed tables ok"), text
