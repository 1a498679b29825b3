"""-m gpu: the rest of the trait on the GPU, mirroring the reference's six non-shuffle tests
[REF barnett-smart-card-protocol/src/discrete_log_cards/tests.rs:48-173; masking.rs:64-107; remasking.rs:65-114;
reveal.rs:43-84] (same accept / reject behaviour and error names), with byte-for-byte parity against the oracle.

Everything here runs on all four curves: the DLCards flow (key generation, key ownership, aggregate key, mask, remask, reveal,
unmask; M, N = 4, 13 on the STARK curve as in the reference, a smaller deck elsewhere -- the flow is one card), and the cases of
tests/trait_cases.py, which the emulator tests of tests/test_cabi_and_host.py share: batched sigma proofs of one and two bases in
batches of 1, 63, 64, 65 and 257 with edge witnesses and equal / opposite bases, one defect per lane of a verify batch, points outside
the prime-order subgroup (BLS12-377), mp_remask_batch and mp_commit_batch on edge factors and points at infinity."""
import pytest

import mp_oracle as po
import trait_cases

pytestmark = pytest.mark.gpu

CURVES = trait_cases.CURVES
SIZES = {"stark": (4, 13)}          # the reference's test parameters [REF tests.rs:52-53]; (2, 3) on the other curves


@pytest.fixture(scope="module")
def envs(mp):
    cache = {}

    def get(curve):
        if curve not in cache:
            M, N_ = SIZES.get(curve, (2, 3))
            cards = mp.DLCards(curve, device=0)
            pp = cards.setup(bytes(range(32)), M, N_)
            cv = po.CURVES[curve]
            opp = po.setup(cv, M, N_, po.ChaCha20Rng(bytes(range(32))))
            assert pp.raw == po.params_to_bytes(opp)
            cache[curve] = cards, pp, cv, opp
        return cache[curve]
    return get


@pytest.fixture(params=CURVES)
def env(request, envs):
    """(cards, parameters, curve, the oracle's parameters); the body of a test that uses it runs with the oracle's encoders set to the curve"""
    e = envs(request.param)
    with po.curve_ctx(e[2]):
        yield e


def setup_players(mp, cards, pp, opp, cv, num):
    rng, orng = mp.ChaCha20Rng(b"\x11" * 32), po.ChaCha20Rng(b"\x11" * 32)
    players, agg = [], None
    for _ in range(num):
        pk, sk = cards.player_keygen(rng, pp)
        opk, osk = po.player_keygen(opp, orng)
        assert sk == osk and pk == po.pt_wire(opk)
        info = mp.fr_rand(cards.curve, rng).to_bytes(32, "little")
        assert info == po.fe_bytes(po.fr_rand(cv, orng))
        players.append((pk, sk, info))
        agg = po.pt_add(cv, agg, opk)
    return players, po.pt_wire(agg)


def test_generate_and_verify_key(mp, env):
    cards, pp, cv, opp = env
    rng = mp.ChaCha20Rng(b"\x21" * 32)
    pk, sk = cards.player_keygen(rng, pp)
    info = b"player public info"
    proof = cards.prove_key_ownership(b"\x05" * 32, pp, pk, sk, info)
    assert proof == po.sigma_proof_bytes(po.prove_key_ownership(opp, po.pt_from_wire(pk), sk, info, b"\x05" * 32))
    assert cards.verify_key_ownership(pp, pk, info, proof) is None
    wrong_sk = mp.fr_rand(cards.curve, rng)
    wrong_proof = cards.prove_key_ownership(b"\x05" * 32, pp, pk, wrong_sk, info)
    with pytest.raises(mp.CryptoError) as e:
        cards.verify_key_ownership(pp, pk, info, wrong_proof)
    assert e.value == mp.CryptoError("Schnorr Identification")


def test_aggregate_keys(mp, env):
    cards, pp, cv, opp = env
    players, expected = setup_players(mp, cards, pp, opp, cv, 10)
    triples = [(pk, cards.prove_key_ownership(bytes([i]) * 32, pp, pk, sk, info), info) for i, (pk, sk, info) in enumerate(players)]
    assert cards.compute_aggregate_key(pp, triples) == expected
    bad = list(triples)
    bad[3] = (bytes(cards.engine.point_bytes), bad[3][1], bad[3][2])          # a zeroed key [REF tests.rs:108-115]
    with pytest.raises(mp.CardProtocolError) as e:
        cards.compute_aggregate_key(pp, bad)
    assert e.value == mp.CardProtocolError("ProofVerificationError", mp.CryptoError("Schnorr Identification"))


def test_verify_masking_remasking_reveal_unmask(mp, env):
    cards, pp, cv, opp = env
    players, agg = setup_players(mp, cards, pp, opp, cv, 10)
    oagg = po.pt_from_wire(agg)
    rng = mp.ChaCha20Rng(b"\x31" * 32)
    card_pt = po.pt_mul(cv, mp.fr_rand(cards.curve, rng), cv.G)
    card = po.pt_wire(card_pt)
    r = mp.fr_rand(cards.curve, rng)
    # test_verify_masking [REF masking.rs:64-107]
    masked, proof = cards.mask(b"\x41" * 32, pp, agg, card, r)
    omasked, oproof = po.mask(opp, oagg, card_pt, r, b"\x41" * 32)
    assert masked == po.deck_to_bytes([omasked]) and proof == po.sigma_proof_bytes(oproof)
    assert cards.verify_mask(pp, agg, card, masked, proof) is None
    wrong_masked = po.deck_to_bytes([(po.pt_mul(cv, 3, cv.G), po.pt_mul(cv, 5, cv.G))])
    with pytest.raises(mp.CryptoError) as e:
        cards.verify_mask(pp, agg, card, wrong_masked, proof)
    assert e.value == mp.CryptoError("Chaum-Pedersen")
    # test_verify_remasking [REF remasking.rs:65-114]
    alpha = mp.fr_rand(cards.curve, rng)
    remasked, rproof = cards.remask(b"\x42" * 32, pp, agg, masked, alpha)
    oremasked, orproof = po.remask_with_proof(opp, oagg, omasked, alpha, b"\x42" * 32)
    assert remasked == po.deck_to_bytes([oremasked]) and rproof == po.sigma_proof_bytes(orproof)
    assert cards.verify_remask(pp, agg, masked, remasked, rproof) is None
    with pytest.raises(mp.CryptoError) as e:
        cards.verify_remask(pp, agg, masked, wrong_masked, rproof)
    assert e.value == mp.CryptoError("Chaum-Pedersen")
    # test_verify_reveal [REF reveal.rs:43-84] and test_unmask [REF tests.rs:125-173]
    tokens = []
    for i, (pk, sk, _) in enumerate(players):
        token, tproof = cards.compute_reveal_token(bytes([0x50 + i]) * 32, pp, sk, pk, remasked)
        otoken, otproof = po.compute_reveal_token(opp, sk, po.pt_from_wire(pk), oremasked, bytes([0x50 + i]) * 32)
        assert token == po.pt_wire(otoken) and tproof == po.sigma_proof_bytes(otproof)
        assert cards.verify_reveal(pp, pk, token, remasked, tproof) is None
        tokens.append((token, tproof, pk))
    with pytest.raises(mp.CryptoError) as e:
        cards.verify_reveal(pp, players[0][0], po.pt_wire(po.pt_mul(cv, 99, cv.G)), remasked, tokens[0][1])
    assert e.value == mp.CryptoError("Chaum-Pedersen")
    assert cards.unmask(pp, tokens, remasked) == card
    bad = list(tokens)
    bad[0] = (po.pt_wire(po.pt_mul(cv, 7, cv.G)), bad[0][1], bad[0][2])
    with pytest.raises(mp.CardProtocolError) as e:
        cards.unmask(pp, bad, remasked)
    assert e.value == mp.CardProtocolError("ProofVerificationError", mp.CryptoError("Chaum-Pedersen"))


def test_sigma_batch_parity(mp, envs):
    """a batch of 64 Chaum-Pedersen proofs through the C ABI equals the oracle; one tampered proof fails alone"""
    cards, pp, cv, opp = envs("stark")
    t = cards.table(pp, pp.enc_parameters)
    rng = po.ChaCha20Rng(b"\x61" * 32)
    B = 64
    bases = pubs = wit = seeds = exp = b""
    for i in range(B):
        x = po.fr_rand(cv, rng)
        g, h = po.pt_mul(cv, po.fr_rand(cv, rng), cv.G), po.pt_mul(cv, po.fr_rand(cv, rng), cv.G)
        a = [po.pt_mul(cv, x, g), po.pt_mul(cv, x, h)]
        seed = bytes([i]) * 32
        bases += po.pt_wire(g) + po.pt_wire(h)
        pubs += po.pt_wire(a[0]) + po.pt_wire(a[1])
        wit += po.fe_bytes(x)
        seeds += seed
        exp += po.sigma_proof_bytes(po.sigma_prove(cv, [g, h], a, x, po.REVEAL_RNG_SEED, seed))
    fsi = cards.engine.blake2s(po.REVEAL_RNG_SEED) * B
    got, st = t.sigma_prove_batch(2, bases, pubs, wit, fsi, seeds)
    assert got == exp and st == [0] * B
    assert t.sigma_verify_batch(2, bases, pubs, got, fsi) == [0] * B
    bad = bytearray(got)
    bad[17 * 160 + 159] ^= 1
    st = t.sigma_verify_batch(2, bases, pubs, bytes(bad), fsi)
    assert st[17] == 6 and sum(1 for v in st if v) == 1


# ---- the cases of tests/trait_cases.py on the gfx950 build (the emulator runs the same ones: tests/test_cabi_and_host.py) ------------
@pytest.mark.parametrize("curve", CURVES)
def test_sigma_batches_match_oracle(envs, coracle, curve):
    fails, checks = trait_cases.run_sigma_honest(envs(curve)[0].engine, coracle, curve)
    assert not fails, "\n".join(fails[:20])
    assert checks == 2 * (3 * 450 + 4 + 65)


@pytest.mark.parametrize("curve", CURVES)
def test_sigma_rejections_match_oracle(envs, coracle, curve):
    fails, checks = trait_cases.run_sigma_rejections(envs(curve)[0].engine, coracle, curve)
    assert not fails, "\n".join(fails[:20])
    assert checks >= 40


def test_sigma_calls_test_subgroup_membership(envs, coracle):
    fails, checks = trait_cases.run_sigma_subgroup(envs("bls12_377")[0].engine, coracle)
    assert not fails, "\n".join(fails[:20])
    assert checks == 19 + 16 + 19


@pytest.mark.parametrize("curve", CURVES)
def test_remask_batch_matches_oracle(envs, coracle, curve):
    fails, checks = trait_cases.run_remask(envs(curve)[0].engine, coracle, curve)
    assert not fails, "\n".join(fails[:20])
    assert checks == 1 + 63 + 65 + 257


@pytest.mark.parametrize("curve", CURVES)
def test_commit_batch_matches_oracle(envs, coracle, curve):
    fails, checks = trait_cases.run_commit(envs(curve)[0].engine, coracle, curve)
    assert not fails, "\n".join(fails[:20])
    assert checks == 1 + 1 + 5 + 65 + 3
