"""-m gpu: the screening pass of the sigma verifiers (mp_set_sigma_screen) on the GPU, all four curves.  The case functions of
open_cases.py and deal_cases.py, unmodified, on tables that screen in groups of 64 lanes (their shapes are 1, 63, 64, 65 and 257 lanes: a
lone short group, a full group, a full group plus a group of one, a ragged tail); the cases of sigma_screen_cases.py -- screened against
unscreened, localisation, cancelling forgeries, the cofactor rule, usage --; both bucket paths under SIGMA_SCREEN_AUTO at the smallest
sizes that reach them; DLCards(sigma_screen=...)."""
import pytest

import deal_cases as dc
import open_cases as oc
import sigma_screen_cases as sc

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


def _screened(engines, curve, honest, fn, coracle, *args):
    eng = sc.Screened(engines(curve))
    _run(fn, eng, coracle, curve, *args)
    fails = sc.honest_log_failures(eng.log) if honest else sc.screened_log_failures(eng.log)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("curve", CURVES)
def test_opening_honest_shapes_under_screening(engines, coracle, curve):
    _screened(engines, curve, True, oc.run_honest, coracle)


@pytest.mark.parametrize("curve", CURVES)
def test_dealing_honest_shapes_under_screening(engines, coracle, curve):
    _screened(engines, curve, True, dc.run_honest, coracle)


@pytest.mark.parametrize("curve", CURVES)
def test_seating_under_screening(engines, coracle, curve):
    _screened(engines, curve, False, dc.run_seating, coracle)


@pytest.mark.parametrize("curve", CURVES)
def test_opening_defects_agreement_and_device_pointers_under_screening(engines, coracle, curve):
    import torch
    _screened(engines, curve, False, oc.run_defects, coracle)
    _screened(engines, curve, False, oc.run_agreement, coracle)
    _screened(engines, curve, False, oc.run_dev, coracle, torch, "cuda")


@pytest.mark.parametrize("curve", CURVES)
def test_dealing_defects_and_device_pointers_under_screening(engines, coracle, curve):
    import torch
    _screened(engines, curve, False, dc.run_defects, coracle)
    _screened(engines, curve, False, dc.run_dev, coracle, torch, "cuda")


def test_points_outside_the_subgroup_under_screening(engines, coracle):
    _screened(engines, "bls12_377", False, oc.run_subgroup, coracle)
    _screened(engines, "bls12_377", False, dc.run_subgroup, coracle)


@pytest.mark.parametrize("curve", CURVES)
def test_screened_equals_unscreened(engines, coracle, curve):
    _run(sc.run_equal, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_a_defect_fails_its_group_alone(engines, coracle, curve):
    _run(sc.run_localisation, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_cancelling_forgeries_are_refused(engines, coracle, curve):
    _run(sc.run_cancelling, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_cofactor_rule(engines, coracle, curve):
    _run(sc.run_cofactor, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_usage(engines, coracle, curve):
    _run(sc.run_usage, engines(curve), coracle, curve)


# Both bucket paths under SIGMA_SCREEN_AUTO at the smallest sizes that reach them.  An opening lane is five points of its group's
# equation.  4 096 lanes are 20 480 points: too few for the split pipeline, so 64 equations of 64 lanes for the one-wave-per-window
# kernel -- on BLS12-377, where that kernel spills and group equations of its size are off (mp_set_group_verify), such a call is not
# screened under AUTO.  12 288 lanes are 61 440 points: one equation for the split pipeline on either curve (from 50 000 points on, 40 000 on
# BLS12-377).  The engine's rule decides; the kernels the call launched say which path it took.
@pytest.mark.parametrize("curve,lanes,kernel", [("stark", 4096, "k_bucket_msm"), ("stark", 12288, "k_bucket_sort"),
                                                ("bls12_377", 4096, None), ("bls12_377", 12288, "k_bucket_sort")])
def test_both_bucket_paths_under_auto(engines, coracle, curve, lanes, kernel):
    _run(sc.run_paths, engines(curve), coracle, curve, lanes, kernel)


def test_dlcards_with_sigma_screen_opens_a_dealt_hand_to_the_same_cards(mp):
    """seating, dealing and opening of one table of 9 through DLCards, with sigma_screen=(64, 1) and without: same aggregate key, same
    verdicts, same cards; a bad token fails its card alone either way"""
    curve, M, N_ = "stark", 4, 13
    results = []
    for screen in (None, (64, 1)):
        cards = mp.DLCards(curve, device=0, sigma_screen=screen)
        pp = cards.setup(bytes(range(32)), M, N_)
        rng = mp.ChaCha20Rng(b"\x11" * 32)
        players = [cards.player_keygen(rng, pp) for _ in range(9)]
        seats = [(pk, cards.prove_key_ownership(bytes([i]) * 32, pp, pk, sk, b"info"), b"info") for i, (pk, sk) in enumerate(players)]
        agg = cards.compute_aggregate_keys(pp, [seats])[0]
        G = pp.enc_parameters
        t = cards.table(pp, G)
        plain = [t.msm(1, 1, mp.fr_rand(curve, rng).to_bytes(32, "little"), G) for _ in range(8)]
        factors = [mp.fr_rand(curve, rng) for _ in plain]
        dealt = cards.deal([bytes([0x41 + i]) * 32 for i in range(8)], pp, [agg], [0] * 8, plain, factors)
        masked = [d[0] for d in dealt]
        vd = cards.verify_deal(pp, [agg], [0] * 8, plain, masked, [d[1] for d in dealt])
        re = cards.deal_remask([bytes([0x61 + i]) * 32 for i in range(8)], pp, [agg], [0] * 8, masked, factors[::-1])
        vr = cards.verify_deal_remask(pp, [agg], [0] * 8, masked, [r[0] for r in re], [r[1] for r in re])
        hand = [r[0] for r in re]
        T = len(players)
        signer = [j for _ in hand for j in range(T)]
        got = cards.compute_reveal_tokens([bytes([0x50 + l]) * 32 for l in range(len(signer))], pp, players, hand, signer)
        keys = [pk for pk, _ in players]
        toks = [g[0] for g in got]
        opened = cards.open_cards(pp, keys, hand, signer, toks, [g[1] for g in got], plain)
        toks[3 * T + 4] = t.msm(1, 1, (7).to_bytes(32, "little"), G)
        opened_bad = cards.open_cards(pp, keys, hand, signer, toks, [g[1] for g in got], plain)
        stats = t.sigma_screen_stats()
        results.append((agg, vd, vr, opened, opened_bad))
        assert opened == [(p, i) for i, p in enumerate(plain)] and vd == [None] * 8 and vr == [None] * 8
        assert opened_bad[3] == mp.CardProtocolError("ProofVerificationError", mp.CryptoError("Chaum-Pedersen"))
        # 9 seats, 8 + 8 dealt cards, 72 + 72 tokens; the bad token fails one of the two groups of the second opening
        assert stats == ([9 + 8 + 8 + 72 + 72, 1 + 1 + 1 + 2 + 2, 1, 64] if screen else [0, 0, 0, 0])
    assert results[0] == results[1]
