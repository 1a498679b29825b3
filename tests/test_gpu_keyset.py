"""GPU tests of key sets whose slots change -- mp_keyset_create_empty, mp_keyset_update[_dev], mp_keyset_clear, mp_keyset_live, the two
_keyset_dev shuffle calls over live and empty slots, the seeded prover, the ragged chain verifier and the dealing calls by index, seating into a set -- on the gfx950 build: the cases of tests/keyset_cases.py, with the ordering case
that only a GPU's streams can fail (a missing wait between a queued prove or verify call and the update behind it shows nowhere else,
as tests/test_gpu_host_pipeline.py notes for its streams) and the build slice at its real size of 1 024 keys."""
import pytest

import keyset_cases as kc

pytestmark = pytest.mark.gpu

SLICE = 1024


@pytest.fixture(scope="module")
def engines(mp):
    mp.build()
    cache = {}

    def get(curve):
        if curve not in cache:
            cache[curve] = mp.Engine(curve, device=0)
        return cache[curve]
    return get


def _run(want, fn, *args):
    import torch
    fails, checks = fn(*args, torch, "cuda:0")
    assert not fails, "\n".join(fails[:40])
    assert checks == want


def _form(k):
    return ("host", "dev")[k % 2]


@pytest.mark.parametrize("curve", kc.CURVES)
def test_every_index_of_an_empty_set_is_refused_and_live_neighbours_serve(engines, coracle, curve):
    _run(kc.empty_count(), kc.run_empty, engines(curve), coracle, curve)


@pytest.mark.parametrize("count", kc.UPDATE_COUNTS)
def test_filled_slots_serve_the_oracles_bytes_under_their_keys(engines, coracle, count):
    _run(kc.fill_count(count), kc.run_fill, count, _form(count), engines("stark"), coracle, "stark")


@pytest.mark.parametrize("curve", kc.CURVES[1:])
def test_filled_slots_on_the_other_curves(engines, coracle, curve):
    _run(kc.fill_count(2), kc.run_fill, 2, "dev", engines(curve), coracle, curve)


@pytest.mark.parametrize("created", [True, False], ids=["mp_keyset_create", "mp_keyset_create_empty"])
@pytest.mark.parametrize("curve", kc.CURVES)
def test_a_replaced_slot_serves_the_new_key_and_its_neighbours_their_own(engines, coracle, curve, created):
    _run(kc.replace_count(created), kc.run_replace, created, _form(created), engines(curve), coracle, curve)


@pytest.mark.parametrize("at", kc.REFUSED_AT)
@pytest.mark.parametrize("name", kc.defects("stark"))
def test_a_refused_key_empties_its_slot_and_no_other(engines, coracle, name, at):
    _run(kc.refused_count(), kc.run_refused, name, at, _form(at), engines("stark"), coracle, "stark")


@pytest.mark.parametrize("curve,name,at", [(c, n, kc.REFUSED_AT[(i + j) % 3]) for j, c in enumerate(kc.CURVES[1:])
                                           for i, n in enumerate(kc.defects(c))]
                         + [("bls12_377", "outside the subgroup", a) for a in kc.REFUSED_AT[1:]])
def test_refused_keys_on_the_other_curves(engines, coracle, curve, name, at):
    _run(kc.refused_count(), kc.run_refused, name, at, "dev", engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_near_misses_enter_the_set(engines, coracle, curve):
    _run(kc.near_miss_count(), kc.run_near_miss, "host", engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_malformed_slots_arrays_change_nothing(engines, coracle, curve):
    _run(kc.bad_slots_count(), kc.run_bad_slots, engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_cleared_slots_are_empty_and_their_neighbours_untouched(engines, coracle, curve):
    _run(kc.clear_count(), kc.run_clear, "dev", engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_calls_queued_around_an_update_see_the_keys_of_their_moment(engines, coracle, curve):
    """fails on the parent for want of any way to make slot s mean another key; an update that does not wait for the prove lane, or that
    leaves a pipelined verify pass unexamined, fails here and nowhere else"""
    _run(kc.ordering_count(), kc.run_ordering, engines(curve), coracle, curve)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_one_key_past_a_build_slice_at_its_real_size(engines, coracle, form):
    """1 025 keys, 0.5 GB of tables: the library as built, not one with a lowered slice"""
    _run(kc.slice_count(), kc.run_slice, SLICE, form, engines("stark"), coracle, "stark")


def test_chains_verified_by_one_index_per_table(engines, coracle):
    _run(kc.chains_count(kc.CHAIN_MODES, (0, 1, 2)), kc.run_chains, kc.CHAIN_MODES, (0, 1, 2), engines("stark"), coracle, "stark")


@pytest.mark.parametrize("curve", kc.CURVES[1:])
def test_one_chain_case_on_the_other_curves(engines, coracle, curve):
    """binary pieces; three honest tables around one past the set and one on an empty slot"""
    _run(kc.chains_count((1,), (2,)), kc.run_chains, (1,), (2,), engines(curve), coracle, curve)


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
def test_the_seeded_prover_by_index(engines, coracle, curve):
    _run(kc.seeded_count(), kc.run_seeded, engines(curve), coracle, curve)


def test_the_protocol_layer_names_chains_by_key_set_index(mp, coracle):
    """DLCards.key_set and verify_shuffle_chains with (key_set, index): the verdicts of the same call with the keys written out, and the
    error of a bad argument on every link of the table whose slot was cleared"""
    w = kc.world(coracle, "stark")
    cards = mp.DLCards("stark", device=0)
    pp = mp.Parameters(w.m, w.n, w.params)
    T = len(kc.CHAIN_LINKS)
    keys = w.keys(300, T)
    decks, proofs = kc._chains(w, keys)
    cb = 2 * w.c.pb
    cut = lambda d: [d[cb * i:cb * (i + 1)] for i in range(w.N)]      # noqa: E731
    rows, o = [], 0
    for k, L in enumerate(kc.CHAIN_LINKS):
        rows.append(([cut(d) for d in decks[o + k:o + k + L + 1]], proofs[o:o + L]))
        o += L
    ks = cards.key_set(pp, T + 1)
    assert ks.live() == 0 and ks.update([T - k for k in range(T)], b"".join(keys)) == [0] * T
    by_key = cards.verify_shuffle_chains(pp, [(keys[k], d, p) for k, (d, p) in enumerate(rows)])
    by_index = cards.verify_shuffle_chains(pp, [((ks, T - k), d, p) for k, (d, p) in enumerate(rows)])
    assert by_key == [[None] * L for L in kc.CHAIN_LINKS] and by_index == by_key
    ks.clear([T - 2])
    again = cards.verify_shuffle_chains(pp, [((ks, T - k), d, p) for k, (d, p) in enumerate(rows)])
    assert [again[k] for k in (0, 1, 3)] == [by_key[k] for k in (0, 1, 3)]
    assert len(again[2]) == kc.CHAIN_LINKS[2] and all(isinstance(e, mp.CardProtocolError) for e in again[2]), again[2]
    with pytest.raises(mp.CardProtocolError):
        cards.verify_shuffle_chains(pp, [((ks, 1), *rows[0]), (keys[1], *rows[1])])
    ks.close()
    ks.table.close()


def _run_deal(want, fn, *args):
    fails, checks = fn(*args)
    assert not fails, "\n".join(fails[:40])
    assert checks == want


@pytest.mark.parametrize("shape", kc.DEAL_SHAPES, ids=lambda s: "C=%d" % s[0])
def test_dealing_by_index_gives_the_oracles_bytes_and_those_of_the_keyed_calls(engines, coracle, shape):
    import torch
    _run_deal(kc.deal_count([shape]), kc.run_deal, [shape], engines("stark"), coracle, "stark", torch, "cuda:0")


@pytest.mark.parametrize("curve", kc.CURVES[1:])
def test_one_deal_case_on_the_other_curves(engines, coracle, curve):
    import torch
    _run_deal(kc.deal_count([(65, 7)]), kc.run_deal, [(65, 7)], engines(curve), coracle, curve, torch, "cuda:0")


def test_the_verifier_by_index_takes_one_defect_per_lane_screened_or_not(engines, coracle):
    _run_deal(kc.deal_defects_count("stark"), kc.run_deal_defects, engines("stark"), coracle, "stark")


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
def test_seating_straight_into_a_set(engines, coracle, curve):
    import torch
    _run_deal(kc.seat_count(), kc.run_seat, engines(curve), coracle, curve, torch, "cuda:0")
