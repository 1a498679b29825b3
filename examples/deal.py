#!/usr/bin/env python3
"""Seating and dealing on the MI355X engine: eight tables of four players and one 52-card deck each (m=2, n=26).  One
compute_aggregate_keys call (mp_aggregate_keys_batch) verifies the 32 proofs of key ownership and sums the keys of every table; one deal
call (mp_mask_batch) masks the 8 x 52 open cards under their tables' keys with a Chaum-Pedersen proof each; one verify_deal call
(mp_verify_mask_batch) is what every player runs over all of them [REF barnett-smart-card-protocol/examples/round.rs:228-262, one player
and one card at a time there].  The first shuffle of a table then takes the dealt deck as it is."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")


def main():
    m, n, num_cards, num_tables, num_players = 2, 26, 52, 8, 4
    cards = mp.DLCards("stark", device=0)
    rng = mp.ChaCha20Rng(b"deal example seed".ljust(32, b"\0"))
    fresh = lambda: b"".join(rng.next_u64().to_bytes(8, "little") for _ in range(4))     # noqa: E731
    pp = cards.setup(fresh(), m, n)

    # seating: every player brings a key, a proof that it knows the secret, and a name
    tables = []
    for k in range(num_tables):
        seats = []
        for j in range(num_players):
            pk, sk = cards.player_keygen(rng, pp)
            info = b"table %d seat %d" % (k, j)
            seats.append((pk, cards.prove_key_ownership(fresh(), pp, pk, sk, info), info))
        tables.append(seats)
    t0 = time.time()
    joint = cards.compute_aggregate_keys(pp, tables)
    t1 = time.time()
    for key in joint:
        if isinstance(key, Exception):
            raise key
    assert joint[0] == cards.compute_aggregate_key(pp, tables[0])

    # open deck: 52 distinct points <-> classic cards [REF round.rs:253-256]; every table deals the same 52 under its own key
    extra = cards.setup(fresh(), m, num_cards)
    card_points = [extra.raw[64 * i:64 * (i + 1)] for i in range(num_cards)]
    plain = card_points * num_tables
    key_index = [k for k in range(num_tables) for _ in range(num_cards)]
    factors = [mp.fr_rand("stark", rng) for _ in plain]
    t2 = time.time()
    dealt = cards.deal([fresh() for _ in plain], pp, joint, key_index, plain, factors)
    t3 = time.time()
    for res in dealt:
        if isinstance(res, Exception):
            raise res
    masked, proofs = [d[0] for d in dealt], [d[1] for d in dealt]
    verdicts = cards.verify_deal(pp, joint, key_index, plain, masked, proofs)
    t4 = time.time()
    assert verdicts == [None] * len(plain), [v for v in verdicts if v is not None][:3]
    assert masked[0] == cards.mask(fresh(), pp, joint[0], plain[0], factors[0])[0]      # the card of `mask`
    # a card dealt under another table's key does not pass
    wrong = cards.verify_deal(pp, joint, [1] + key_index[1:num_cards], plain[:num_cards], masked[:num_cards], proofs[:num_cards])
    assert wrong[0] == mp.CryptoError("Chaum-Pedersen") and wrong[1:] == [None] * (num_cards - 1)

    # the first shuffle of table 0 takes the dealt deck
    deck = masked[:num_cards]
    perm = mp.Permutation.new(rng, num_cards)
    shuffled, proof = cards.shuffle_and_remask(fresh(), pp, joint[0], deck, [mp.fr_rand("stark", rng) for _ in range(num_cards)], perm)
    cards.verify_shuffle(pp, joint[0], deck, shuffled, proof)

    print("%d players seated at %d tables in %.1f ms" % (num_tables * num_players, num_tables, (t1 - t0) * 1e3))
    print("%d cards dealt in %.1f ms, verified in %.1f ms" % (len(plain), (t3 - t2) * 1e3, (t4 - t3) * 1e3))
    print("table 0 shuffled its dealt deck of %d cards" % num_cards)
    print("deal ok")


if __name__ == "__main__":
    main()
