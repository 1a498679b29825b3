#!/usr/bin/env python3
"""A showdown on the MI355X engine: four players, one 52-card deck (m=2, n=26), one shuffle -- then EVERY card is opened.  Each
player gives a reveal token with its Chaum-Pedersen proof for every card, all 4 x 52 in one compute_reveal_tokens call
(mp_reveal_batch), and one open_cards call (mp_unmask_batch) verifies the 208 proofs, subtracts the tokens and looks the 52
plaintexts up in the list of cards [REF barnett-smart-card-protocol/examples/round.rs:159-206, 352-430, one card and one player at a
time there].  The opened order must be the permutation that was applied."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")

SUITS, VALUES = ["Club", "Diamond", "Heart", "Spade"], ["2", "3", "4", "5", "6", "7", "8", "9", "10", "J", "Q", "K", "A"]


def main():
    m, n, num_cards = 2, 26, 52
    cards = mp.DLCards("stark", device=0)
    rng = mp.ChaCha20Rng(b"showdown example seed".ljust(32, b"\0"))
    fresh = lambda: b"".join(rng.next_u64().to_bytes(8, "little") for _ in range(4))     # noqa: E731
    pp = cards.setup(fresh(), m, n)

    names = [b"Andrija", b"Kobi", b"Nico", b"Tom"]
    players = []
    for name in names:
        pk, sk = cards.player_keygen(rng, pp)
        players.append(dict(name=name, pk=pk, sk=sk, proof=cards.prove_key_ownership(fresh(), pp, pk, sk, name)))
    joint_pk = cards.compute_aggregate_key(pp, [(p["pk"], p["proof"], p["name"]) for p in players])

    # open deck: 52 distinct points <-> classic cards, masked with r = 1 [REF round.rs:253-256]
    extra = cards.setup(fresh(), m, num_cards)
    card_points = [extra.raw[64 * i:64 * (i + 1)] for i in range(num_cards)]
    names_of = ["%s of %ss" % (v, s) for s in SUITS for v in VALUES]
    deck = [cards.mask(fresh(), pp, joint_pk, pt, 1)[0] for pt in card_points]

    perm = mp.Permutation.new(rng, num_cards)
    factors = [mp.fr_rand("stark", rng) for _ in range(num_cards)]
    shuffled, proof = cards.shuffle_and_remask(fresh(), pp, joint_pk, deck, factors, perm)
    cards.verify_shuffle(pp, joint_pk, deck, shuffled, proof)

    # the showdown: token j of card c comes from player j
    T = len(players)
    signer = [j for _ in range(num_cards) for j in range(T)]
    t0 = time.time()
    revealed = cards.compute_reveal_tokens([fresh() for _ in signer], pp, [(p["pk"], p["sk"]) for p in players], shuffled, signer)
    t1 = time.time()
    opened = cards.open_cards(pp, [p["pk"] for p in players], shuffled, signer, [r[0] for r in revealed], [r[1] for r in revealed], card_points)
    t2 = time.time()
    for res in opened:
        if isinstance(res, Exception):
            raise res
    order = [idx for _, idx in opened]
    assert order == perm.permute_array(list(range(num_cards))), "the opened order is not the permutation applied"
    assert all(pt == card_points[idx] for pt, idx in opened)
    print("%d reveal tokens in %.1f ms, %d cards opened in %.1f ms" % (len(signer), (t1 - t0) * 1e3, num_cards, (t2 - t1) * 1e3))
    print("the table shows: %s ..." % ", ".join(names_of[i] for i in order[:5]))
    print("showdown ok")


if __name__ == "__main__":
    main()
