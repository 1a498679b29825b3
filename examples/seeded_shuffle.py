#!/usr/bin/env python3
"""A table's chain of four shuffles from four seeds on the MI355X engine (m=2, n=26): each of four players shuffles the deck the player
before left, and all a player supplies -- and has to remember -- is one fresh 32-byte seed.  Masking factors and permutation are drawn on
the device from the seed ("mpshuffle secret stream v1", include/mpshuffle.h), which is the prover seed as well: the witness never exists
on the host [REF barnett-smart-card-protocol/examples/round.rs:264-350: sample_vector / Permutation::new, then shuffle_and_remask, per
player].  Afterwards one permutation is derived again from its seed on the CPU (secret_stream), applied by hand, and compared with the
deck the engine produced."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")


def main():
    m, n, num_cards, num_players = 2, 26, 52, 4
    cards = mp.DLCards("stark", device=0)
    rng = mp.ChaCha20Rng(b"seeded shuffle example".ljust(32, b"\0"))      # stands for the players' CSPRNGs
    fresh = lambda: b"".join(rng.next_u64().to_bytes(8, "little") for _ in range(4))     # noqa: E731
    pp = cards.setup(fresh(), m, n)

    # seating: keys and proofs of key ownership from one seed per player
    infos = [b"seat %d" % j for j in range(num_players)]
    players = cards.player_keygen_batch([fresh() for _ in range(num_players)], pp, infos)
    joint = cards.compute_aggregate_keys(pp, [[(pk, proof, info) for (pk, _, proof), info in zip(players, infos)]])[0]
    if isinstance(joint, Exception):
        raise joint

    # the open deck, masked with factor 1 by whoever deals [REF round.rs:253-262]
    extra = cards.setup(fresh(), m, num_cards)
    plain = [extra.raw[64 * i:64 * (i + 1)] for i in range(num_cards)]
    dealt = cards.deal([fresh() for _ in plain], pp, [joint], [0] * num_cards, plain, [1] * num_cards)
    decks = [[d[0] for d in dealt]]

    # four shuffles, one per player, each from one seed
    seeds = [fresh() for _ in range(num_players)]
    proofs = []
    t0 = time.time()
    for seed in seeds:
        (shuffled, proof), = cards.shuffle_and_remask_batch_seeded([seed], pp, joint, [decks[-1]])
        decks.append(shuffled)
        proofs.append(proof)
    t1 = time.time()
    verdicts = cards.verify_shuffle_batch(pp, joint, decks[:-1], decks[1:], proofs)
    assert verdicts == [None] * num_players, verdicts

    # player 2 looks its shuffle up again: the seed gives factors and permutation back, and they explain the deck
    k = 2
    factors, perm = mp.secret_stream("stark", seeds[k], num_cards, num_cards)
    perms, facs = cards.sample_shuffle_witnesses([seeds[k]], pp)
    assert (factors, perm) == (facs[0], perms[0].mapping)
    permuted = [decks[k][perm[i]] for i in range(num_cards)]                 # out[i] = in[perm[i]] ...
    t = cards.table(pp, joint)
    by_hand = t.remask_batch(b"".join(permuted), b"".join(f.to_bytes(32, "little") for f in factors))      # ... + (rho_i G, rho_i pk)
    assert by_hand == b"".join(decks[k + 1]), "the deck is not the seed's permutation and factors applied to the deck before"
    assert sorted(perm) == list(range(num_cards)) and perm != list(range(num_cards))

    print("%d shuffles from %d seeds in %.1f ms, all verified" % (num_players, num_players, (t1 - t0) * 1e3))
    print("shuffle %d re-derived from its seed: permutation starts %s" % (k, perm[:6]))
    print("seeded shuffle ok")


if __name__ == "__main__":
    main()
