#!/usr/bin/env python3
"""Tables of different sizes in one call each: five tables with 2, 3, 5, 9 and 3 seats and a small deck of eight cards (m=2, n=4).  One
compute_aggregate_keys call seats all 22 players (mp_aggregate_keys_ragged_batch: the tables differ in size); every table deals its deck
and every player shuffles it once, so a table's chain has as many links as it has seats; one verify_shuffle_chains call verifies all 22
links (mp_verify_shuffle_chain_ragged), and one mp_verify_shuffle_chain_ragged_dev call verifies them once more from device buffers, where a
prover leaves them; at the showdown every table opens its first three cards, one token per seated player and card, in
one compute_reveal_tokens and one open_cards call (mp_reveal_ragged_batch, mp_unmask_ragged_batch: 2 to 9 tokens per card)
[REF barnett-smart-card-protocol/examples/round.rs, one table of four there]."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")

SEATS = [2, 3, 5, 9, 3]
NAMES = ["7♠", "8♠", "9♠", "10♠", "J♠", "Q♠", "K♠", "A♠"]
SHOWN = 3


def main():
    import torch      # (before the library is loaded: torch ships a HIP runtime of its own)
    m, n = 2, 4
    num_cards = m * n
    cards = mp.DLCards("stark", device=0)
    rng = mp.ChaCha20Rng(b"mixed tables example".ljust(32, b"\0"))
    fresh = lambda: b"".join(rng.next_u64().to_bytes(8, "little") for _ in range(4))     # noqa: E731
    pp = cards.setup(fresh(), m, n)

    # seating: tables of 2 to 9 players in one call
    players, tables = [], []                # players: (pk, sk) of everybody, table after table
    for k, seats in enumerate(SEATS):
        row = []
        for j in range(seats):
            pk, sk = cards.player_keygen(rng, pp)
            info = b"table %d seat %d" % (k, j)
            players.append((pk, sk))
            row.append((pk, cards.prove_key_ownership(fresh(), pp, pk, sk, info), info))
        tables.append(row)
    t0 = time.time()
    joint = cards.compute_aggregate_keys(pp, tables)
    t1 = time.time()
    for key in joint:
        if isinstance(key, Exception):
            raise key
    assert joint[3] == cards.compute_aggregate_key(pp, tables[3])

    # every table deals the same eight open cards under its own key
    extra = cards.setup(fresh(), m, num_cards)
    card_points = [extra.raw[64 * i:64 * (i + 1)] for i in range(num_cards)]
    plain = card_points * len(SEATS)
    key_index = [k for k in range(len(SEATS)) for _ in range(num_cards)]
    dealt = cards.deal([fresh() for _ in plain], pp, joint, key_index, plain, [mp.fr_rand("stark", rng) for _ in plain])
    for res in dealt:
        if isinstance(res, Exception):
            raise res

    # the shuffle chains: every seated player shuffles the deck of its table once
    chains = []
    for k, seats in enumerate(SEATS):
        decks, proofs = [[d[0] for d in dealt[k * num_cards:(k + 1) * num_cards]]], []
        for _ in range(seats):
            deck, proof = cards.shuffle_and_remask(fresh(), pp, joint[k], decks[-1], [mp.fr_rand("stark", rng) for _ in range(num_cards)],
                                                   mp.Permutation.new(rng, num_cards))
            decks.append(deck)
            proofs.append(proof)
        chains.append((joint[k], decks, proofs))
    t2 = time.time()
    verdicts = cards.verify_shuffle_chains(pp, chains)
    t3 = time.time()
    assert verdicts == [[None] * seats for seats in SEATS], verdicts
    # a link that does not belong to its chain is found, and nothing else is
    swapped = list(chains)
    swapped[1] = (joint[1], chains[1][1], [chains[1][2][0], chains[4][2][1], chains[1][2][2]])
    bad = cards.verify_shuffle_chains(pp, swapped)
    assert isinstance(bad[1][1], mp.CryptoError) and [v for row in bad for v in row].count(None) == sum(SEATS) - 1

    # once more from device buffers in the same table-major layout: the links are a host list, the words are final after sync()
    gpu = torch.device("cuda:0")
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gpu)      # noqa: E731
    d_keys = dev(b"".join(joint[k] * seats for k, seats in enumerate(SEATS)))
    d_decks = dev(b"".join(card for _, decks, _ in chains for deck in decks for card in deck))
    d_proofs = dev(b"".join(proof for _, _, proofs in chains for proof in proofs))
    d_status = torch.full((sum(SEATS),), -1, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    table = cards.table(pp, joint[0])
    table.verify_shuffle_chain_ragged_dev(SEATS, d_keys.data_ptr(), d_decks.data_ptr(), d_proofs.data_ptr(), d_status.data_ptr())
    cards.engine.sync()
    assert d_status.cpu().tolist() == [0] * sum(SEATS), d_status.cpu().tolist()
    passes, pieces = table.chain_ragged_stats()[:2]

    # showdown: the first three cards of every table, one token from every player at the table
    shown, signer, counts, at = [], [], [], 0
    for k, seats in enumerate(SEATS):
        for card in chains[k][1][-1][:SHOWN]:
            shown.append(card)
            signer += list(range(at, at + seats))
            counts.append(seats)
        at += seats
    t4 = time.time()
    revealed = cards.compute_reveal_tokens([fresh() for _ in signer], pp, players, shown, signer, counts=counts)
    opened = cards.open_cards(pp, [pk for pk, _ in players], shown, signer, [r[0] for r in revealed], [r[1] for r in revealed], card_points,
                              counts=counts)
    t5 = time.time()
    for res in opened:
        if isinstance(res, Exception):
            raise res
    assert all(idx is not None and point == card_points[idx] for point, idx in opened)
    # the single-card member says the same about the first card of the largest table
    c0 = 3 * SHOWN
    lanes = range(sum(counts[:c0]), sum(counts[:c0 + 1]))
    assert cards.unmask(pp, [(revealed[l][0], revealed[l][1], players[signer[l]][0]) for l in lanes], shown[c0]) == opened[c0][0]

    print("%d players seated at %d tables of %s seats in %.1f ms" % (len(players), len(SEATS), SEATS, (t1 - t0) * 1e3))
    print("%d shuffle links in %d chains verified in %.1f ms" % (sum(SEATS), len(SEATS), (t3 - t2) * 1e3))
    print("the same links verified from device buffers in %d passes of %d pieces" % (passes, pieces))
    print("%d reveal tokens made and %d cards opened in %.1f ms" % (len(signer), len(shown), (t5 - t4) * 1e3))
    for k, seats in enumerate(SEATS):
        print("table %d (%d seats) shows %s" % (k, seats, " ".join(NAMES[idx] for _, idx in opened[k * SHOWN:(k + 1) * SHOWN])))
    print("mixed tables ok")


if __name__ == "__main__":
    main()
