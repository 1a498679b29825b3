#!/usr/bin/env python3
"""Five card tables in ONE key set, two hands, and a change of seats between them (m = 2, n = 26, STARK curve, device buffers are torch
tensors).  The server names a table by its slot in the set: it seats the tables straight into their slots
(mp_keyset_seat_ragged_batch: the aggregate keys never leave the device), deals the open deck at every table by index
(mp_mask_batch_keyset, verified with mp_verify_mask_batch_keyset), every table's deck is shuffled by as many players as sit there -- by index, each shuffle from one seed
(mp_shuffle_and_remask_batch_seeded_keyset_dev) -- and the chains, of different lengths, are verified in one call with one index per table
(mp_verify_shuffle_chain_ragged_keyset).  Then one player leaves tables 1 and 3 and another sits down: only those two slots are seated
again (1 MB of tables instead of the whole set), and the second hand is played the same way.  At the end table 1's first
shuffle of each hand is checked byte for byte against the CPU oracle under the key its slot held at the time."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "py")):
    sys.path.insert(0, p)
mp = importlib.import_module("mental-poker_amd")

DEV = "cuda:0"
SEATS = [2, 3, 4, 3, 2]          # players per table = shuffles per hand


def gpu(raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)


def main():
    import coracle
    m, n, N = 2, 26, 52
    cards = mp.DLCards("stark", device=0)
    rng = mp.ChaCha20Rng(b"reseat example".ljust(32, b"\0"))      # stands for the players' CSPRNGs
    fresh = lambda: b"".join(rng.next_u64().to_bytes(8, "little") for _ in range(4))     # noqa: E731
    pp = cards.setup(fresh(), m, n)
    T = len(SEATS)
    ks = cards.key_set(pp, T)
    t = ks.table
    assert ks.live() == 0

    def sit(count, tag):
        infos = [b"%s seat %d" % (tag, j) for j in range(count)]
        players = cards.player_keygen_batch([fresh() for _ in range(count)], pp, infos)
        return [(pk, proof, info) for (pk, _, proof), info in zip(players, infos)]

    def seat(slots, rows):
        """the aggregate keys of the tables `rows`, into the slots `slots`"""
        sums = cards.compute_aggregate_keys(pp, rows, into=(ks, slots))
        assert not any(isinstance(s, Exception) for s in sums), sums
        return sums

    extra = cards.setup(fresh(), m, N)
    plain = [extra.raw[64 * i:64 * (i + 1)] for i in range(N)]

    def hand(keys):
        """deal, shuffle every table SEATS[k] times by index, verify the ragged chains by index -> (decks, proofs, seeds) per table"""
        by_slot = [k for k in range(T) for _ in range(N)]
        dealt = cards.deal([fresh() for _ in range(T * N)], pp, ks, by_slot, plain * T, [1] * (T * N))
        assert cards.verify_deal(pp, ks, by_slot, plain * T, [d[0] for d in dealt], [d[1] for d in dealt]) == [None] * (T * N)
        assert dealt[N][0] == cards.deal([fresh()], pp, [keys[1]], [0], plain[:1], [1])[0][0]      # the same card under the key written out
        decks = [[b"".join(d[0] for d in dealt[k * N:(k + 1) * N])] for k in range(T)]
        proofs, seeds = [[] for _ in range(T)], [[] for _ in range(T)]
        dsz, psz = len(decks[0][0]), t.proof_bytes
        for j in range(max(SEATS)):
            rows = [k for k in range(T) if SEATS[k] > j]
            B = len(rows)
            sd = [fresh() for _ in rows]
            d_in, d_seeds = gpu(b"".join(decks[k][-1] for k in rows)), gpu(b"".join(sd))
            d_idx = torch.tensor(rows, dtype=torch.int32, device=DEV)
            od, op = torch.zeros(B * dsz, dtype=torch.uint8, device=DEV), torch.zeros(B * psz, dtype=torch.uint8, device=DEV)
            st = torch.full((B,), 7, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            t.shuffle_and_remask_batch_seeded_keyset_dev(ks, B, d_idx.data_ptr(), d_in.data_ptr(), d_seeds.data_ptr(), od.data_ptr(),
                                                         op.data_ptr(), st.data_ptr())
            cards.engine.sync()
            assert st.tolist() == [0] * B
            out_d, out_p = od.cpu().numpy().tobytes(), op.cpu().numpy().tobytes()
            for i, k in enumerate(rows):
                decks[k].append(out_d[i * dsz:(i + 1) * dsz])
                proofs[k].append(out_p[i * psz:(i + 1) * psz])
                seeds[k].append(sd[i])
        cut = lambda d: [d[128 * i:128 * (i + 1)] for i in range(N)]      # noqa: E731
        words = cards.verify_shuffle_chains(pp, [((ks, k), [cut(d) for d in decks[k]], proofs[k]) for k in range(T)])
        assert words == [[None] * SEATS[k] for k in range(T)], words
        return decks, proofs, seeds

    def oracle_check(key, decks, proofs, seeds):
        """the first shuffle of a table, again on the CPU from its seed"""
        factors, perm = mp.secret_stream("stark", seeds[0], N, N)
        rho = b"".join(f.to_bytes(32, "little") for f in factors)
        want = coracle.shuffle_and_remask("stark", m, n, pp.raw, key, decks[0], rho, perm, seeds[0])
        assert (decks[1], proofs[0]) == tuple(want), "not the oracle's bytes under the slot's key"

    # first hand
    tables = [sit(c, b"table %d" % k) for k, c in enumerate(SEATS)]
    keys1 = seat(list(range(T)), tables)
    assert ks.live() == T
    first = hand(keys1)

    # the last player of tables 1 and 3 leaves, someone else sits down: two slots of five change
    for k in (1, 3):
        tables[k] = tables[k][:-1] + sit(1, b"table %d, second hand" % k)
    changed = seat([1, 3], [tables[1], tables[3]])
    keys2 = list(keys1)
    keys2[1], keys2[3] = changed
    assert keys2[1] != keys1[1] and keys2[3] != keys1[3] and ks.live() == T
    second = hand(keys2)

    # a proof of the first hand no longer verifies under table 1's index; table 0's still does
    cut = lambda d: [d[128 * i:128 * (i + 1)] for i in range(N)]      # noqa: E731
    stale = cards.verify_shuffle_chains(pp, [((ks, k), [cut(d) for d in first[0][k][:2]], first[1][k][:1]) for k in (0, 1)])
    assert stale[0] == [None] and isinstance(stale[1][0], mp.CryptoError), stale

    oracle_check(keys1[1], first[0][1], first[1][1], first[2][1])
    oracle_check(keys2[1], second[0][1], second[1][1], second[2][1])
    ks.close()
    t.close()
    print("%d tables, %d shuffles per hand, two hands; slots 1 and 3 re-seated between them" % (T, sum(SEATS)))
    print("reseat ok")


if __name__ == "__main__":
    main()
