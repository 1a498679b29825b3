#!/usr/bin/env python3
"""A verifier that holds everything as arkworks-canonical bytes, as every caller of the reference's trait does (all associated types
are CanonicalSerialize + CanonicalDeserialize [REF barnett-smart-card-protocol/src/lib.rs:45-71]): a batch of input decks, shuffled decks
and shuffle proofs (m=2, n=26) arrives compressed, is converted to the engine's wire format ON THE DEVICE by the two batch forms
(DLCards.deserialize_decks / deserialize_proofs: mp_decks_deserialize_batch / mp_proofs_deserialize_batch -- one square root per point,
none of them on the host) and verified with verify_shuffle_batch.  One proof and one deck are damaged on the way: they come back as
errors of their own entries, and everything else verifies."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")


def main():
    m, n, batch = 2, 26, 64
    cards = mp.DLCards("stark", device=0)
    ser = mp.Serializer("stark")
    rng = mp.ChaCha20Rng(b"canonical verify example".ljust(32, b"\0"))
    fresh = lambda: b"".join(rng.next_u64().to_bytes(8, "little") for _ in range(4))     # noqa: E731
    pp = cards.setup(fresh(), m, n)
    (joint, _), = cards.player_keygen_batch([fresh()], pp)

    # the other side of the wire: shuffles made somewhere, serialised the arkworks way
    plain = cards.setup(fresh(), m, m * n).raw
    dealt = cards.deal([fresh() for _ in range(m * n)], pp, [joint], [0] * (m * n), [plain[64 * i:64 * (i + 1)] for i in range(m * n)],
                       [1] * (m * n))
    deck = [d[0] for d in dealt]
    made = cards.shuffle_and_remask_batch_seeded([fresh() for _ in range(batch)], pp, joint, [deck] * batch)
    sent_decks = [ser.deck_serialize(b"".join(deck))] * batch
    sent_shuffled = [ser.deck_serialize(b"".join(s)) for s, _ in made]
    sent_proofs = [cards.serialize_proof(pp, p) for _, p in made]
    damaged_proof, damaged_deck = 5, 9
    sent_proofs[damaged_proof] = (m + 1).to_bytes(8, "little") + sent_proofs[damaged_proof][8:]      # a Vec of commitments one too long
    sent_shuffled[damaged_deck] = (m * n + 1).to_bytes(8, "little") + sent_shuffled[damaged_deck][8:]

    # this side: canonical bytes in, verdicts out
    t0 = time.time()
    decks = cards.deserialize_decks(pp, sent_decks)
    shuffled = cards.deserialize_decks(pp, sent_shuffled)
    proofs = cards.deserialize_proofs(pp, sent_proofs)
    t1 = time.time()
    refused = [k for k in range(batch) if any(isinstance(v[k], Exception) for v in (decks, shuffled, proofs))]
    assert refused == [damaged_proof, damaged_deck], refused
    keep = [k for k in range(batch) if k not in refused]
    verdicts = cards.verify_shuffle_batch(pp, joint, [decks[k] for k in keep], [shuffled[k] for k in keep], [proofs[k] for k in keep])
    t2 = time.time()
    assert verdicts == [None] * len(keep), verdicts
    assert proofs[0] == made[0][1] and shuffled[0] == made[0][0]

    size = len(sent_proofs[0]) + len(sent_decks[0]) + len(sent_shuffled[0])
    print("%d shuffles as canonical bytes (%d bytes each): converted on the device in %.1f ms, verified in %.1f ms"
          % (batch, size, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    print("entries %s refused at conversion: %s" % (refused, proofs[damaged_proof]))
    print("canonical verify ok")


if __name__ == "__main__":
    main()
