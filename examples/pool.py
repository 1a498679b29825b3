#!/usr/bin/env python3
"""Eight card tables with their own aggregate keys, shuffled and verified in one sharded call each on a device pool (m=2, n=26).

The pool is four members on device 0 -- four lanes that run side by side on the chip; `python examples/pool.py 0 1` puts one member on
each of two GPUs instead.  One keyless pool table holds the parameters the card tables share (the lanes of a device share one set of
fixed-base tables); every proof names its table's key.  The call cuts the eight proofs into contiguous blocks over the members and
returns the bytes one context would [REF barnett-smart-card-protocol/examples/round.rs:263-350: the players' shuffles are independent]."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")


def main(devices):
    m, n, N, tables = 2, 26, 52, 8
    pool = mp.Pool("stark", devices)
    eng = pool.engine(0)
    rng = mp.ChaCha20Rng(b"pool example".ljust(32, b"\0"))      # stands for the players' CSPRNGs
    fresh = lambda: b"".join(rng.next_u64().to_bytes(8, "little") for _ in range(4))     # noqa: E731
    params = eng.setup(m, n, fresh())
    points = eng.setup(m, tables + 2 * N - 3, fresh())               # independent points: 8 aggregate keys and one open deck
    keys, deck = points[:64 * tables], points[64 * tables:]
    pt = pool.table(m, n, params)                                    # keyless: one aggregate key per proof

    factors = b"".join((mp.fr_rand("stark", rng)).to_bytes(32, "little") for _ in range(tables * N))
    perms = []
    for _ in range(tables):
        p = list(range(N))
        for i in range(N - 1, 0, -1):
            j = rng.next_u64() % (i + 1)
            p[i], p[j] = p[j], p[i]
        perms += p
    seeds = b"".join(fresh() for _ in range(tables))

    shuffled, proofs, status = pt.shuffle_and_remask_batch(deck * tables, factors, perms, seeds, keys=keys)
    assert status == [0] * tables, status
    assert pt.verify_shuffle_batch(deck * tables, shuffled, proofs, keys=keys) == [0] * tables
    wrong = keys[64:] + keys[:64]                                    # every proof under its neighbour's key: all rejected
    assert all(s > 0 for s in pt.verify_shuffle_batch(deck * tables, shuffled, proofs, keys=wrong))

    # the same proofs from one context: a sharded call returns exactly these bytes
    one = pt.member(0).shuffle_and_remask_batch_keys(keys, deck * tables, factors, perms, seeds)
    assert one == (shuffled, proofs, status)

    st = pt.stats()
    print("pool of %d members on devices %s: %d calls, %d proofs, %d members used by the last call, %d fixed-base build(s)"
          % (st[4], devices, st[0], st[1], st[2], st[3]))
    for i in range(len(pool)):
        print("  member %d: %s" % (i, pt.member_stats(i)))
    pt.close()
    pool.close()
    print("pool ok")


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [0, 0, 0, 0])
