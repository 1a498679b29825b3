"""Shared body of the on-device decompression tests (mp_points_deserialize_dev / mp_deck_deserialize_dev): run against the development
emulator on CPU (tests/test_cabi_and_host.py) and against the HIP engine on the GPU box (tests/test_gpu_round4.py,
tests/test_gpu_decompress.py), and of the host decoders' run over the same inputs (run_host_cases).  The expected bytes come from the
ORACLE's encoder / decoder (oracle/py/ark_canonical.py, big integers), not from the package.  The inputs random points miss come from
tests/decompress_pool.py; what is covered, what is not and the mutants the checks were tried against: tests/decompress_cases.md."""
import random

import ark_canonical as ac
import decompress_pool as dp
import mp_oracle as po


def run_decompress_cases(eng, mem, curve, golden, n_random=24, pool=None):
    """eng: _native.Engine; mem: object with put(bytes) -> (handle, address), new(nbytes) -> (handle, address), get(handle, nbytes) -> bytes;
    pool: the structured pool to add to the launch of single points (default: the curve's full pool of tests/decompress_pool.py)"""
    cv = po.CURVES[curve]
    L = ac.compressed_len(cv)
    rng = random.Random(4242)
    with po.curve_ctx(cv):
        PB = po.point_bytes()
        # ---- (1) the decks of the golden vector: serialised Vec<MaskedCard> -> wire decks, two decks in one call
        if golden is not None:
            m, n = golden["m"], golden["n"]
            wire = [bytes.fromhex(golden["deck"]), bytes.fromhex(golden["shuffled"])]
            data = b"".join(ac.enc_deck(cv, po.deck_from_bytes(w)) for w in wire)
            hin, pin = mem.put(data)
            hout, pout = mem.new(2 * len(wire[0]))
            hst, pst = mem.new(8)
            eng.deck_deserialize_dev(2, m * n, pin, pout, pst)
            eng.sync()
            assert mem.get(hst, 8) == bytes(8)
            assert mem.get(hout, 2 * len(wire[0])) == wire[0] + wire[1]
            # a wrong length prefix fails its deck only
            bad = bytearray(data)
            bad[0] ^= 1
            hin, pin = mem.put(bytes(bad))
            eng.deck_deserialize_dev(2, m * n, pin, pout, pst)
            eng.sync()
            st = mem.get(hst, 8)
            assert int.from_bytes(st[:4], "little", signed=True) == -1 and st[4:] == bytes(4)
        # ---- (2) single points: random multiples of G with both signs, infinity, and everything that must be refused
        pts, expect = [], []
        for _ in range(n_random):
            P = po.pt_mul(cv, rng.randrange(1, cv.q), cv.G)
            pts.append(ac.enc_point(cv, P))
            expect.append((0, po.pt_wire(P)))
        pts.append(ac.enc_point(cv, None))
        expect.append((0, bytes(PB)))
        x = 2
        while po.fq_sqrt(cv, (x * x * x + cv.a * x + cv.b) % cv.p) is not None:
            x += 1
        bad_list = [x.to_bytes(L, "little"),                                        # x not on the curve
                    cv.p.to_bytes(L, "little"),                                     # x = p: not canonical
                    (cv.p + cv.G[0]).to_bytes(L, "little") if (cv.p + cv.G[0]).bit_length() <= 8 * L - 2 else cv.p.to_bytes(L, "little"),
                    bytes([1]) + ac.enc_point(cv, None)[1:],                        # infinity flag with x != 0
                    ac.enc_point(cv, None)[:-1] + bytes([0xC0])]                    # infinity and sign flag
        if 8 * L - 2 > cv.p.bit_length():                                           # spare bits below the flags must be clear
            sp = bytearray(ac.enc_point(cv, cv.G))
            sp[-1] |= 0x20
            bad_list.append(bytes(sp))
        if curve == "bls12_377":                                                    # on the curve, outside the prime-order subgroup
            while True:
                xx = rng.randrange(cv.p)
                yy = po.fq_sqrt(cv, (xx * xx * xx + cv.a * xx + cv.b) % cv.p)
                if yy is None:
                    continue
                Q = po.pt_mul_raw(cv, cv.q, (xx, yy))
                if Q is not None:
                    break
            bad_list.append(ac.enc_point(cv, Q))
            bad_list.append(ac.enc_point(cv, po.pt_add(cv, Q, po.pt_mul(cv, 777, cv.G))))
        for b in bad_list:
            try:
                ac.dec_point(cv, b)
                raise AssertionError("the oracle decoder accepts a case meant to be refused: " + b.hex())
            except ac.DecodeError:
                pass
            pts.append(b)
            expect.append((-1, bytes(PB)))
        order = list(range(len(pts)))
        rng.shuffle(order)                                                          # bad encodings in the middle of a wave of good ones
        hin, pin = mem.put(b"".join(pts[i] for i in order))
        hout, pout = mem.new(len(pts) * PB)
        hst, pst = mem.new(4 * len(pts))
        eng.points_deserialize_dev(len(pts), pin, pout, pst)
        eng.sync()
        out, st = mem.get(hout, len(pts) * PB), mem.get(hst, 4 * len(pts))
        for k, i in enumerate(order):
            code = int.from_bytes(st[4 * k:4 * k + 4], "little", signed=True)
            assert (code, out[k * PB:(k + 1) * PB]) == expect[i], (curve, i, pts[i].hex(), code)
        # ---- (3) the structured pool (tests/decompress_pool.py): everything random points miss, one launch, good and refused lanes mixed
        if pool is None:
            pool = dp.pool(curve)
        run_points(eng, mem, curve, pool, rng)


def run_points(eng, mem, curve, entries, rng=None):
    """one mp_points_deserialize_dev call over `entries` (shuffled if `rng`): every status word and every output slot against the oracle.
    Status and output start from the memory object's non-zero fill, so "0 on success" and "all-zero slot on refusal" are observed"""
    cv = po.CURVES[curve]
    PB = 2 * cv.fq_bytes
    entries = list(entries)
    if rng is not None:
        rng.shuffle(entries)
    n = len(entries)
    hin, pin = mem.put(b"".join(e.enc for e in entries))
    hout, pout = mem.new(n * PB)
    hst, pst = mem.new(4 * n)
    eng.points_deserialize_dev(n, pin, pout, pst)
    eng.sync()
    out, st = mem.get(hout, n * PB), mem.get(hst, 4 * n)
    for k, e in enumerate(entries):
        code = int.from_bytes(st[4 * k:4 * k + 4], "little", signed=True)
        assert (code, out[k * PB:(k + 1) * PB]) == (0 if e.ok else -1, e.wire), (curve, k, e, code, out[k * PB:(k + 1) * PB].hex())


def run_pool_launches(eng, mem, curve, pool):
    """launches of 1, 63, 64, 65 points and of the whole pool, good and refused cases shuffled together: refused lanes skip the square
    root beside lanes that run it, below, at and above a wave of 64"""
    rng = random.Random(777)
    good, bad = [e for e in pool if e.ok], [e for e in pool if not e.ok]
    walkers = [e for e in bad if e.E is not None]           # refused after a full walk (non-residues, points outside the subgroup)
    for e in (rng.choice(good), rng.choice(bad), rng.choice(walkers)):
        run_points(eng, mem, curve, [e])
    for n in (63, 64, 65):
        for rep in range(2):
            nb = rng.randrange(n // 4, n // 2)
            run_points(eng, mem, curve, rng.sample(good, n - nb) + rng.sample(walkers, nb // 2) + rng.sample(bad, nb - nb // 2), rng)
    run_points(eng, mem, curve, pool, rng)


def deck_bytes(cv, prefix, entries):
    return int(prefix).to_bytes(8, "little") + b"".join(e.enc for e in entries)


def check_decks(eng, mem, curve, cards, decks):
    """decks: list of (prefix, entries); one mp_deck_deserialize_dev call.  A deck reads -1 iff its prefix is not `cards` or one of its
    points is refused; every point is decoded on its own (include/mpshuffle.h: "a failing point leaves an all-zero wire point"), and
    the point behind a wrong prefix counts as failing: slot for slot the output is the oracle's wire point or zeros"""
    cv = po.CURVES[curve]
    PB, per = 2 * cv.fq_bytes, 2 * cards
    assert all(len(es) == per for _, es in decks)
    hin, pin = mem.put(b"".join(deck_bytes(cv, pf, es) for pf, es in decks))
    hout, pout = mem.new(len(decks) * per * PB)
    hst, pst = mem.new(4 * len(decks))
    eng.deck_deserialize_dev(len(decks), cards, pin, pout, pst)
    eng.sync()
    out, st = mem.get(hout, len(decks) * per * PB), mem.get(hst, 4 * len(decks))
    for d, (pf, es) in enumerate(decks):
        code = int.from_bytes(st[4 * d:4 * d + 4], "little", signed=True)
        assert code == (0 if pf == cards and all(e.ok for e in es) else -1), (curve, cards, d, pf, code)
        for j, e in enumerate(es):
            want = bytes(PB) if (j == 0 and pf != cards) else e.wire
            assert out[(d * per + j) * PB:(d * per + j + 1) * PB] == want, (curve, cards, d, j, pf, e)


def run_framing_cases(eng, mem, curve, pool):
    """the u64 length prefix (all 8 bytes of it) and the deck / call sizes at the small end"""
    rng = random.Random(4711)
    good, bad = [e for e in pool if e.ok], [e for e in pool if not e.ok]
    cards = 3
    deck = lambda: rng.sample(good, 2 * cards)
    with_bad = deck()
    with_bad[4] = rng.choice([e for e in bad if e.E is not None])
    decks = [(cards, deck()), (cards + 1, deck()), (cards, deck()), (cards - 1, deck()), (cards + (1 << 32), deck()),
             (cards + (1 << 56), deck()), (0, deck()), (cards, with_bad), (cards, deck())]
    check_decks(eng, mem, curve, cards, decks)
    for i in range(len(decks)):                              # each of them alone: a call of one deck
        check_decks(eng, mem, curve, cards, decks[i:i + 1])
    one = lambda: rng.sample(good, 2)                        # decks of one card
    check_decks(eng, mem, curve, 1, [(1, one()), (2, one()), (1, one()), (0, one()), (1 + (1 << 32), one()), (1, [good[0], bad[0]]), (1, one())])
    check_decks(eng, mem, curve, 1, [(1, one())])


class _raises:
    """`with _raises(Exc):` -- the block must raise Exc (and carry `.code == code` if given)"""

    def __init__(self, exc, code=None):
        self.exc, self.code = exc, code

    def __enter__(self):
        return self

    def __exit__(self, tp, val, tb):
        assert tp is not None and issubclass(tp, self.exc), "refusal expected, got %r" % (val,)
        assert self.code is None or val.code == self.code, val
        return True


def run_host_cases(ser, NativeError, curve, pool):
    """ser: _native.Serializer (host code of the library: mp_points_deserialize / mp_points_serialize / mp_deck_deserialize)"""
    cv = po.CURVES[curve]
    good, bad = [e for e in pool if e.ok], [e for e in pool if not e.ok]
    join = lambda es: b"".join(e.enc for e in es)
    wires = lambda es: b"".join(e.wire for e in es)
    assert ser.points_deserialize(join(good)) == wires(good)                 # strided over the threads
    for lo in range(0, len(good), 15):                                       # one thread
        assert ser.points_deserialize(join(good[lo:lo + 15])) == wires(good[lo:lo + 15])
    for e in good:
        assert ser.points_deserialize(e.enc) == e.wire, e
    for e in bad:
        with _raises(NativeError):
            ser.points_deserialize(e.enc)
    walkers = [e for e in bad if e.E is not None]
    for n, where in ((10, (3,)), (15, (14,)), (16, (0,)), (16, (15,)), (100, (40,)), (100, (99,)), (100, (17, 18)), (100, (3, 64))):
        es = (good * 3)[:n]
        for j, i in enumerate(where):
            es[i] = walkers[j]
        with _raises(NativeError, -1):                            # MP_ERR_BAD_ENCODING
            ser.points_deserialize(join(es))
    # the compress direction: the oracle's flag bit for every y of the pool (points outside the subgroup included: compression does not judge)
    with po.curve_ctx(cv):
        pts = [e for e in pool if e.P is not None]
        assert len(pts) >= 16
        assert ser.points_serialize(b"".join(po.pt_wire(e.P) for e in pts)) == b"".join(ac.enc_point(cv, e.P) for e in pts) == join(pts)
        for e in pts:
            assert ser.points_serialize(po.pt_wire(e.P)) == e.enc, e
    # decks: Vec<MaskedCard>
    cards = 9
    assert ser.deck_deserialize(ac.enc_usize(cards) + join(good[:2 * cards])) == wires(good[:2 * cards])
    assert ser.deck_deserialize(ac.enc_usize(1) + join(good[:2])) == wires(good[:2])
    for prefix, es in ((cards + 1, good[:2 * cards]), (cards - 1, good[:2 * cards]), (cards + (1 << 32), good[:2 * cards]),
                       (cards + (1 << 56), good[:2 * cards]), (0, good[:2 * cards]), (cards, good[:2 * cards - 1] + walkers[:1]),
                       (cards, walkers[:1] + good[:2 * cards - 1]), (cards, good[:2 * cards - 1] + bad[-1:])):
        with _raises(NativeError):
            ser.deck_deserialize(ac.enc_usize(prefix) + join(es))


def run_tiled_points(eng, mem, curve, pool, count):
    """one mp_points_deserialize_dev call of `count` points, the pool (refused cases included) tiled over it: a call beyond 2^20 points
    is cut into launches, and every status word and output slot is compared with the tiled expectation"""
    cv = po.CURVES[curve]
    PB, n = 2 * cv.fq_bytes, len(pool)
    reps = -(-count // n)
    tile = lambda rows: (b"".join(rows) * reps)[:count * len(rows[0])]
    hin, pin = mem.put(tile([e.enc for e in pool]))
    hout, pout = mem.new(count * PB)
    hst, pst = mem.new(4 * count)
    eng.points_deserialize_dev(count, pin, pout, pst)
    eng.sync()
    out, st = mem.get(hout, count * PB), mem.get(hst, 4 * count)
    want_out = tile([e.wire for e in pool])
    want_st = tile([(0 if e.ok else -1).to_bytes(4, "little", signed=True) for e in pool])
    if st != want_st or out != want_out:
        k = next(k for k in range(count) if st[4 * k:4 * k + 4] != want_st[4 * k:4 * k + 4] or out[k * PB:(k + 1) * PB] != want_out[k * PB:(k + 1) * PB])
        raise AssertionError((curve, count, k, pool[k % n], st[4 * k:4 * k + 4].hex(), out[k * PB:(k + 1) * PB].hex()))
