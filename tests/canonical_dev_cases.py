"""Shared body of the tests of the device conversions between wire v1 and arkworks-canonical bytes that came after point and deck
decompression: mp_points_serialize_dev, mp_deck_serialize_dev, mp_proof_serialize_dev, mp_proof_deserialize_dev and the host-buffer forms
mp_decks_deserialize_batch / mp_proofs_deserialize_batch.  Run against the development emulator on CPU (tests/test_canonical_dev_emu.py)
and against the HIP engine on the GPU (tests/test_gpu_canonical_dev.py), the split of decompress_cases.py / test_gpu_decompress.py.

Expected bytes: for points the ORACLE's (the pool of tests/decompress_pool.py: entry.enc / entry.wire come from oracle/py/ark_canonical.py)
and the library's host functions (mp_points_serialize, mp_deck_serialize, mp_proof_serialize, mp_proof_deserialize), which the device
forms must reproduce byte for byte and verdict for verdict.  The layout of a canonical proof is restated here from
ark_canonical.enc_proof, not read from the library.

`mem` is the memory object of decompress_cases.py: put(bytes) / new(nbytes) -> (handle, address), get(handle, nbytes); fresh buffers hold
0x5A, so "written" and "zeroed" are observed."""
import ctypes
import random
import threading

import ark_canonical as ac
import mp_oracle as po

BAD_ENCODING, BAD_ARGUMENT = -1, -3
SYMBOLS = ["mp_points_serialize_dev", "mp_deck_serialize_dev", "mp_proof_serialize_dev", "mp_proof_deserialize_dev",
           "mp_decks_deserialize_batch", "mp_proofs_deserialize_batch"]


def statuses(b):
    return [int.from_bytes(b[i:i + 4], "little", signed=True) for i in range(0, len(b), 4)]


def convert(eng, mem, call, data, units, out_size):
    """one device call `call(d_in, d_out, d_status)` on fresh 0x5A buffers -> (output bytes, [status per unit])"""
    hin, pin = mem.put(data)
    hout, pout = mem.new(units * out_size)
    hst, pst = mem.new(4 * units)
    call(pin, pout, pst)
    eng.sync()
    return mem.get(hout, units * out_size), statuses(mem.get(hst, 4 * units))


def sizes(curve):
    cv = po.CURVES[curve]
    return 2 * cv.fq_bytes, ac.compressed_len(cv)


# ---- points ---------------------------------------------------------------------------------------------------------------------------
def points_serialize(eng, mem, curve, wire):
    PB, CB = sizes(curve)
    k = len(wire) // PB
    return convert(eng, mem, lambda i, o, s: eng.points_serialize_dev(k, i, o, s), wire, k, CB)


def points_deserialize(eng, mem, curve, data):
    PB, CB = sizes(curve)
    k = len(data) // CB
    return convert(eng, mem, lambda i, o, s: eng.points_deserialize_dev(k, i, o, s), data, k, PB)


def run_point_compression(eng, mem, ser, curve, pool):
    """every accepted entry of the pool, wire -> enc, in calls of 1, 63, 64, 65 points and of the whole pool: the bytes are the oracle's
    (entry.enc) and the host's (mp_points_serialize), and decompressing them on the device gives the wire bytes back"""
    good = [e for e in pool if e.ok]
    assert len(good) >= 32 and any(e.wire == bytes(len(e.wire)) for e in good)      # (infinity is among them)
    rng = random.Random(99)
    for n in (1, 63, 64, 65, len(good)):
        es = good if n == len(good) else rng.choices(good, k=n)      # (the secp256k1 pool has fewer than 63 accepted entries)
        wire = b"".join(e.wire for e in es)
        out, st = points_serialize(eng, mem, curve, wire)
        assert st == [0] * n, (curve, n, st)
        assert out == b"".join(e.enc for e in es), (curve, n)
        assert out == ser.points_serialize(wire), (curve, n)
        back, st = points_deserialize(eng, mem, curve, out)
        assert st == [0] * n and back == wire, (curve, n)


def run_point_range_checks(eng, mem, ser, NativeError, curve, pool):
    """coordinates at and beyond p: x = p, y = p, x = 2^(8 FB) - 1 are refused (status -1, all-zero slot, the call's other points
    untouched); y = p - 1 with x valid is accepted with the sign bit set (compression checks ranges only, as the host does)"""
    cv = po.CURVES[curve]
    PB, CB = sizes(curve)
    FB = PB // 2
    le = lambda v: v.to_bytes(FB, "little")
    good = [e for e in pool if e.ok and e.P is not None][:8]
    x, y = good[0].P
    cases = [(le(cv.p) + le(y), False), (le(x) + le(cv.p), False), (le((1 << (8 * FB)) - 1) + le(y), False),
             (le(x) + le((1 << (8 * FB)) - 1), False), (le(x) + le(cv.p - 1), True), (le(cv.p - 1) + le(1), True)]
    rows = [e.wire for e in good[:3]] + [c[0] for c in cases[:3]] + [good[3].wire] + [c[0] for c in cases[3:]] + [e.wire for e in good[4:]]
    ok = [True] * 3 + [c[1] for c in cases[:3]] + [True] + [c[1] for c in cases[3:]] + [True] * len(good[4:])
    out, st = points_serialize(eng, mem, curve, b"".join(rows))
    for k, (w, fine) in enumerate(zip(rows, ok)):
        slot = out[k * CB:(k + 1) * CB]
        if fine:
            assert st[k] == 0 and slot == ser.points_serialize(w), (curve, k, st[k], slot.hex())
        else:
            assert st[k] == BAD_ENCODING and slot == bytes(CB), (curve, k, st[k], slot.hex())
            try:
                ser.points_serialize(w)
                raise AssertionError("the host accepts a coordinate out of range")
            except NativeError as e:
                assert e.code == BAD_ENCODING
    signed = out[8 * CB:9 * CB]                                 # (x, p - 1): 2 y > p
    assert signed[-1] & 0x80 and not signed[-1] & 0x40, signed.hex()
    for k, w in enumerate(rows):                                # each of them alone: a call of one point
        o1, s1 = points_serialize(eng, mem, curve, w)
        assert (o1, s1) == (out[k * CB:(k + 1) * CB], [st[k]]), (curve, k)


# ---- decks ----------------------------------------------------------------------------------------------------------------------------
def run_deck_framing(eng, mem, ser, curve, pool, shapes=((1, 1), (1, 65), (2, 1), (2, 65), (52, 1), (52, 65))):
    """decks of 1, 2 and 52 cards in calls of 1 and 65 decks: u64 card count in front, mp_deck_serialize's bytes deck by deck, accepted
    by mp_deck_deserialize_dev with the wire bytes back; one coordinate out of range fails its own deck only"""
    cv = po.CURVES[curve]
    PB, CB = sizes(curve)
    good = [e for e in pool if e.ok]
    rng = random.Random(31)
    for cards, decks in shapes:
        per, dsz = 2 * cards, 8 + 2 * cards * CB
        wire = [b"".join(e.wire for e in rng.choices(good, k=per)) for _ in range(decks)]
        call = lambda i, o, s: eng.deck_serialize_dev(decks, cards, i, o, s)
        out, st = convert(eng, mem, call, b"".join(wire), decks, dsz)
        assert st == [0] * decks, (curve, cards, decks, st)
        for d in range(decks):
            got = out[d * dsz:(d + 1) * dsz]
            assert got[:8] == cards.to_bytes(8, "little") and got == ser.deck_serialize(wire[d]), (curve, cards, decks, d)
        back, st = convert(eng, mem, lambda i, o, s: eng.deck_deserialize_dev(decks, cards, i, o, s), out, decks, per * PB)
        assert st == [0] * decks and back == b"".join(wire), (curve, cards, decks)
        # y = p in one point of one deck
        d, j = decks // 2, per - 1
        bad = bytearray(wire[d])
        bad[j * PB + PB // 2:(j + 1) * PB] = cv.p.to_bytes(PB // 2, "little")
        out2, st2 = convert(eng, mem, call, b"".join(wire[:d] + [bytes(bad)] + wire[d + 1:]), decks, dsz)
        assert st2 == [BAD_ENCODING if k == d else 0 for k in range(decks)], (curve, cards, decks, st2)
        at = d * dsz + 8 + j * CB
        assert out2[at:at + CB] == bytes(CB) and out2[:at] == out[:at] and out2[at + CB:] == out[at + CB:], (curve, cards, decks)


# ---- proofs ---------------------------------------------------------------------------------------------------------------------------
def schema(m, n):
    """(kind, count, Vec length or None) per group, the order of ark_canonical.enc_proof: 14 groups of points, 13 of scalars, 11 Vecs"""
    P, S = "P", "S"
    return [(P, m, m), (P, m, m), (P, 1, None), (P, m, m), (P, 1, None), (P, 1, None), (P, 2 * m + 1, 2 * m + 1),
            (S, n, n), (S, n, n), (S, 1, None), (S, 1, None), (S, 1, None),
            (P, 1, None), (P, 1, None), (P, 1, None), (S, n, n), (S, n, n), (S, 1, None), (S, 1, None),
            (P, 1, None), (P, 2 * m, 2 * m), (P, 4 * m, 2 * m),
            (S, n, n), (S, 1, None), (S, 1, None), (S, 1, None), (S, 1, None)]


class Layout:
    """where the groups of a proof lie: per group (kind, prefix offset or None, Vec length, [canonical offsets], [wire offsets])"""

    def __init__(self, curve, m, n):
        PB, CB = sizes(curve)
        self.PB, self.CB, self.groups = PB, CB, []
        co = wo = 0
        for kind, count, vec in schema(m, n):
            pre = None
            if vec is not None:
                pre, co = co, co + 8
            cs, ws = (CB, PB) if kind == "P" else (32, 32)
            self.groups.append((kind, pre, vec, [co + i * cs for i in range(count)], [wo + i * ws for i in range(count)]))
            co, wo = co + count * cs, wo + count * ws
        self.canon_size, self.wire_size = co, wo
        assert co == ac.proof_serialized_size(po.CURVES[curve], m, n)
        assert wo == (11 * m + 8) * PB + (5 * n + 9) * 32


def proofs_serialize(eng, mem, curve, m, n, wire):
    lay = Layout(curve, m, n)
    B = len(wire) // lay.wire_size
    return convert(eng, mem, lambda i, o, s: eng.proof_serialize_dev(m, n, B, i, o, s), wire, B, lay.canon_size)


def proofs_deserialize(eng, mem, curve, m, n, data):
    lay = Layout(curve, m, n)
    B = len(data) // lay.canon_size
    return convert(eng, mem, lambda i, o, s: eng.proof_deserialize_dev(m, n, B, i, o, s), data, B, lay.wire_size)


def run_proof_round_trip(eng, mem, ser, curve, m, n, proofs, verify=None):
    """`proofs`: wire proofs.  mp_proof_serialize_dev gives mp_proof_serialize's bytes, mp_proof_deserialize_dev of those gives the wire
    proofs back with status 0, and what comes back verifies (verify: wire proofs -> status words of the existing verify call)"""
    lay = Layout(curve, m, n)
    B = len(proofs)
    canon, st = proofs_serialize(eng, mem, curve, m, n, b"".join(proofs))
    assert st == [0] * B, (curve, m, n, st)
    for k, p in enumerate(proofs):
        assert canon[k * lay.canon_size:(k + 1) * lay.canon_size] == ser.proof_serialize(m, n, p), (curve, m, n, k)
    wire, st = proofs_deserialize(eng, mem, curve, m, n, canon)
    assert st == [0] * B, (curve, m, n, st)
    assert wire == b"".join(proofs), (curve, m, n)
    if verify is not None:
        assert verify(wire) == [0] * B
    return canon


def refused_points(curve, pool):
    """one refused encoding of each family the decoders know: non-canonical x, bad flags, x not on the curve, and on BLS12-377 a point of
    the curve outside the prime-order subgroup"""
    cv = po.CURVES[curve]
    fam = {}
    for e in pool:
        if e.ok:
            continue
        x = int.from_bytes(e.enc[:-1] + bytes([e.enc[-1] & 0x3F]), "little")
        if e.enc[-1] & 0x40:
            kind = "flags"
        elif x >= cv.p:
            kind = "non-canonical x"
        elif e.x is not None and po.fq_sqrt(cv, (e.x ** 3 + cv.a * e.x + cv.b) % cv.p) is None:
            kind = "not on the curve"
        else:
            kind = "outside the subgroup"
        fam.setdefault(kind, e.enc)
    want = {"flags", "non-canonical x", "not on the curve"} | ({"outside the subgroup"} if curve == "bls12_377" else set())
    assert set(fam) == want, (curve, sorted(fam))
    return sorted(fam.items())


def proof_defects(curve, m, n, canon, wire, pool):
    """-> [(note, defective canonical proof, expected wire proof, accepted?)]: one defect each, in a proof otherwise `canon`.  Expected
    wire bytes: the clean ones with the refused element zeroed (a wrong length refuses the proof and zeroes nothing)"""
    cv = po.CURVES[curve]
    lay = Layout(curve, m, n)
    out = []

    def put(note, at, new, w_at=None, w_len=0, accepted=False, w_new=None):
        c = bytearray(canon)
        c[at:at + len(new)] = new
        w = bytearray(wire)
        if w_at is not None:
            w[w_at:w_at + w_len] = bytes(w_len) if w_new is None else w_new
        out.append((note, bytes(c), bytes(w), accepted))

    bad_pts = refused_points(curve, pool)
    rng = random.Random(5)
    for g, (kind, pre, vec, cos, wos) in enumerate(lay.groups):
        if pre is not None:
            for note, v in (("+1", vec + 1), ("-1", vec - 1), ("+2^32", vec + (1 << 32))):
                put("group %d length %s" % (g, note), pre, v.to_bytes(8, "little"))
        if kind == "P":
            i = rng.randrange(len(cos))
            for name, enc in bad_pts:
                put("group %d point %d: %s" % (g, i, name), cos[i], enc, wos[i], lay.PB)
        else:
            for i in sorted({0, len(cos) - 1}):
                for name, v in (("q", cv.q), ("2^256 - 1", (1 << 256) - 1)):
                    put("group %d scalar %d = %s" % (g, i, name), cos[i], v.to_bytes(32, "little"), wos[i], 32)
    kind, pre, vec, cos, wos = lay.groups[7]
    qm1 = (cv.q - 1).to_bytes(32, "little")
    put("scalar q - 1", cos[1], qm1, wos[1], 32, accepted=True, w_new=qm1)
    return out


def run_malformed_proofs(eng, mem, ser, NativeError, curve, m, n, wire, pool, lanes=65, per_batch=40, convert_batch=None):
    """batches of `lanes` proofs, one defect per defective lane, the other lanes clean: status -1 exactly on the refused lanes and the
    host's mp_proof_deserialize agrees lane by lane; the refused element is all-zero, every other element of that proof and every
    other proof byte-exact.  convert_batch(canonical bytes) -> (wire, status), if given, must return the same (the host-buffer form)"""
    lay = Layout(curve, m, n)
    canon = ser.proof_serialize(m, n, wire)
    assert ser.proof_deserialize(m, n, canon) == wire
    defects = proof_defects(curve, m, n, canon, wire, pool)
    lengths = [d for d in defects if "length" in d[0]]
    assert len(lengths) == 33 and sum(d[3] for d in defects) == 1
    rng, verdicts = random.Random(17), {}
    for lo in range(0, len(defects), per_batch):
        part = defects[lo:lo + per_batch]
        slots = sorted(rng.sample(range(lanes), len(part)))
        rows = [("clean", canon, wire, True)] * lanes
        for s, d in zip(slots, part):
            rows[s] = d
        data = b"".join(r[1] for r in rows)
        out, st = proofs_deserialize(eng, mem, curve, m, n, data)
        for k, (note, c, w, accepted) in enumerate(rows):
            if c not in verdicts:                                 # (the clean proof is judged once, not once per lane)
                try:
                    verdicts[c] = ser.proof_deserialize(m, n, c)
                except NativeError as e:
                    assert e.code == BAD_ENCODING
                    verdicts[c] = None
            host = verdicts[c]
            assert (host is not None) == accepted, (curve, note)
            assert st[k] == (0 if accepted else BAD_ENCODING), (curve, k, note, st[k])
            got = out[k * lay.wire_size:(k + 1) * lay.wire_size]
            assert got == w, (curve, k, note)
            assert host is None or host == got, (curve, k, note)
        if convert_batch is not None:
            assert convert_batch(data) == (out, st), (curve, lo)


def run_refusals(eng, mem, NativeError, curve, m=2, n=3):
    """null pointers, a zero count, cards > 4096, m < 2 and n < 2: MP_ERR_BAD_ARGUMENT, and no buffer is touched"""
    lay = Layout(curve, m, n)
    big = max(lay.canon_size, lay.wire_size, 4 * lay.PB)
    hin, pin = mem.new(big)
    hout, pout = mem.new(big)
    hst, pst = mem.new(16)
    calls = []
    for i, o, s in ((0, pout, pst), (pin, 0, pst), (pin, pout, 0)):
        calls += [lambda i=i, o=o, s=s: eng.points_serialize_dev(1, i, o, s), lambda i=i, o=o, s=s: eng.deck_serialize_dev(1, 1, i, o, s),
                  lambda i=i, o=o, s=s: eng.proof_serialize_dev(m, n, 1, i, o, s), lambda i=i, o=o, s=s: eng.proof_deserialize_dev(m, n, 1, i, o, s)]
    calls += [lambda: eng.points_serialize_dev(0, pin, pout, pst), lambda: eng.deck_serialize_dev(0, 1, pin, pout, pst),
              lambda: eng.deck_serialize_dev(1, 0, pin, pout, pst), lambda: eng.deck_serialize_dev(1, 4097, pin, pout, pst),
              lambda: eng.proof_serialize_dev(m, n, 0, pin, pout, pst), lambda: eng.proof_deserialize_dev(m, n, 0, pin, pout, pst),
              lambda: eng.proof_serialize_dev(1, n, 1, pin, pout, pst), lambda: eng.proof_serialize_dev(m, 1, 1, pin, pout, pst),
              lambda: eng.proof_deserialize_dev(1, n, 1, pin, pout, pst), lambda: eng.proof_deserialize_dev(m, 1, 1, pin, pout, pst)]
    lib, h = eng.lib, eng.h
    host_in, host_out, host_st = bytes(big), (ctypes.c_uint8 * big)(), (ctypes.c_int32 * 4)()
    raw = lambda rc: eng._chk(rc)
    calls += [lambda: raw(lib.mp_decks_deserialize_batch(h, 0, 1, host_in, host_out, host_st)),
              lambda: raw(lib.mp_decks_deserialize_batch(h, 1, 4097, host_in, host_out, host_st)),
              lambda: raw(lib.mp_decks_deserialize_batch(h, 1, 1, None, host_out, host_st)),
              lambda: raw(lib.mp_decks_deserialize_batch(h, 1, 1, host_in, None, host_st)),
              lambda: raw(lib.mp_decks_deserialize_batch(h, 1, 1, host_in, host_out, None)),
              lambda: raw(lib.mp_proofs_deserialize_batch(h, m, n, 0, host_in, host_out, host_st)),
              lambda: raw(lib.mp_proofs_deserialize_batch(h, 1, n, 1, host_in, host_out, host_st)),
              lambda: raw(lib.mp_proofs_deserialize_batch(h, m, 1, 1, host_in, host_out, host_st)),
              lambda: raw(lib.mp_proofs_deserialize_batch(h, m, n, 1, None, host_out, host_st)),
              lambda: raw(lib.mp_proofs_deserialize_batch(h, m, n, 1, host_in, None, host_st)),
              lambda: raw(lib.mp_proofs_deserialize_batch(h, m, n, 1, host_in, host_out, None))]
    for k, call in enumerate(calls):
        try:
            call()
            raise AssertionError("call %d was not refused" % k)
        except NativeError as e:
            assert e.code == BAD_ARGUMENT, (k, e)
    eng.sync()
    assert mem.get(hout, big) == b"\x5a" * big and mem.get(hst, 16) == b"\x5a" * 16 and mem.get(hin, big) == b"\x5a" * big
    assert bytes(host_out) == bytes(big)


def run_two_threads(eng, mem, curve, m, n, proofs, rounds=4):
    """two host threads on ONE context, one serialising and one deserialising proofs, each on buffers of its own: the bytes of every
    round equal the single-threaded ones"""
    lay = Layout(curve, m, n)
    B = len(proofs)
    wire = b"".join(proofs)
    canon, st = proofs_serialize(eng, mem, curve, m, n, wire)
    assert st == [0] * B
    assert proofs_deserialize(eng, mem, curve, m, n, canon) == (wire, st)
    got, errs = {"ser": [], "de": []}, []

    def work(name, fn, data):
        try:
            for _ in range(rounds):
                got[name].append(fn(eng, mem, curve, m, n, data))
        except Exception as e:      # noqa: BLE001 -- reported by the asserting thread
            errs.append(e)
    ts = [threading.Thread(target=work, args=("ser", proofs_serialize, wire)), threading.Thread(target=work, args=("de", proofs_deserialize, canon))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got["ser"] == [(canon, st)] * rounds and got["de"] == [(wire, st)] * rounds


def run_host_batch_forms(eng, mem, curve, m, n, canon_proofs, cards, canon_decks, pinned):
    """mp_proofs_deserialize_batch / mp_decks_deserialize_batch against the _dev forms on the same input (bytes and statuses)"""
    lay = Layout(curve, m, n)
    B = len(canon_proofs) // lay.canon_size
    assert eng.proofs_deserialize_batch(m, n, B, canon_proofs, pinned=pinned) == proofs_deserialize(eng, mem, curve, m, n, canon_proofs)
    dsz = 8 + 2 * cards * lay.CB
    D = len(canon_decks) // dsz
    dev = convert(eng, mem, lambda i, o, s: eng.deck_deserialize_dev(D, cards, i, o, s), canon_decks, D, 2 * cards * lay.PB)
    assert eng.decks_deserialize_batch(D, cards, canon_decks, pinned=pinned) == dev
    return dev


def defective_decks(curve, cards, pool, decks=7):
    """canonical decks, some refused (a wrong card count, a refused point), the rest accepted -> (bytes, [accepted?])"""
    rng = random.Random(23)
    good, bad = [e for e in pool if e.ok], [e for e in pool if not e.ok]
    rows, ok = [], []
    for d in range(decks):
        es = rng.choices(good, k=2 * cards)
        prefix = cards
        if d == 2:
            prefix = cards + 1
        if d == 4:
            es[rng.randrange(2 * cards)] = rng.choice(bad)
        rows.append(prefix.to_bytes(8, "little") + b"".join(e.enc for e in es))
        ok.append(d not in (2, 4))
    return b"".join(rows), ok


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def distinct_proofs(co, curve, m, n, K, seed=77):
    """K different proofs over ONE set of parameters, key and input deck (the C oracle proves: oracle/coracle.py), so that one table
    verifies them all -> (inputs, [shuffled deck], [wire proof])"""
    cv = po.CURVES[curve]
    g = co.gen_inputs(curve, m, n, seed)
    rng = random.Random(seed)
    shuffled, proofs = [], []
    for _ in range(K):
        perm = list(range(m * n))
        rng.shuffle(perm)
        w = dict(g, perm=perm, prover_seed=bytes(rng.randrange(256) for _ in range(32)),
                 rho=b"".join(rng.randrange(1, cv.q).to_bytes(32, "little") for _ in range(m * n)))
        d, p = co.shuffle_and_remask(curve, m, n, **w)
        shuffled.append(d)
        proofs.append(p)
    assert len(set(proofs)) == K
    return g, shuffled, proofs


def tiled(rows, B, seed=3):
    """B rows drawn from `rows` in a shuffled order that uses every one of them -> (indices, rows)"""
    idx = [k % len(rows) for k in range(B)]
    random.Random(seed).shuffle(idx)
    return idx, [rows[i] for i in idx]
