"""The device conversions between wire v1 and canonical bytes on the MI355X (kernels_canonical.hpp behind mp_points_serialize_dev,
mp_deck_serialize_dev, mp_proof_serialize_dev, mp_proof_deserialize_dev, mp_decks_deserialize_batch, mp_proofs_deserialize_batch): the
shared cases of tests/canonical_dev_cases.py, proofs from the device prover, calls cut into several launches, the Python mirror and
examples/canonical_verify.py.  Expected bytes are the oracle's and the host functions'; the emulator run of the same cases is
tests/test_canonical_dev_emu.py."""
import os
import subprocess
import sys

import pytest

import canonical_dev_cases as cc
import decompress_pool as dp
from conftest import GOLDEN, ROOT, load_json

pytestmark = pytest.mark.gpu

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
FIXTURES = ["shuffle_stark_m2_n3_s1.json", "shuffle_stark_m3_n4_s11.json", "shuffle_stark_m2_n26_s7.json", "shuffle_stark_m4_n13_s9.json",
            "shuffle_bn254_m2_n4_s3.json", "shuffle_secp256k1_m3_n3_s5.json", "shuffle_bls12_377_m2_n3_s13.json"]
MALFORMED = ["shuffle_stark_m2_n3_s1.json", "shuffle_bls12_377_m2_n3_s13.json", "shuffle_secp256k1_m3_n3_s5.json"]
LAUNCH = 1 << 20                  # points per launch of the proof decompressor (engine_core.hpp: proof_convert_device)
COMPRESS_LAUNCH = 1 << 22         # elements per launch of the compressor and of the scalar kernel (engine_core.hpp: CANON_LAUNCH)


class _TorchMem:
    """device buffers; fresh ones are filled with 0x5A so that "zeroed" and "written" are observed, not assumed"""

    def __init__(self):
        import torch
        self.torch, self.gpu = torch, torch.device("cuda", 0)

    def put(self, b):
        t = self.torch.frombuffer(bytearray(b), dtype=self.torch.uint8).to(self.gpu)
        self.torch.cuda.synchronize()
        return t, t.data_ptr()

    def new(self, nbytes):
        t = self.torch.full((max(nbytes, 4),), 0x5A, dtype=self.torch.uint8, device=self.gpu)
        self.torch.cuda.synchronize()      # the fill runs on torch's stream, the engine on its own: finish it before the engine zeroes
        return t, t.data_ptr()

    def get(self, h, nbytes):
        return bytes(h[:nbytes].cpu().numpy().tobytes())


@pytest.fixture(scope="module")
def engines(mp):
    """curve -> (engine, the library's host serialiser)"""
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = (mp._native.Engine(curve, 0), mp.Serializer(curve))
        return made[curve]
    yield get
    for e, _ in made.values():
        e.close()


@pytest.mark.parametrize("curve", CURVES)
def test_point_compression_on_the_device(engines, mp, curve):
    eng, ser = engines(curve)
    pool = dp.pool(curve)
    cc.run_point_compression(eng, _TorchMem(), ser, curve, pool)
    cc.run_point_range_checks(eng, _TorchMem(), ser, mp.NativeError, curve, pool)


@pytest.mark.parametrize("curve", CURVES)
def test_deck_framing_on_the_device(engines, curve):
    eng, ser = engines(curve)
    cc.run_deck_framing(eng, _TorchMem(), ser, curve, dp.pool(curve))


@pytest.mark.parametrize("name", FIXTURES)
def test_proof_conversion_on_the_fixtures(engines, mp, name):
    """the committed proofs through both directions, then through the verifier"""
    g = load_json(os.path.join(GOLDEN, name))
    curve, m, n = g["curve"], g["m"], g["n"]
    eng, ser = engines(curve)
    t = mp._native.Table(eng, m, n, bytes.fromhex(g["params"]), bytes.fromhex(g["pk"]))
    verify = lambda wire: t.verify_shuffle_batch(bytes.fromhex(g["deck"]), bytes.fromhex(g["shuffled"]), wire)
    cc.run_proof_round_trip(eng, _TorchMem(), ser, curve, m, n, [bytes.fromhex(g["proof"])], verify)
    t.close()


@pytest.fixture(scope="module")
def proved(engines, mp, coracle):
    """257 proofs of the device prover at (2, 3) on the STARK curve, one table -> (table, inputs, shuffled decks, proofs)"""
    import random
    m, n, B = 2, 3, 257
    eng, _ = engines("stark")
    g = coracle.gen_inputs("stark", m, n, 4)
    t = mp._native.Table(eng, m, n, g["params"], g["pk"])
    rng = random.Random(8)
    q = mp.protocol.CURVE_ORDERS["stark"]
    perms = []
    for _ in range(B):
        p = list(range(m * n))
        rng.shuffle(p)
        perms += p
    d, p, st = t.shuffle_and_remask_batch(g["deck"] * B, b"".join(rng.randrange(1, q).to_bytes(32, "little") for _ in range(B * m * n)),
                                          perms, bytes(rng.randrange(256) for _ in range(32 * B)))
    assert st == [0] * B
    ds, ps = len(d) // B, len(p) // B
    yield t, g, [d[k * ds:(k + 1) * ds] for k in range(B)], [p[k * ps:(k + 1) * ps] for k in range(B)]
    t.close()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_proof_conversion_on_the_prover_s_output(engines, proved, B):
    eng, ser = engines("stark")
    t, g, shuffled, proofs = proved
    verify = lambda wire: t.verify_shuffle_batch(g["deck"] * B, b"".join(shuffled[:B]), wire)
    cc.run_proof_round_trip(eng, _TorchMem(), ser, "stark", 2, 3, proofs[:B], verify)


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_proofs_on_the_device(engines, mp, name):
    """batches of 65 with one defect per defective lane (canonical_dev_cases.proof_defects), through mp_proof_deserialize_dev and through
    mp_proofs_deserialize_batch with pageable buffers"""
    g = load_json(os.path.join(GOLDEN, name))
    curve, m, n = g["curve"], g["m"], g["n"]
    eng, ser = engines(curve)
    batch = lambda data: eng.proofs_deserialize_batch(m, n, 65, data)
    cc.run_malformed_proofs(eng, _TorchMem(), ser, mp.NativeError, curve, m, n, bytes.fromhex(g["proof"]), dp.pool(curve), convert_batch=batch)


def _rows(torch, gpu, rows):
    import numpy as np
    return torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1).copy()).to(gpu)


def _first_bad(got, want):
    rows = (got != want).reshape(got.shape[0], -1).any(dim=1).nonzero()
    return None if rows.numel() == 0 else int(rows[0])


def test_proofs_across_launches(engines, proved):
    """2^20 // 30 + 70 proofs at (2, 3): the 30 points of one proof lie in two launches of 2^20 points.  Five valid proofs tiled over the
    call, a refused point in the straddling proof's second-launch half, a scalar = q in the last scalar of the last proof, a wrong Vec
    length elsewhere: exactly those three proofs read -1, their refused element is all-zero, everything else is byte-exact"""
    import torch
    curve, m, n = "stark", 2, 3
    eng, ser = engines(curve)
    gpu = torch.device("cuda", 0)
    lay = cc.Layout(curve, m, n)
    B, straddle = LAUNCH // 30 + 70, LAUNCH // 30
    assert straddle * 30 < LAUNCH < (straddle + 1) * 30 and LAUNCH - straddle * 30 <= 20
    wire = proved[3][:5]
    canon = [ser.proof_serialize(m, n, w) for w in wire]
    points = [(c, w) for kind, _, _, cos, wos in lay.groups if kind == "P" for c, w in zip(cos, wos)]
    scalars = [(c, w) for kind, _, _, cos, wos in lay.groups if kind == "S" for c, w in zip(cos, wos)]
    assert len(points) == 30 and len(scalars) == 24
    non_residue = next(e for e in dp.pool(curve) if not e.ok and e.E is not None)
    q = cc.po.CURVES[curve].q

    def damaged(k, c_at, new, w_at, w_len):
        c, w = bytearray(canon[k]), bytearray(wire[k])
        c[c_at:c_at + len(new)] = new
        w[w_at:w_at + w_len] = bytes(w_len)
        return bytes(c), bytes(w)
    bad = [damaged(0, points[20][0], non_residue.enc, points[20][1], lay.PB),           # point 20: lane 2^20 + 4 of the call
           damaged(1, scalars[-1][0], q.to_bytes(32, "little"), scalars[-1][1], 32),
           damaged(2, lay.groups[6][1], (2 * m + 1 + (1 << 32)).to_bytes(8, "little"), 0, 0)]
    enc, want_rows = _rows(torch, gpu, canon + [b[0] for b in bad]), _rows(torch, gpu, list(wire) + [b[1] for b in bad])
    idx = torch.arange(B, device=gpu) % 5
    idx[straddle], idx[B - 1], idx[17] = 5, 6, 7
    data = enc[idx].contiguous()
    want = want_rows[idx]
    want_st = torch.zeros(B, dtype=torch.int32, device=gpu)
    for k in (17, straddle, B - 1):
        want_st[k] = -1
    out = torch.full_like(want, 0x5A)
    st = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()      # inputs and preset buffers are written on torch's stream, the engine works on its own
    eng.proof_deserialize_dev(m, n, B, data.data_ptr(), out.data_ptr(), st.data_ptr())
    eng.sync()
    assert _first_bad(st, want_st) is None, st.nonzero().reshape(-1).tolist()
    assert _first_bad(out, want) is None, _first_bad(out, want)


def test_point_compression_across_launches(engines):
    """2^22 + 1 points, one more than a launch of the compressor takes: the accepted points of the pool and one with x = p tiled over
    the call; every status word and every output slot against the tiled expectation"""
    import torch
    curve = "stark"
    eng, _ = engines(curve)
    gpu = torch.device("cuda", 0)
    PB, CB = cc.sizes(curve)
    good = [e for e in dp.pool(curve) if e.ok]
    p = cc.po.CURVES[curve].p
    wire = _rows(torch, gpu, [e.wire for e in good] + [p.to_bytes(PB // 2, "little") + good[0].wire[PB // 2:]])
    enc = _rows(torch, gpu, [e.enc for e in good] + [bytes(CB)])
    code = torch.tensor([0] * len(good) + [-1], dtype=torch.int32, device=gpu)
    count = COMPRESS_LAUNCH + 1
    idx = torch.arange(count, device=gpu) % (len(good) + 1)
    assert int(idx[count - 1]) != len(good) and len(good) + 1 < COMPRESS_LAUNCH
    idx[count - 1] = len(good)                                  # the lone lane of the second launch is a refused one
    data = wire[idx].contiguous()
    out = torch.full((count, CB), 0x5A, dtype=torch.uint8, device=gpu)
    st = torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    eng.points_serialize_dev(count, data.data_ptr(), out.data_ptr(), st.data_ptr())
    eng.sync()
    assert _first_bad(st, code[idx]) is None
    assert _first_bad(out, enc[idx]) is None


@pytest.mark.parametrize("pinned", [False, True])
def test_host_batch_forms(engines, proved, pinned):
    """mp_proofs_deserialize_batch / mp_decks_deserialize_batch against the _dev forms, accepted and refused entries mixed, with pageable
    buffers and with buffers from mp_host_alloc"""
    eng, ser = engines("stark")
    m, n = 2, 3
    canon = [ser.proof_serialize(m, n, p) for p in proved[3][:3]]
    bad = bytearray(canon[1])
    bad[0] ^= 1                                                 # the first Vec length
    decks, ok = cc.defective_decks("stark", m * n, dp.pool("stark"))
    out, st = cc.run_host_batch_forms(eng, _TorchMem(), "stark", m, n, b"".join([canon[0], bytes(bad), canon[2], canon[1]]), m * n, decks, pinned)
    assert [s == 0 for s in st] == ok


def test_python_mirror_returns_an_error_per_refused_entry(mp, proved):
    """DLCards.deserialize_proofs / deserialize_decks: wire values for the accepted entries, a CardProtocolError.io for each refused one
    (wrong Vec length, refused point, wrong size), and what is accepted verifies"""
    t, g, shuffled, proofs = proved
    m, n = 2, 3
    cards = mp.DLCards("stark", device=0)
    ser = mp.Serializer("stark")
    pp = mp.Parameters(m, n, g["params"])
    canon = [cards.serialize_proof(pp, p) for p in proofs[:4]]
    bad = bytearray(canon[1])
    bad[0] ^= 1
    got = cards.deserialize_proofs(pp, [canon[0], bytes(bad), canon[2], canon[3][:-1], canon[3]])
    assert [isinstance(v, mp.CardProtocolError) for v in got] == [False, True, False, True, False]
    assert [got[0], got[2], got[4]] == [proofs[0], proofs[2], proofs[3]]
    decks, ok = cc.defective_decks("stark", m * n, dp.pool("stark"))
    dsz = len(decks) // len(ok)
    rows = cards.deserialize_decks(pp, [decks[k * dsz:(k + 1) * dsz] for k in range(len(ok))] + [b"\0" * 7])
    assert [not isinstance(v, mp.CardProtocolError) for v in rows] == ok + [False]
    for k, fine in enumerate(ok):
        if fine:
            assert ser.deck_serialize(b"".join(rows[k])) == decks[k * dsz:(k + 1) * dsz]
    cb = 2 * cards.engine.point_bytes
    sent = [ser.deck_serialize(s) for s in shuffled[:3]]
    back = cards.deserialize_decks(pp, sent)
    deck = [g["deck"][i * cb:(i + 1) * cb] for i in range(m * n)]
    assert cards.verify_shuffle_batch(pp, g["pk"], [deck] * 3, back, [got[0], proofs[1], got[2]]) == [None] * 3
    assert cards.deserialize_proofs(pp, []) == []


@pytest.mark.parametrize("curve", ["stark", "secp256k1"])
def test_refusals(engines, mp, curve):
    cc.run_refusals(engines(curve)[0], _TorchMem(), mp.NativeError, curve)


def test_two_threads_on_one_context(engines, proved):
    cc.run_two_threads(engines("stark")[0], _TorchMem(), "stark", 2, 3, proved[3][:33])


def test_canonical_verify_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "canonical_verify.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "canonical verify ok" in r.stdout
