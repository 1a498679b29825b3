"""Point decompression on the MI355X (k_decompress behind mp_points_deserialize_dev / mp_deck_deserialize_dev) on the inputs random points
miss: the structured pool of tests/decompress_pool.py (prescribed 2-Sylow digits, non-residues with a root, y at the sign rule's limb
boundaries, x at every edge, torsion on BLS12-377), the u64 length prefix, and calls long enough to be cut into several launches of
2^20 points.  Expected bytes and verdicts are the oracle's (oracle/py); cases and checks shared with the emulator run:
tests/decompress_cases.py, notes and the mutants these tests were tried against: tests/decompress_cases.md."""
import pytest

import decompress_cases as dc
import decompress_pool as dp

pytestmark = pytest.mark.gpu

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
LAUNCH = 1 << 20                  # points per launch of decompress_device (engine_core.hpp)


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
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = mp._native.Engine(curve, 0)
        return made[curve]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("curve", CURVES)
def test_structured_pool_on_the_device(engines, curve):
    """every family of the pool through launches of 1, 63, 64, 65 points and of the whole pool, exact against the oracle; the coverage the
    pool claims (every first non-zero window, every (window, digit) of Ghalf and (row, digit) of R twice, every limb that can decide the
    sign, every refused family) is asserted from the reference discrete logarithm first.  On BLS12-377 families a and b are not
    observable (decompress_pool.py): the digit pairs come from 200 random subgroup points there"""
    pool = dp.pool(curve)
    dp.assert_coverage(curve, pool)
    dc.run_pool_launches(engines(curve), _TorchMem(), curve, pool)


@pytest.mark.parametrize("curve", CURVES)
def test_length_prefix_and_small_decks_on_the_device(engines, curve):
    """cards +- 1, cards + 2^32, cards + 2^56 and 0 in the u64 prefix each fail their own deck only; decks of one card; calls of one deck"""
    dc.run_framing_cases(engines(curve), _TorchMem(), curve, dp.pool(curve))


def _pool_tensors(torch, gpu, curve, entries):
    import numpy as np
    as_t = lambda rows: torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1).copy()).to(gpu)
    return (as_t([e.enc for e in entries]), as_t([e.wire for e in entries]),
            torch.tensor([0 if e.ok else -1 for e in entries], dtype=torch.int32, device=gpu))


def _first_bad(torch, got, want):
    rows = (got != want).reshape(got.shape[0], -1).any(dim=1).nonzero()
    return None if rows.numel() == 0 else int(rows[0])


@pytest.mark.parametrize("count", [LAUNCH + 1, 2 * LAUNCH + 65])
@pytest.mark.parametrize("curve", ["stark", "secp256k1", "bls12_377"])
def test_points_across_launches(engines, curve, count):
    """a call of 2^20 + 1 and of 2 * 2^20 + 65 points is cut into two and three launches (a.first, a.lanes, the scratch stride): the pool,
    refused cases included, tiled over the call; every status word and every output slot against the tiled expectation"""
    import torch
    gpu = torch.device("cuda", 0)
    pool = dp.pool(curve)
    enc, wire, code = _pool_tensors(torch, gpu, curve, pool)
    n = len(pool)
    assert n < LAUNCH and count > (count - 1) // LAUNCH * LAUNCH >= LAUNCH          # every launch holds the whole pool, bad lanes too
    idx = torch.arange(count, device=gpu) % n
    data = enc[idx].contiguous()
    out = torch.full((count, wire.shape[1]), 0x5A, dtype=torch.uint8, device=gpu)
    st = torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    eng = engines(curve)
    torch.cuda.synchronize()      # inputs and preset buffers are written on torch's stream, the engine works on its own
    eng.points_deserialize_dev(count, data.data_ptr(), out.data_ptr(), st.data_ptr())
    eng.sync()
    k = _first_bad(torch, st, code[idx])
    assert k is None, (curve, count, k, pool[k % n], int(st[k]))
    k = _first_bad(torch, out, wire[idx])
    assert k is None, (curve, count, k, pool[k % n], bytes(out[k].cpu().numpy()).hex())


def test_decks_across_launches(engines):
    """52-card decks (104 points: 2^20 / 104 is not whole, so one deck has points in two launches), enough of them to pass 2^20 points;
    one refused point in the straddling deck's second-launch half, one as the last point of the last deck, one wrong prefix elsewhere:
    exactly those three decks read -1, their failing slot is all-zero, and every other slot of the call is byte-exact"""
    import torch
    curve, cards, decks = "stark", 52, 10100
    gpu = torch.device("cuda", 0)
    pool = dp.pool(curve)
    good = [e for e in pool if e.ok]
    bad = [e for e in pool if not e.ok and e.E is not None][:2] + [e for e in pool if not e.ok and e.E is None][:1]
    enc, wire, code = _pool_tensors(torch, gpu, curve, good + bad)
    per, ng = 2 * cards, len(good)
    straddle = LAUNCH // per
    assert straddle * per < LAUNCH < (straddle + 1) * per <= decks * per and straddle * per + 70 >= LAUNCH
    idx = (torch.arange(decks * per, device=gpu) % ng).reshape(decks, per).clone()
    idx[straddle, 70] = ng                                   # a non-residue with a root, in the second launch
    idx[decks - 1, per - 1] = ng + 2                         # refused before the square root
    prefix = torch.tensor(list(cards.to_bytes(8, "little")), dtype=torch.uint8, device=gpu).repeat(decks, 1)
    prefix[17, 4] = 1                                        # cards + 2^32
    data = torch.cat([prefix, enc[idx.reshape(-1)].reshape(decks, -1)], dim=1).contiguous()
    want = wire[idx.reshape(-1)].clone()
    want[17 * per] = 0
    want_st = torch.zeros(decks, dtype=torch.int32, device=gpu)
    for d in (17, straddle, decks - 1):
        want_st[d] = -1
    out = torch.full_like(want, 0x5A)
    st = torch.full((decks,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    eng = engines(curve)
    torch.cuda.synchronize()      # inputs and preset buffers are written on torch's stream, the engine works on its own
    eng.deck_deserialize_dev(decks, cards, data.data_ptr(), out.data_ptr(), st.data_ptr())
    eng.sync()
    assert _first_bad(torch, st, want_st) is None, st.nonzero().reshape(-1).tolist()
    k = _first_bad(torch, out, want)
    assert k is None, (k // per, k % per)
