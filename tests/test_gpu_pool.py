"""GPU tests of the device pool (mp_pool_*, include/mpshuffle.h): a batch cut into contiguous blocks over several contexts -- lanes of one
GPU here -- returns exactly the bytes and status words of the same call on one table [REF barnett-smart-card-protocol/examples/round.rs:
263-350: the players' shuffles are independent].  8-bit tables except where the shared fixed-base tables are measured.  The references
(one Table.shuffle_and_remask_batch call of 37 proofs, three proofs of the oracle) are computed once per module."""
import os
import random
import subprocess
import sys
import threading
from types import SimpleNamespace

import pytest

pytestmark = pytest.mark.gpu

CV, M, N_ = "stark", 2, 26
B = 37                                         # blocks 10 / 9 / 9 / 9 over four members
EDGES = (0, 9, 10, 18, 19, 27, 28, 36)         # first and last proof of every block


def _requests(coracle, curve, m, n, R, seed):
    g0 = coracle.gen_inputs(curve, m, n, seed)
    rnd = random.Random(seed)
    N = m * n
    rho, perms, seeds = [], [], []
    for _ in range(R):
        r = bytearray(rnd.randbytes(32 * N))
        for i in range(31, len(r), 32):
            r[i] &= 7
        p = list(range(N))
        rnd.shuffle(p)
        rho.append(bytes(r))
        perms.append(p)
        seeds.append(rnd.randbytes(32))
    return g0, rho, perms, seeds


def _args(c, n, perms=None):
    """the first n requests as the arguments of shuffle_and_remask_batch"""
    return c.deck * n, b"".join(c.rho[:n]), sum((perms or c.perms)[:n], []), b"".join(c.seeds[:n])


@pytest.fixture(scope="module")
def case(mp, coracle):
    g0, rho, perms, seeds = _requests(coracle, CV, M, N_, B, 8100)
    eng = mp._native.Engine(CV, 0)
    t = eng.table(M, N_, g0["params"], g0["pk"], fb_bits=8)
    pool = mp.Pool(CV, [0, 0, 0, 0])
    pt = pool.table(M, N_, g0["params"], g0["pk"], fb_bits=8)
    c = SimpleNamespace(mp=mp, g0=g0, rho=rho, perms=perms, seeds=seeds, deck=g0["deck"], eng=eng, t=t, pool=pool, pt=pt,
                        dsz=len(g0["deck"]), psz=t.proof_bytes)
    c.ref = t.shuffle_and_remask_batch(*_args(c, B))
    assert c.ref[2] == [0] * B
    yield c
    pt.close()
    pool.close()
    t.close()
    eng.close()


def test_sharding(case, coracle):
    """B = 37 (blocks 10/9/9/9), 3 (one member idle) and 1: the bytes of one Table call; proofs 0, 10 and 36 are the oracle's"""
    c = case
    for n, used in ((B, 4), (3, 3), (1, 1)):
        want = c.ref if n == B else c.t.shuffle_and_remask_batch(*_args(c, n))
        before = [c.pt.member_stats(i)["proofs"] for i in range(4)]
        got = c.pt.shuffle_and_remask_batch(*_args(c, n))
        assert got == want, n
        assert c.pt.stats()[2] == used and c.pt.stats()[4] == 4
        blocks = [c.pt.member_stats(i)["proofs"] - before[i] for i in range(4)]
        assert blocks == {B: [10, 9, 9, 9], 3: [1, 1, 1, 0], 1: [1, 0, 0, 0]}[n]
        assert c.pt.verify_shuffle_batch(c.deck * n, got[0], got[1]) == [0] * n
    for b in (0, 10, 36):
        d, p = coracle.shuffle_and_remask(CV, M, N_, c.g0["params"], c.g0["pk"], c.deck, c.rho[b], c.perms[b], c.seeds[b])
        assert (c.ref[0][b * c.dsz:(b + 1) * c.dsz], c.ref[1][b * c.psz:(b + 1) * c.psz]) == (d, p), b
    assert all(c.pt.member_stats(i)["device"] == 0 for i in range(4)) and c.pt.member_stats(0)["busy_us"] > 0


def test_verify_status_words(case):
    """a tampered response scalar, a swapped deck, an off-curve point (verify) and a non-permutation (prove) at the first and last proof
    of every block: the status words -- and so the check names -- of the single-table call; every other proof is accepted"""
    c = case
    decks, (shuf, proofs, _) = c.deck * B, c.ref

    def tamper_scalar(b, s, p):
        p[b * c.psz + c.psz - 31] ^= 2

    def swap_deck(b, s, p):
        o = (b + 1) % B
        s[b * c.dsz:(b + 1) * c.dsz] = shuf[o * c.dsz:(o + 1) * c.dsz]

    def off_curve(b, s, p):
        s[b * c.dsz + 32] ^= 1             # y of the shuffled deck's first point

    for name, fn, sign in (("scalar", tamper_scalar, 1), ("deck", swap_deck, 1), ("off-curve", off_curve, -1)):
        s, p = bytearray(shuf), bytearray(proofs)
        for b in EDGES:
            fn(b, s, p)
        want = c.t.verify_shuffle_batch(decks, bytes(s), bytes(p))
        got = c.pt.verify_shuffle_batch(decks, bytes(s), bytes(p))
        assert got == want, name
        assert [c.eng.check_name(v) for v in got] == [c.eng.check_name(v) for v in want]
        assert all((got[b] * sign > 0) if b in EDGES else got[b] == 0 for b in range(B)), (name, got)
    perms = [list(p) for p in c.perms]
    for b in EDGES:
        perms[b][1] = perms[b][0]
    want = c.t.shuffle_and_remask_batch(*_args(c, B, perms))
    got = c.pt.shuffle_and_remask_batch(*_args(c, B, perms))
    assert got == want
    assert [got[2][b] for b in EDGES] == [c.mp._native.MP_ERR_BAD_PERMUTATION] * len(EDGES)
    for b in set(range(B)) - set(EDGES):
        assert got[2][b] == 0 and got[1][b * c.psz:(b + 1) * c.psz] == c.ref[1][b * c.psz:(b + 1) * c.psz], b


def test_key_per_proof(case):
    """a keyless pool table with 5 keys: the bytes of tables created with those keys"""
    c, K = case, 5
    raw = c.eng.setup(2, K - 3, bytes(range(32)))
    keys = [raw[i * 64:(i + 1) * 64] for i in range(K)]
    ptl = c.pool.table(M, N_, c.g0["params"], None, fb_bits=8)
    d, p, st = ptl.shuffle_and_remask_batch(*_args(c, K), keys=b"".join(keys))
    assert st == [0] * K and ptl.stats()[2] == 4
    for k in range(K):
        tk = c.eng.table(M, N_, c.g0["params"], keys[k], fb_bits=8)
        dk, pk, sk = tk.shuffle_and_remask_batch(c.deck, c.rho[k], c.perms[k], c.seeds[k])
        tk.close()
        assert sk == [0] and (d[k * c.dsz:(k + 1) * c.dsz], p[k * c.psz:(k + 1) * c.psz]) == (dk, pk), k
    assert ptl.verify_shuffle_batch(c.deck * K, d, p, keys=b"".join(keys)) == [0] * K
    wrong = b"".join(keys[1:] + keys[:1])
    tl = c.eng.table(M, N_, c.g0["params"], None, fb_bits=8)
    want = tl.verify_shuffle_batch_keys(wrong, c.deck * K, d, p)
    tl.close()
    assert ptl.verify_shuffle_batch(c.deck * K, d, p, keys=wrong) == want and all(v > 0 for v in want)
    ptl.close()


def test_bls12_377(mp, coracle):
    """pool [0, 0], (2, 3), B = 5 on the 14-limb curve: 96-byte points in every slice offset; a point outside the prime-order subgroup
    keeps its single-table status"""
    import mp_oracle as po
    n = 5
    g0, rho, perms, seeds = _requests(coracle, "bls12_377", 2, 3, n, 8200)
    eng = mp._native.Engine("bls12_377", 0)
    t = eng.table(2, 3, g0["params"], g0["pk"], fb_bits=8)
    pool = mp.Pool("bls12_377", [0, 0])
    pt = pool.table(2, 3, g0["params"], g0["pk"], fb_bits=8)
    args = (g0["deck"] * n, b"".join(rho), sum(perms, []), b"".join(seeds))
    want = t.shuffle_and_remask_batch(*args)
    assert want[2] == [0] * n and pt.shuffle_and_remask_batch(*args) == want
    assert [pt.member_stats(i)["proofs"] for i in range(2)] == [3, 2]
    assert pt.verify_shuffle_batch(args[0], want[0], want[1]) == [0] * n
    cv = po.CURVES["bls12_377"]
    with po.curve_ctx(cv):
        x = 5
        while True:                      # a curve point that was not multiplied by the cofactor, times q: of order dividing the cofactor
            y = po.fq_sqrt(cv, (x ** 3 + cv.b) % cv.p)
            if y is not None and po.pt_mul_raw(cv, cv.q, (x, y)) is not None:
                break
            x += 1
        bad = po.pt_wire(po.pt_mul_raw(cv, cv.q, (x, y)))
    dsz = len(g0["deck"])
    decks = bytearray(args[0])
    decks[3 * dsz:3 * dsz + 96] = bad      # proof 3: the first proof of member 1's block
    bad_args = (bytes(decks),) + args[1:]
    want_p = t.shuffle_and_remask_batch(*bad_args)
    assert want_p[2] == [0, 0, 0, mp._native.MP_ERR_BAD_ENCODING, 0] and pt.shuffle_and_remask_batch(*bad_args) == want_p
    want_v = t.verify_shuffle_batch(bytes(decks), want[0], want[1])
    assert want_v == [0, 0, 0, mp._native.MP_ERR_BAD_ENCODING, 0] and pt.verify_shuffle_batch(bytes(decks), want[0], want[1]) == want_v
    pt.close()
    pool.close()
    t.close()
    eng.close()


def test_min_shard(case):
    """set_min_shard(16): 37 proofs take 2 members (blocks 19 / 18); the bytes do not change"""
    c = case
    c.pt.set_min_shard(16)
    try:
        before = [c.pt.member_stats(i)["proofs"] for i in range(4)]
        assert c.pt.shuffle_and_remask_batch(*_args(c, B)) == c.ref
        assert c.pt.stats()[2] == 2
        assert [c.pt.member_stats(i)["proofs"] - before[i] for i in range(4)] == [19, 18, 0, 0]
    finally:
        c.pt.set_min_shard(1)
    with pytest.raises(c.mp.NativeError):
        c.pt.set_min_shard(0)


def test_shared_tables(case):
    """four lanes at 16 bits build the fixed-base tables once and hold them once: free HBM drops by less than twice what one plain 16-bit
    table takes (unshared it would be four times)"""
    import torch
    c = case

    def free():
        return torch.cuda.mem_get_info(0)[0]

    f0 = free()
    t16 = c.eng.table(M, N_, c.g0["params"], c.g0["pk"], fb_bits=16)
    one = f0 - free()
    t16.close()
    f1 = free()
    pt16 = c.pool.table(M, N_, c.g0["params"], c.g0["pk"], fb_bits=16)
    four = f1 - free()
    print("one 16-bit table: %.0f MB; pool table of four lanes: %.0f MB" % (one / 2**20, four / 2**20))
    assert pt16.stats()[3] == 1 and [pt16.member(i).fb_bits for i in range(4)] == [16] * 4
    assert one > 2**30 and four < 2 * one, (one, four)
    assert pt16.shuffle_and_remask_batch(*_args(c, 5)) == tuple(x[:5 * k] for x, k in zip(c.ref, (c.dsz, c.psz, 1)))
    pt16.close()


def test_errors(case):
    """a device that does not exist, 0 and 65 members, a null buffer, a keyless table without keys"""
    c, nat = case, case.mp._native
    with pytest.raises(nat.NoDeviceError) as e:
        c.mp.Pool(CV, [0, 99])
    assert "member 1 (device 99)" in str(e.value)
    for devs in ([], [0] * 65):
        with pytest.raises(nat.NativeError) as e:
            c.mp.Pool(CV, devs)
        assert e.value.code == nat.MP_ERR_BAD_ARGUMENT
    import ctypes
    lib = c.t.lib
    decks, rho, perms, seeds = _args(c, 2)
    buf = lambda b: (ctypes.c_uint8 * len(b)).from_buffer_copy(b)      # noqa: E731
    pm = (ctypes.c_uint32 * len(perms))(*perms)
    od, op, st = (ctypes.c_uint8 * (2 * c.dsz))(), (ctypes.c_uint8 * (2 * c.psz))(), (ctypes.c_int32 * 2)()
    calls = c.pt.stats()[0]
    want = lib.mp_shuffle_and_remask_batch(c.t.h, 2, None, buf(rho), pm, buf(seeds), od, op, st)
    text = lib.mp_last_error()
    assert want < 0 and lib.mp_pool_shuffle_and_remask_batch(c.pt.h, 2, None, None, buf(rho), pm, buf(seeds), od, op, st) == want
    assert lib.mp_last_error() == text
    want = lib.mp_verify_shuffle_batch(c.t.h, 2, buf(decks), buf(decks), buf(bytes(2 * c.psz)), None)
    assert want < 0 and lib.mp_pool_verify_shuffle_batch(c.pt.h, 2, None, buf(decks), buf(decks), buf(bytes(2 * c.psz)), None) == want
    assert c.pt.stats()[0] == calls
    tl = c.eng.table(M, N_, c.g0["params"], None, fb_bits=8)
    ptl = c.pool.table(M, N_, c.g0["params"], None, fb_bits=8)
    codes = []
    for x in (tl, ptl):
        with pytest.raises(nat.NativeError) as e:
            x.shuffle_and_remask_batch(decks, rho, perms, seeds)
        codes.append((e.value.code, str(e.value)))
        with pytest.raises(nat.NativeError) as e:
            x.verify_shuffle_batch(decks, decks, bytes(2 * c.psz))
        codes.append((e.value.code, str(e.value)))
    assert codes[:2] == codes[2:] and codes[0][0] == nat.MP_ERR_BAD_ARGUMENT
    with pytest.raises(nat.NativeError) as e:      # a member build that fails: the member is named, nothing is left
        c.pool.table(1, N_, c.g0["params"], c.g0["pk"], fb_bits=8)
    assert e.value.code == nat.MP_ERR_BAD_ARGUMENT and "member 0 (device 0)" in str(e.value)
    ptl.close()
    tl.close()


def test_two_python_threads(case):
    """two threads call the pool at once, 6 iterations each: every call returns the single-threaded bytes"""
    c = case
    errors = []

    def body(k):
        try:
            for _ in range(6):
                assert c.pt.shuffle_and_remask_batch(*_args(c, B)) == c.ref
                assert c.pt.verify_shuffle_batch(c.deck * B, c.ref[0], c.ref[1]) == [0] * B
        except Exception as e:      # (reported below: an assertion in a thread does not fail the test by itself)
            errors.append((k, repr(e)))

    th = [threading.Thread(target=body, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


def test_dlcards_devices(case):
    """DLCards(devices=[0, 0]): the batch members give the bytes of DLCards(); the single-proof members run on member 0"""
    c, mp, n = case, case.mp, 5
    pp = mp.Parameters(M, N_, c.g0["params"])
    N = M * N_
    deck = [c.deck[i * 128:(i + 1) * 128] for i in range(N)]
    rho = [[int.from_bytes(r[i * 32:(i + 1) * 32], "little") for i in range(N)] for r in c.rho[:n]]
    perms = [mp.Permutation(p) for p in c.perms[:n]]
    raw = c.eng.setup(2, n - 3, bytes(range(32)))
    keys = [raw[i * 64:(i + 1) * 64] for i in range(n)]
    plain, pooled = mp.DLCards(CV, device=0), mp.DLCards(CV, devices=[0, 0])
    assert pooled.pool is not None and plain.pool is None
    a = plain.shuffle_and_remask_batch(c.seeds[:n], pp, c.g0["pk"], [deck] * n, rho, perms)
    b = pooled.shuffle_and_remask_batch(c.seeds[:n], pp, c.g0["pk"], [deck] * n, rho, perms)
    assert a == b and b"".join(b[4][0]) == c.ref[0][4 * c.dsz:5 * c.dsz] and b[4][1] == c.ref[1][4 * c.psz:5 * c.psz]
    proofs = [x[1] for x in b]
    proofs[3] = proofs[3][:-31] + bytes([proofs[3][-31] ^ 2]) + proofs[3][-30:]
    va = plain.verify_shuffle_batch(pp, c.g0["pk"], [deck] * n, [x[0] for x in a], proofs)
    vb = pooled.verify_shuffle_batch(pp, c.g0["pk"], [deck] * n, [x[0] for x in b], proofs)
    assert [repr(v) for v in va] == [repr(v) for v in vb] and [v is None for v in vb] == [True, True, True, False, True]
    ak = plain.shuffle_and_remask_batch_keys(c.seeds[:n], pp, keys, [deck] * n, rho, perms)
    bk = pooled.shuffle_and_remask_batch_keys(c.seeds[:n], pp, keys, [deck] * n, rho, perms)
    assert ak == bk and ak != a
    assert pooled.verify_shuffle_batch_keys(pp, keys, [deck] * n, [x[0] for x in bk], [x[1] for x in bk]) == [None] * n
    assert pooled.table(pp, c.g0["pk"]).pool_table.stats()[:3] == [2, 2 * n, 2]
    assert pooled.shuffle_and_remask(c.seeds[0], pp, c.g0["pk"], deck, rho[0], perms[0]) == a[0]
    assert pooled.verify_shuffle(pp, c.g0["pk"], deck, a[0][0], a[0][1]) is None


def test_example_runs():
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pool.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "pool ok" in out.stdout and "member 3: {'device': 0" in out.stdout, out.stdout + out.stderr


def test_two_devices(case):
    """one member on each of two GPUs: the sharding case once more (skipped on a machine with one GPU)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: torch.cuda.device_count() = %d" % torch.cuda.device_count())
    c = case
    pool = c.mp.Pool(CV, [0, 1])
    pt = pool.table(M, N_, c.g0["params"], c.g0["pk"], fb_bits=8)
    assert pt.shuffle_and_remask_batch(*_args(c, B)) == c.ref
    assert pt.stats()[2:5] == [2, 2, 2] and [pt.member_stats(i)["device"] for i in range(2)] == [0, 1]
    assert pt.verify_shuffle_batch(c.deck * B, c.ref[0], c.ref[1]) == [0] * B
    pt.close()
    pool.close()


def test_cpp_driver(tmp_path):
    """tests/cpp/pool_threads.cpp against libmpshuffle.so: the scenarios of tests/test_pool_tsan.py on the device, and
    include/barnett_smart.hpp with a device list"""
    from conftest import ROOT
    exe = tmp_path / "pool_threads"
    libdir = os.path.join(ROOT, "mental-poker_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pool_threads.cpp"), "-L", libdir, "-lmpshuffle", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "pool ok" in out.stdout, out.stdout + out.stderr
