"""GPU tests of request coalescing (mp_set_coalesce, include/mpshuffle.h): many host threads making one proof per call, as callers of the
reference's trait do [REF barnett-smart-card-protocol/src/lib.rs:181-197], share batched calls -- same bytes as the oracle and as the
uncoalesced calls, a tampered request rejected alone with its own check name, batches of many requests, and the rate that buys."""
import os
import random
import subprocess
import threading
import time

import pytest

pytestmark = pytest.mark.gpu

CV, M, N_ = "stark", 2, 26


def _requests(coracle, R, seed):
    g0 = coracle.gen_inputs(CV, M, N_, seed)
    rnd = random.Random(seed)
    N = M * N_
    reqs = []
    for _ in range(R):
        rho = bytearray(rnd.randbytes(32 * N))
        for i in range(31, len(rho), 32):
            rho[i] &= 7
        perm = list(range(N))
        rnd.shuffle(perm)
        reqs.append(dict(deck=g0["deck"], rho=bytes(rho), perm=perm, prover_seed=rnd.randbytes(32)))
    return g0, reqs


def _run_threads(T, fn):
    errors = []
    barrier = threading.Barrier(T)

    def body(r):
        try:
            barrier.wait()
            fn(r)
        except Exception as e:      # (reported below: an assertion in a thread does not fail the test by itself)
            errors.append((r, repr(e)))

    th = [threading.Thread(target=body, args=(r,)) for r in range(T)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    assert not errors, errors[:5]
    return dt


def test_256_threads_one_table(mp, coracle):
    """256 Python threads, each 4 x (shuffle_and_remask + verify_shuffle) on one table with coalescing (256, 1 000 us): outputs equal
    the batched call's and, sampled, the oracle's; one tampered request per round is rejected alone with its own check name; batches of
    at least 16 requests on average; at least 10x the rate of one thread making one proof per call"""
    T, ROUNDS = 256, 4
    g0, reqs = _requests(coracle, T, 7100)
    eng = mp._native.Engine(CV, 0)
    t = eng.table(M, N_, g0["params"], g0["pk"], fb_bits=16)
    dsz, psz = len(g0["deck"]), t.proof_bytes
    ref_d, ref_p, st = t.shuffle_and_remask_batch(b"".join(r["deck"] for r in reqs), b"".join(r["rho"] for r in reqs),
                                                  sum((r["perm"] for r in reqs), []), b"".join(r["prover_seed"] for r in reqs))
    assert st == [0] * T
    ref = [(ref_d[r * dsz:(r + 1) * dsz], ref_p[r * psz:(r + 1) * psz]) for r in range(T)]
    for r in (0, 77, 255):
        q = reqs[r]
        assert ref[r] == coracle.shuffle_and_remask(CV, M, N_, g0["params"], g0["pk"], q["deck"], q["rho"], q["perm"], q["prover_seed"])
    bad = {}
    for k in range(ROUNDS):
        r = (37 + 61 * k) % T
        p = bytearray(ref[r][1])
        p[psz - 31 - 32 * k] ^= 2
        code = t.verify_shuffle(reqs[r]["deck"], ref[r][0], bytes(p))          # uncoalesced: what the tampered request must get
        assert code > 0
        bad[(k, r)] = (bytes(p), eng.check_name(code))
    # one thread, one proof per call, coalescing off: the B = 1 rate
    t0 = time.perf_counter()
    for r in range(8):
        q = reqs[r]
        assert t.shuffle_and_remask(q["deck"], q["rho"], q["perm"], q["prover_seed"]) == ref[r]
        assert t.verify_shuffle(q["deck"], ref[r][0], ref[r][1]) == 0
    single_rate = 8 / (time.perf_counter() - t0)

    t.set_coalesce(256, 1000)

    def worker(r):
        q = reqs[r]
        for k in range(ROUNDS):
            d, p = t.shuffle_and_remask(q["deck"], q["rho"], q["perm"], q["prover_seed"])
            assert (d, p) == ref[r], r
            if (k, r) in bad:
                code = t.verify_shuffle(q["deck"], d, bad[(k, r)][0])
                assert code > 0 and eng.check_name(code) == bad[(k, r)][1], (r, code)
            else:
                assert t.verify_shuffle(q["deck"], d, p) == 0, r

    dt = _run_threads(T, worker)
    s = t.coalesce_stats()
    rate = T * ROUNDS / dt
    print("coalesced: %.0f proofs/s (prove + verify), one thread at B = 1: %.0f proofs/s, stats %s" % (rate, single_rate, s))
    assert s["served"] == 2 * T * ROUNDS and s["rerun"] == 0
    assert s["served"] / s["batches"] >= 16, s
    assert rate >= 10 * single_rate, (rate, single_rate)
    t.close()
    eng.close()


def test_dlcards_coalesced_many_keys(mp, coracle):
    """DLCards(coalesce=(256, 1000)): 128 threads with 32 distinct aggregate keys share ONE table of the parameters; bytes equal those of
    tables created per key, and the proofs verify with the oracle"""
    T, K = 128, 32
    g0, reqs = _requests(coracle, T, 7200)
    cards = mp.DLCards(CV, device=0, coalesce=(256, 1000))
    keys_raw = cards.engine.setup(2, K - 3, bytes(range(32)))          # K independent points as the aggregate keys
    keys = [keys_raw[i * 64:(i + 1) * 64] for i in range(K)]
    pp = mp.Parameters(M, N_, g0["params"])
    eng = cards.engine
    ref = {}
    for k in range(K):                                                 # per-key tables, batched: the bytes each request must get
        t = eng.table(M, N_, g0["params"], keys[k], fb_bits=8)
        mine = list(range(k, T, K))
        d, p, st = t.shuffle_and_remask_batch(b"".join(reqs[r]["deck"] for r in mine), b"".join(reqs[r]["rho"] for r in mine),
                                              sum((reqs[r]["perm"] for r in mine), []), b"".join(reqs[r]["prover_seed"] for r in mine))
        assert st == [0] * len(mine)
        for j, r in enumerate(mine):
            ref[r] = (d[j * len(g0["deck"]):(j + 1) * len(g0["deck"])], p[j * t.proof_bytes:(j + 1) * t.proof_bytes])
        t.close()
    out = {}

    def worker(r):
        q = reqs[r]
        deck = [q["deck"][i * 128:(i + 1) * 128] for i in range(M * N_)]
        rho = [int.from_bytes(q["rho"][i * 32:(i + 1) * 32], "little") for i in range(M * N_)]
        shuffled, proof = cards.shuffle_and_remask(q["prover_seed"], pp, keys[r % K], deck, rho, mp.Permutation(q["perm"]))
        assert (b"".join(shuffled), proof) == ref[r], r
        assert cards.verify_shuffle(pp, keys[r % K], deck, shuffled, proof) is None
        with pytest.raises(mp.CryptoError):
            cards.verify_shuffle(pp, keys[(r + 1) % K], deck, shuffled, proof)
        out[r] = (b"".join(shuffled), proof)

    _run_threads(T, worker)
    assert len(cards._params_tables) == 1 and not cards._tables
    s = cards.params_table(pp).coalesce_stats()
    print("DLCards, %d keys: stats %s" % (K, s))
    assert s["served"] == 3 * T and s["batches"] < 3 * T
    for r in (0, 33, 127):
        assert coracle.verify_shuffle(CV, M, N_, g0["params"], keys[r % K], reqs[r]["deck"], out[r][0], out[r][1]) == 0


def test_cpp_driver_64_threads(mp, tmp_path):
    """tests/cpp/coalesce_threads.cpp against libmpshuffle.so: 64 std::threads, 4 x (prove + verify) each, coalesced; equal bytes"""
    from conftest import ROOT
    exe = tmp_path / "coalesce_threads"
    libdir = os.path.join(ROOT, "mental-poker_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coalesce_threads.cpp"), "-L", libdir, "-lmpshuffle", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "gpu", "64", "4"], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "coalesce ok" in out.stdout, out.stdout + out.stderr
