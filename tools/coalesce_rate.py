#!/usr/bin/env python3
"""What request coalescing (mp_set_coalesce) buys a server whose callers make one proof per call, as the reference's trait does
[REF barnett-smart-card-protocol/src/lib.rs:181-197].  Rates are proofs proved AND verified per second (bench.py's count), STARK, 52 cards.

  1. T = 1, 16, 64, 256 Python threads, each looping shuffle_and_remask + verify_shuffle on ONE table with coalescing (T, 1 000 us),
     with the coalescing counters; the same with C++ threads (tests/cpp/coalesce_threads.cpp against libmpshuffle.so: no GIL);
  2. DLCards(coalesce=(256, 1000)) with a different aggregate key per thread (256 threads, one table of the parameters);
  3. for comparison, 4 and 8 host threads each with a context of its own and 1 024 proofs per mp_*_batch call -- run in a child process
     with GPU_MAX_HW_QUEUES=32 (a context owns four streams; INTEGRATION.md, multi-GPU), set for that child only.

usage: python tools/coalesce_rate.py [--rounds R] [--seconds S]     (prints the report; profiles/coalesce_rates.txt holds one)"""
import argparse
import importlib
import json
import os
import random
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
CV, M, N_ = "stark", 2, 26


def _pkg():
    import torch  # noqa: F401  (torch's HIP runtime first, as tests/conftest.py does)
    return importlib.import_module("mental-poker_amd")


def _requests(co, R, seed):
    g0 = co.gen_inputs(CV, M, N_, seed)
    rnd = random.Random(seed)
    N = M * N_
    reqs = []
    for _ in range(R):
        rho = bytearray(rnd.randbytes(32 * N))
        for i in range(31, len(rho), 32):
            rho[i] &= 7
        perm = list(range(N))
        rnd.shuffle(perm)
        reqs.append((g0["deck"], bytes(rho), perm, rnd.randbytes(32)))
    return g0, reqs


def _threads(T, fn):
    errors = []
    bar = threading.Barrier(T)

    def body(r):
        try:
            bar.wait()
            fn(r)
        except Exception as e:
            errors.append(repr(e))

    th = [threading.Thread(target=body, args=(r,)) for r in range(T)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errors:
        raise RuntimeError(errors[:3])
    return time.perf_counter() - t0


def python_sweep(mp, co, rounds, out):
    g0, reqs = _requests(co, 256, 9100)
    eng = mp._native.Engine(CV, 0)
    t = eng.table(M, N_, g0["params"], g0["pk"], fb_bits=16)
    d, p = t.shuffle_and_remask(*reqs[0])
    t.verify_shuffle(reqs[0][0], d, p)                         # (first-call costs out of the timings)
    for T in (1, 16, 64, 256):
        t.set_coalesce(T, 1000)

        def worker(r):
            q = reqs[r]
            for _ in range(rounds):
                d, p = t.shuffle_and_remask(*q)
                if t.verify_shuffle(q[0], d, p) != 0:
                    raise AssertionError("rejected")

        dt = _threads(T, worker)
        s = t.coalesce_stats()
        out("python threads T=%3d  %9.0f proofs/s   %s" % (T, T * rounds / dt, json.dumps(s)))
    t.close()
    eng.close()


def cpp_sweep(rounds, out):
    exe = os.path.join(ROOT, "tools", "_coalesce_threads")
    libdir = os.path.join(ROOT, "mental-poker_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coalesce_threads.cpp"), "-L", libdir, "-lmpshuffle", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    for T in (1, 16, 64, 256):
        r = subprocess.run([exe, "gpu", str(T), str(rounds)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0 or "coalesce ok" not in r.stdout:
            raise RuntimeError("C++ driver T=%d failed (%d): %s" % (T, r.returncode, (r.stdout + r.stderr)[-2000:]))
        j = json.loads(r.stdout.splitlines()[0])
        out("C++ threads    T=%3d  %9.0f proofs/s   %s" % (T, j["proofs_per_s"], json.dumps({k: j[k] for k in
            ("served", "batches", "largest", "closed_full", "closed_time", "rerun", "wait_us")})))


def dlcards_keys(mp, co, rounds, out):
    T = 256
    g0, reqs = _requests(co, T, 9200)
    cards = mp.DLCards(CV, device=0, coalesce=(256, 1000))
    raw = cards.engine.setup(2, T - 3, bytes(range(32)))
    keys = [raw[i * 64:(i + 1) * 64] for i in range(T)]
    pp = mp.Parameters(M, N_, g0["params"])
    args = []
    for deck, rho, perm, seed in reqs:
        args.append(([deck[i * 128:(i + 1) * 128] for i in range(M * N_)],
                     [int.from_bytes(rho[i * 32:(i + 1) * 32], "little") for i in range(M * N_)], mp.Permutation(perm), seed))
    sh, pf = cards.shuffle_and_remask(args[0][3], pp, keys[0], args[0][0], args[0][1], args[0][2])
    cards.verify_shuffle(pp, keys[0], args[0][0], sh, pf)
    cards.params_table(pp).set_coalesce(256, 1000)             # (counters from here)

    def worker(r):
        deck, rho, perm, seed = args[r]
        for _ in range(rounds):
            sh, pf = cards.shuffle_and_remask(seed, pp, keys[r], deck, rho, perm)
            cards.verify_shuffle(pp, keys[r], deck, sh, pf)

    dt = _threads(T, worker)
    out("DLCards, %d threads, %d distinct aggregate keys, one table of the parameters  %9.0f proofs/s   %s"
        % (T, T, T * rounds / dt, json.dumps(cards.params_table(pp).coalesce_stats())))


def contexts_child(K, B, seconds):
    """K host threads, a context each, B proofs per mp_*_batch call (prove then verify), for `seconds`"""
    mp = _pkg()
    import coracle as co
    g0, reqs = _requests(co, B, 9300)
    decks = b"".join(q[0] for q in reqs)
    rho = b"".join(q[1] for q in reqs)
    perms = sum((q[2] for q in reqs), [])
    seeds = b"".join(q[3] for q in reqs)
    done = [0] * K
    ready = threading.Barrier(K + 1)
    errors = []

    def worker(k):
        try:
            eng = mp._native.Engine(CV, 0)
            t = eng.table(M, N_, g0["params"], g0["pk"], fb_bits=16)
            d, p, st = t.shuffle_and_remask_batch(decks, rho, perms, seeds)
            assert not any(st) and not any(t.verify_shuffle_batch(decks, d, p))
            ready.wait()
            ready.wait()
            t_end = time.perf_counter() + seconds
            while time.perf_counter() < t_end:
                d, p, st = t.shuffle_and_remask_batch(decks, rho, perms, seeds)
                sv = t.verify_shuffle_batch(decks, d, p)
                assert not any(st) and not any(sv)
                done[k] += B
            t.close()
            eng.close()
        except Exception as e:
            errors.append(repr(e))
            ready.abort()

    th = [threading.Thread(target=worker, args=(k,)) for k in range(K)]
    for x in th:
        x.start()
    ready.wait()
    t0 = time.perf_counter()
    ready.wait()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    if errors:
        raise RuntimeError(errors[:3])
    print(json.dumps({"contexts": K, "proofs_per_call": B, "proofs": sum(done), "seconds": round(dt, 3), "proofs_per_s": round(sum(done) / dt, 1)}))


def contexts(seconds, out):
    for K in (4, 8):
        env = dict(os.environ, GPU_MAX_HW_QUEUES="32")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--contexts-child", str(K), "--seconds", str(seconds)],
                           capture_output=True, text=True, timeout=900, env=env)
        if r.returncode != 0:
            raise RuntimeError("contexts K=%d failed (%d): %s" % (K, r.returncode, (r.stdout + r.stderr)[-2000:]))
        j = json.loads(r.stdout.strip().splitlines()[-1])
        out("%d host threads, a context each, 1 024 proofs per _batch call  %9.0f proofs/s   %s" % (K, j["proofs_per_s"], json.dumps(j)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8, help="single-proof calls (prove + verify) per thread")
    ap.add_argument("--seconds", type=float, default=5.0, help="duration of each multi-context run")
    ap.add_argument("--contexts-child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.contexts_child:
        contexts_child(a.contexts_child, 1024, a.seconds)
        return

    def out(line):
        print(line, flush=True)

    mp = _pkg()
    import coracle as co
    co.build()
    out("coalesce_rate: STARK m=%d n=%d (52 cards), proofs proved and verified per second; %d rounds per thread" % (M, N_, a.rounds))
    python_sweep(mp, co, a.rounds, out)
    cpp_sweep(a.rounds, out)
    dlcards_keys(mp, co, a.rounds, out)
    contexts(a.seconds, out)


if __name__ == "__main__":
    main()
