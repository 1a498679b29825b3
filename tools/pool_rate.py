#!/usr/bin/env python3
"""What the device pool (mp_pool_*, include/mpshuffle.h) delivers on ONE GPU: host-buffer calls of 1 024, 4 096, 16 384 and 65 536 proofs
through pools of 1, 2, 4 and 8 lanes on device 0 against the same calls on one plain mp_table in the same process.  STARK, 52 cards,
16-bit tables, page-locked buffers from mp_host_alloc; a call is mp_*_shuffle_and_remask_batch followed by mp_*_verify_shuffle_batch of
its outputs, timed with a host clock around calls that return complete.  Rates are proofs proved AND verified per second (bench.py's
count), separately for the prover's and the verifier's half as well.

For every (lanes, shape) the two variants are warmed up and then alternated: REPS repetitions of at least SECONDS each per variant; the
report gives the median and the spread (min .. max) of each, and the pool's rate over the plain table's -- median over median, with the
extreme ratios of the repetitions.  The pool of ONE lane against the plain table is the cost of the pool itself.

The measurement runs twice, each in a fresh child process: at the default number of hardware queues and with GPU_MAX_HW_QUEUES=16 set
for that child (a context owns four streams; INTEGRATION.md advises raising it for several contexts per GPU).  If more than one device is
visible, pools of one member per device [0 .. k-1] are measured too; otherwise the report says that no multi-GPU rate was measured.

usage: python tools/pool_rate.py [--reps R] [--seconds S] [--out profiles/pool_rates.txt]"""
import argparse
import ctypes
import importlib
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
CV, M, N_ = "stark", 2, 26
N = M * N_
SHAPES = (1024, 4096, 16384, 65536)
LANES = (1, 2, 4, 8)
DISTINCT = 1024          # distinct requests; larger shapes repeat them


class Pinned:
    """page-locked host buffers of one shape, in the layout of the batched entry points"""

    def __init__(self, lib, base, B, dsz, psz):
        self.lib, self.B = lib, B
        sizes = dict(decks=B * dsz, rho=B * N * 32, perm=B * N * 4, seeds=B * 32, out_decks=B * dsz, out_proofs=B * psz, status=B * 4)
        self.p = {}
        for k, n in sizes.items():
            ptr = lib.mp_host_alloc(n)
            if not ptr:
                raise MemoryError(lib.mp_last_error().decode())
            self.p[k] = ptr
        for k in ("decks", "rho", "perm", "seeds"):
            src = base[k]
            for o in range(0, sizes[k], len(src)):
                ctypes.memmove(self.p[k] + o, src, min(len(src), sizes[k] - o))

    def free(self):
        for ptr in self.p.values():
            self.lib.mp_host_free(ptr)

    def status_ok(self):
        st = (ctypes.c_int32 * self.B).from_address(self.p["status"])
        return not any(st)


def _base(co):
    g0 = co.gen_inputs(CV, M, N_, 9400)
    rnd = random.Random(9400)
    rho = bytearray(rnd.randbytes(DISTINCT * N * 32))
    for i in range(31, len(rho), 32):
        rho[i] &= 7
    perm = []
    for _ in range(DISTINCT):
        p = list(range(N))
        rnd.shuffle(p)
        perm += p
    return g0, dict(decks=g0["deck"] * DISTINCT, rho=bytes(rho), perm=bytes((ctypes.c_uint32 * len(perm))(*perm)),
                    seeds=rnd.randbytes(DISTINCT * 32))


def _call(lib, handle, pooled, buf):
    """one prove + verify of buf.B proofs; returns (prove seconds, verify seconds)"""
    p, B = buf.p, buf.B
    t0 = time.perf_counter()
    if pooled:
        rc = lib.mp_pool_shuffle_and_remask_batch(handle, B, None, p["decks"], p["rho"], p["perm"], p["seeds"], p["out_decks"], p["out_proofs"], p["status"])
    else:
        rc = lib.mp_shuffle_and_remask_batch(handle, B, p["decks"], p["rho"], p["perm"], p["seeds"], p["out_decks"], p["out_proofs"], p["status"])
    t1 = time.perf_counter()
    if rc != 0 or not buf.status_ok():
        raise RuntimeError("prove failed: %d %s" % (rc, lib.mp_last_error().decode()))
    if pooled:
        rc = lib.mp_pool_verify_shuffle_batch(handle, B, None, p["decks"], p["out_decks"], p["out_proofs"], p["status"])
    else:
        rc = lib.mp_verify_shuffle_batch(handle, B, p["decks"], p["out_decks"], p["out_proofs"], p["status"])
    t2 = time.perf_counter()
    if rc != 0 or not buf.status_ok():
        raise RuntimeError("verify failed: %d %s" % (rc, lib.mp_last_error().decode()))
    return t1 - t0, t2 - t1


def _rep(lib, handle, pooled, buf, seconds):
    """calls for at least `seconds` -> proofs/s of (prove + verify, prove alone, verify alone)"""
    tp = tv = 0.0
    n = 0
    while tp + tv < seconds:
        a, b = _call(lib, handle, pooled, buf)
        tp, tv, n = tp + a, tv + b, n + buf.B
    return n / (tp + tv), n / tp, n / tv


def _fmt(v):
    return "%8.0f (%8.0f .. %8.0f)" % (statistics.median(v), min(v), max(v))


def _measure(mp, lib, g0, bufs, devices, label, reps, seconds, out):
    eng = mp._native.Engine(CV, 0)
    t = eng.table(M, N_, g0["params"], g0["pk"], fb_bits=16)
    pool = mp.Pool(CV, devices)
    pt = pool.table(M, N_, g0["params"], g0["pk"], fb_bits=16)
    for B in SHAPES:
        buf = bufs[B]
        for handle, pooled in ((t.h, False), (pt.h, True)):      # warm-up: workspaces, staging, first-call costs
            _call(lib, handle, pooled, buf)
        plain, pooled_r = [], []
        for _ in range(reps):                                    # alternate the variants
            plain.append(_rep(lib, t.h, False, buf, seconds))
            pooled_r.append(_rep(lib, pt.h, True, buf, seconds))
        ratios = [b[0] / a[0] for a, b in zip(plain, pooled_r)]
        med = statistics.median(x[0] for x in pooled_r) / statistics.median(x[0] for x in plain)
        out("%-14s B=%6d  plain %s  pool %s  pool/plain %.3f (%.3f .. %.3f)" % (label, B, _fmt([x[0] for x in plain]), _fmt([x[0] for x in pooled_r]),
                                                                                med, min(ratios), max(ratios)))
        out("%-14s          prove: plain %s  pool %s | verify: plain %s  pool %s" % ("", _fmt([x[1] for x in plain]), _fmt([x[1] for x in pooled_r]),
                                                                                      _fmt([x[2] for x in plain]), _fmt([x[2] for x in pooled_r])))
    st = pt.stats()
    out("%-14s pool stats: %d calls, %d proofs, %d fixed-base build(s), members %s" % ("", st[0], st[1], st[3],
                                                                                         [pt.member_stats(i)["busy_us"] // 1000 for i in range(len(pool))]))
    pt.close()
    pool.close()
    t.close()
    eng.close()


def child(reps, seconds):
    import torch  # noqa: F401  (torch's HIP runtime first, as tests/conftest.py does)
    mp = importlib.import_module("mental-poker_amd")
    import coracle as co
    lib = mp.load()

    def out(line):
        print(line, flush=True)

    g0, base = _base(co)
    dsz, psz = len(g0["deck"]), lib.mp_proof_size(M, N_)
    ndev = torch.cuda.device_count()
    out("GPU_MAX_HW_QUEUES=%s, visible devices: %d" % (os.environ.get("GPU_MAX_HW_QUEUES", "(runtime default)"), ndev))
    out("columns: proofs proved and verified per second, median (min .. max) of %d repetitions of >= %.1f s per variant, alternated" % (reps, seconds))
    bufs = {B: Pinned(lib, base, B, dsz, psz) for B in SHAPES}
    for L in LANES:
        _measure(mp, lib, g0, bufs, [0] * L, "%d lane%s" % (L, "" if L == 1 else "s"), reps, seconds, out)
    if ndev > 1:
        for k in range(2, ndev + 1):
            _measure(mp, lib, g0, bufs, list(range(k)), "devices 0..%d" % (k - 1), reps, seconds, out)
    else:
        out("one device visible: no multi-GPU rate was measured")
    for b in bufs.values():
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and shape")
    ap.add_argument("--seconds", type=float, default=1.0, help="least duration of a repetition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_rates.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.reps, a.seconds)
        return
    import coracle as co
    co.build()
    lines = ["pool_rate: STARK m=%d n=%d (52 cards), 16-bit tables, page-locked host buffers; calls of %s proofs through pools of %s lanes on device 0"
             % (M, N_, ", ".join(str(b) for b in SHAPES), ", ".join(str(k) for k in LANES)),
             "and on one plain mp_table in the same process; host clock around mp_*_shuffle_and_remask_batch + mp_*_verify_shuffle_batch"]
    for queues in (None, "16"):
        env = dict(os.environ)
        if queues is not None:
            env["GPU_MAX_HW_QUEUES"] = queues        # for this fresh child only
        r = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--seconds", str(a.seconds)],
                             stdout=subprocess.PIPE, text=True, env=env)
        lines.append("")
        for line in r.stdout:
            lines.append(line.rstrip("\n"))
            print(lines[-1], flush=True)
        if r.wait() != 0:
            raise RuntimeError("child failed (%d)" % r.returncode)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
