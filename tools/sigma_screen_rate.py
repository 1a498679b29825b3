#!/usr/bin/env python3
"""The sigma verifiers with and without the screening pass (mp_set_sigma_screen), on ONE table, alternating off and on: the shapes of
profiles/open_rates.txt (8 192 cards x 8 tokens through mp_unmask_batch) and profiles/deal_rates.txt (1 024 tables x 52 cards through
mp_verify_mask_batch, MASK and REMASK; 1 024 tables x 8 seats through mp_aggregate_keys_batch), each once honest and once with one lane
in 1 000 tampered (response + 1).  Host-buffer API, PCIe included: every timed call ends in a synchronise.  A warm-up of each setting,
then `--reps` repetitions of off, on, off, on ...; per shape the times, their spread ((max - min) / median), off-time over on-time, what
the screened calls added to mp_sigma_screen_stats, and whether outputs and status words are identical.  Everything goes to the output
file (default profiles/sigma_screen_rates.txt).  --scale divides the batch sizes (a slower curve, a quick look)."""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--curve", default="stark")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--scale", type=int, default=1)
ap.add_argument("--lanes", type=lambda v: int(v, 0), default=0xFFFFFFFF, help="lanes per group (default: MP_SIGMA_SCREEN_AUTO)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_screen_rates.txt"))
args = ap.parse_args()
if args.reps < 5:
    ap.error("at least 5 repetitions")

curve, m, n = args.curve, 2, 26
eng = mp.Engine(curve, 0)
lib, PB = eng.lib, eng.point_bytes
params = eng.setup(m, n, bytes([1] * 32))
G = params[:PB]
t = eng.table(m, n, params, params[PB:2 * PB])
h = t.h
q = mp.protocol.CURVE_ORDERS[curve]
rng = mp.ChaCha20Rng(bytes([9] * 32))
sc = lambda k: int(k).to_bytes(32, "little")      # noqa: E731
rand_scalars = lambda k: b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(k))      # noqa: E731
seeds_of = lambda k: b"".join(bytes([l & 0xFF, (l >> 8) & 0xFF, l >> 16]) + bytes(29) for l in range(k))      # noqa: E731


def buf(raw):
    return (ctypes.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw if raw else b"\0")


def chk(rc):
    if rc != 0:
        raise RuntimeError("call failed: %d %s" % (rc, lib.mp_last_error().decode()))


def tamper(proofs, psz, lanes):
    """response + 1 in lane 500, 1 500, ...: one lane in 1 000"""
    p = bytearray(proofs)
    bad = list(range(500, lanes, 1000))
    for l in bad:
        z = (int.from_bytes(p[(l + 1) * psz - 32:(l + 1) * psz], "little") + 1) % q
        p[(l + 1) * psz - 32:(l + 1) * psz] = sc(z)
    return bytes(p), bad


lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def measure(name, lanes, unit, call, outputs, want_bad, fail_code):
    """call() fills `outputs` (ctypes arrays; the first one holds the lanes' status words)"""
    snap = lambda: [bytes(o) for o in outputs]      # noqa: E731
    res, times = {}, {False: [], True: []}
    for on in (False, True):                         # warm-up of both settings, and the outputs to compare
        t.set_sigma_screen(args.lanes if on else 0, 1)
        call()
        res[on] = snap()
    stats = [0, 0, 0, 0]
    for _ in range(args.reps):
        for on in (False, True):
            t.set_sigma_screen(args.lanes if on else 0, 1)
            t0 = time.perf_counter()
            call()
            times[on].append(time.perf_counter() - t0)
            if on:
                stats = t.sigma_screen_stats()
            elif t.sigma_screen_stats() != [0, 0, 0, 0]:
                raise RuntimeError("the switch is off and the counters moved")
    t.set_sigma_screen(0, 1)
    words = list(outputs[0])
    same = res[False] == res[True] and snap() == res[False]
    if [l for l, v in enumerate(words) if v] != want_bad or any(words[l] != fail_code for l in want_bad):
        raise RuntimeError("%s: status words %s" % (name, [(l, v) for l, v in enumerate(words) if v][:8]))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    ratio = med[False] / med[True]
    noise = max(spread.values())
    verdict = "faster" if ratio > 1 + noise else ("SLOWER" if ratio < 1 - noise else "no difference beyond the spread")
    say("%s: %d lanes%s" % (name, lanes, ", %d tampered" % len(want_bad) if want_bad else ""))
    for on in (False, True):
        say("  screen %-3s %s ms  median %8.2f ms = %9.0f %s/s  spread %4.1f %%" %
            ("on" if on else "off", " ".join("%8.2f" % (v * 1e3) for v in times[on]), med[on] * 1e3, lanes / med[on], unit, spread[on] * 100))
    say("  off / on = %.3f (%s)   stats of one screened call: lanes %d, equations %d, failing groups %d, lanes re-verified %d   outputs and status words %s"
        % (ratio, verdict, stats[0], stats[1], stats[2], stats[3], "identical" if same else "DIFFER"))
    return same


ok = True
S = args.scale
# ---- opening: C cards x T tokens, tables of T players and 52 cards
C, T = 8192 // S, 8
B = C * T
PSZ = 2 * PB + 32
K = ((C + 51) // 52) * T
sks = [mp.fr_rand(curve, rng) for _ in range(K)]
keys = t.msm(K, 1, b"".join(sc(k) for k in sks), G * K)
cards = t.msm(2 * C, 1, rand_scalars(2 * C), G * (2 * C))
signer = [(c // 52) * T + j for c in range(C) for j in range(T)]
listed = b"".join(cards[2 * PB * c + PB:2 * PB * (c + 1)] for c in range(52))
tokens, proofs, st = t.reveal_batch(keys, b"".join(sc(k) for k in sks), cards, T, signer, seeds_of(B))
assert not any(st)
b_keys, b_cards, b_tok, b_list = buf(keys), buf(cards), buf(tokens), buf(listed)
b_signer = (ctypes.c_uint32 * B)(*signer)
o_plain, o_idx, o_ts, o_cs = (ctypes.c_uint8 * (C * PB))(), (ctypes.c_uint32 * C)(), (ctypes.c_int32 * B)(), (ctypes.c_int32 * C)()
say("sigma screening, curve %s, lanes per group %s, %d repetitions alternating off / on after a warm-up of each; host-buffer calls, PCIe included"
    % (curve, "AUTO" if args.lanes == 0xFFFFFFFF else args.lanes, args.reps))
for pf, bad in ((proofs, []), tamper(proofs, PSZ, B)):
    b_prf = buf(pf)
    ok &= measure("mp_unmask_batch %d cards x %d tokens" % (C, T), B, "tokens",
                  lambda: chk(lib.mp_unmask_batch(h, K, b_keys, C, b_cards, T, b_signer, b_tok, b_prf, 52, b_list, o_plain, o_idx, o_ts, o_cs)),
                  [o_ts, o_cs, o_plain, o_idx], bad, 6)

# ---- dealing: `tables` tables x 52 cards, one aggregate key per table
tables = 1024 // S
Cd = tables * 52
dkeys = t.msm(tables, 1, rand_scalars(tables), G * tables)
kidx = [c // 52 for c in range(Cd)]
plain = t.msm(Cd, 1, rand_scalars(Cd), G * Cd)
b_dkeys, b_kidx = buf(dkeys), (ctypes.c_uint32 * Cd)(*kidx)
o_st = (ctypes.c_int32 * Cd)()
inputs = plain
for kind, kname in ((t.DEAL_MASK, "MASK"), (t.DEAL_REMASK, "REMASK")):
    masked, dproofs, st = t.mask_batch(kind, dkeys, kidx, inputs, rand_scalars(Cd), seeds_of(Cd))
    assert not any(st)
    b_in, b_masked = buf(inputs), buf(masked)
    for pf, bad in ((dproofs, []), tamper(dproofs, PSZ, Cd)):
        b_prf = buf(pf)
        ok &= measure("mp_verify_mask_batch %s %d tables x 52 cards" % (kname, tables), Cd, "cards",
                      lambda: chk(lib.mp_verify_mask_batch(h, kind, tables, b_dkeys, Cd, b_kidx, b_in, b_masked, b_prf, o_st)), [o_st], bad, 6)
    inputs = masked      # the remasked cards are the masked ones

# ---- seating: `tables` tables x 8 seats
P = 8
Bs = tables * P
ssk = rand_scalars(Bs)
skeys = t.msm(Bs, 1, ssk, G * Bs)
fs = b"".join(eng.blake2s(b"Key Ownership Proof" + b"player %d" % l) for l in range(Bs))
sproofs, st = t.sigma_prove_batch(1, G * Bs, skeys, ssk, fs, seeds_of(Bs))
assert not any(st)
b_skeys, b_fs = buf(skeys), buf(fs)
o_agg, o_ps, o_tst = (ctypes.c_uint8 * (tables * PB))(), (ctypes.c_int32 * Bs)(), (ctypes.c_int32 * tables)()
for pf, bad in ((sproofs, []), tamper(sproofs, PB + 32, Bs)):
    b_prf = buf(pf)
    ok &= measure("mp_aggregate_keys_batch %d tables x %d seats" % (tables, P), Bs, "seats",
                  lambda: chk(lib.mp_aggregate_keys_batch(h, tables, P, b_skeys, b_prf, b_fs, o_agg, o_ps, o_tst)), [o_ps, o_tst, o_agg], bad, 5)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("sigma_screen_rate: %s" % ("ok" if ok else "outputs or status words DIFFER between the two settings"))
sys.exit(0 if ok else 1)
