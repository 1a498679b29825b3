#!/usr/bin/env python3
"""Dealing and seating in batches against the same work composed from the older entry points, on the STARK curve (host-buffer API, PCIe
included, one table): 1 024 tables of 52 cards under K = 1 024 aggregate keys, and 1 024 tables of 8 seats.
  (a) mp_verify_mask_batch(MP_DEAL_MASK)       against  mp_msm(n_msm = C, k = 2) for c1 - card + mp_sigma_verify_batch
  (b) mp_mask_batch(MP_DEAL_MASK)              against  the three mp_msm calls of DLCards.mask (r G | card + r pk | c1 - card) + mp_sigma_prove_batch
  (c) mp_verify_mask_batch(MP_DEAL_REMASK)     against  mp_msm(n_msm = 2 C, k = 2) for remasked - original + mp_sigma_verify_batch
  (d) mp_mask_batch(MP_DEAL_REMASK), every card under the table's own key (mp_remask_batch knows no other)
                                               against  mp_remask_batch + mp_msm(n_msm = 2 C, k = 2) + mp_sigma_prove_batch
  (e) mp_aggregate_keys_batch                  against  mp_sigma_verify_batch(nbases = 1) + mp_msm(n_msm = tables, k = P)
One warm-up and three timed repetitions each; only the library calls are timed (buffers are prepared before; the host's statement
assembly of the composed forms is reported on its own).  Bytes and status words of each pair are asserted equal.  No ratio is expected
in advance: every figure, whichever way it falls, goes to the output file (default profiles/deal_rates.txt)."""
import argparse
import ctypes
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--tables", type=int, default=1024)
ap.add_argument("--cards", type=int, default=52, help="cards per table")
ap.add_argument("--seats", type=int, default=8, help="players per table")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deal_rates.txt"))
args = ap.parse_args()

curve, m, n, PB = "stark", 2, 26, 64
K, P = args.tables, args.seats
C = K * args.cards
CB, PSZ, SSZ = 2 * PB, 2 * PB + 32, PB + 32
MASK, REMASK = 0, 1
eng = mp.Engine(curve, 0)
lib = eng.lib
params = eng.setup(m, n, bytes([1] * 32))
G = params[:PB]
q = mp.protocol.CURVE_ORDERS[curve]
rng = mp.ChaCha20Rng(bytes([9] * 32))
sc = lambda k: int(k).to_bytes(32, "little")      # noqa: E731
pt = lambda raw, i: raw[PB * i:PB * (i + 1)]       # noqa: E731

boot = eng.table(m, n, params, params[PB:2 * PB])
keys = boot.msm(K, 1, b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(K)), G * K)      # the tables' aggregate keys
deck = boot.msm(args.cards, 1, b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(args.cards)), G * args.cards)      # the open deck
boot.close()
t = eng.table(m, n, params, pt(keys, 0))      # (d) remasks under the table's own key: the first of the keys
h = t.h
key_index = [c // args.cards for c in range(C)]
factors = [mp.fr_rand(curve, rng) for _ in range(C)]
seeds = b"".join(bytes([c & 0xFF, (c >> 8) & 0xFF, c >> 16]) + bytes(29) for c in range(C))
plain = deck * K


def buf(raw):
    return (ctypes.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw if raw else b"\0")


def out(nbytes):
    return (ctypes.c_uint8 * nbytes)()


def words(count):
    return (ctypes.c_int32 * count)()


host = {"assemble": 0.0, "all": 0.0}      # seconds a composed form spends assembling statements from its own outputs (Python)


def timed(fn, reps=3):
    fn()                                   # warm-up
    ts = []
    for _ in range(reps):
        host["assemble"] = 0.0
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0 - host["assemble"])      # library calls only
        host["all"] += host["assemble"] / reps
    return ts


def chk(rc):
    if rc != 0:
        raise RuntimeError("call failed: %d %s" % (rc, lib.mp_last_error().decode()))


lines, ratios = [], []
assembly = 0.0                             # statements assembled once, ahead of the timed calls


def report(name, ts, items, unit):
    best = min(ts)
    lines.append("%-78s %s ms  (best %.2f ms = %.0f %s/s)" % (name, " ".join("%8.2f" % (v * 1e3) for v in ts), best * 1e3, items / best, unit))
    print(lines[-1], flush=True)
    return best


def pair(tag, new_name, new_ts, old_name, old_ts, items, unit):
    a, b = report("(%s) %s" % (tag, new_name), new_ts, items, unit), report("(%s) %s" % (tag, old_name), old_ts, items, unit)
    ratios.append("(%s) %.3f" % (tag, a / b))


one, minus = sc(1), sc(q - 1)
b_keys, b_ki, b_plain, b_seeds = buf(keys), (ctypes.c_uint32 * C)(*key_index), buf(plain), buf(seeds)
b_r = buf(b"".join(sc(r) for r in factors))
b_fs = {kind: buf(eng.blake2s(name) * C) for kind, name in ((MASK, b"Masking Proof"), (REMASK, b"Remasking Proof"))}
t0 = time.perf_counter()
g_host = b"".join(G + pt(keys, k) for k in key_index)
assembly += time.perf_counter() - t0
b_g = buf(g_host)

# ---- (b) masking
o_m, o_p, o_st = out(C * CB), out(C * PSZ), words(C)
tb = timed(lambda: chk(lib.mp_mask_batch(h, MASK, K, b_keys, C, b_ki, b_plain, b_r, b_seeds, o_m, o_p, o_st)))
assert not any(o_st)
masked, proofs = bytes(o_m), bytes(o_p)
b_G = buf(G * C)
b_sc2 = buf(b"".join(one + sc(r) for r in factors))
b_pt2 = buf(b"".join(pt(plain, c) + pt(keys, key_index[c]) for c in range(C)))
b_diff_sc = buf((one + minus) * C)
o_c0, o_c1, o_a1, o_p2, o_st2 = out(C * PB), out(C * PB), out(C * PB), out(C * PSZ), words(C)


def composed_mask():
    chk(lib.mp_msm(h, C, 1, b_r, b_G, o_c0))
    chk(lib.mp_msm(h, C, 2, b_sc2, b_pt2, o_c1))
    t0 = time.perf_counter()
    c0, c1 = bytes(o_c0), bytes(o_c1)
    d = buf(b"".join(pt(c1, c) + pt(plain, c) for c in range(C)))
    host["assemble"] += time.perf_counter() - t0
    chk(lib.mp_msm(h, C, 2, b_diff_sc, d, o_a1))
    t0 = time.perf_counter()
    a1 = bytes(o_a1)
    a = buf(b"".join(pt(c0, c) + pt(a1, c) for c in range(C)))
    host["assemble"] += time.perf_counter() - t0
    chk(lib.mp_sigma_prove_batch(h, C, 2, b_g, a, b_r, b_fs[MASK], b_seeds, o_p2, o_st2))


tb2 = timed(composed_mask)                 # (its statements depend on its own outputs: their assembly is taken out of the figure)
assert b"".join(pt(bytes(o_c0), c) + pt(bytes(o_c1), c) for c in range(C)) == masked and bytes(o_p2) == proofs and not any(o_st2), \
    "mp_mask_batch and its composed form differ"

# ---- (a) verification of the masking
b_m, b_p = buf(masked), buf(proofs)
o_v = words(C)
ta = timed(lambda: chk(lib.mp_verify_mask_batch(h, MASK, K, b_keys, C, b_ki, b_plain, b_m, b_p, o_v)))
assert not any(o_v)
t0 = time.perf_counter()
b_d1 = buf(b"".join(pt(masked, 2 * c + 1) + pt(plain, c) for c in range(C)))
assembly += time.perf_counter() - t0
o_sv = words(C)


def composed_verify_mask():
    chk(lib.mp_msm(h, C, 2, b_diff_sc, b_d1, o_a1))
    t0 = time.perf_counter()
    a1 = bytes(o_a1)
    a = buf(b"".join(pt(masked, 2 * c) + pt(a1, c) for c in range(C)))
    host["assemble"] += time.perf_counter() - t0
    chk(lib.mp_sigma_verify_batch(h, C, 2, b_g, a, b_p, b_fs[MASK], o_sv))


ta2 = timed(composed_verify_mask)
assert list(o_sv) == list(o_v), "mp_verify_mask_batch and its composed form differ"

# ---- (c) verification of a remasking under the K keys: the dealt cards remasked once more
alphas = b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(C))
b_al = buf(alphas)
o_rm, o_rp = out(C * CB), out(C * PSZ)
chk(lib.mp_mask_batch(h, REMASK, K, b_keys, C, b_ki, b_m, b_al, b_seeds, o_rm, o_rp, o_st))
assert not any(o_st)
remasked, rproofs = bytes(o_rm), bytes(o_rp)
b_rm, b_rp = buf(remasked), buf(rproofs)
tc = timed(lambda: chk(lib.mp_verify_mask_batch(h, REMASK, K, b_keys, C, b_ki, b_m, b_rm, b_rp, o_v)))
assert not any(o_v)
t0 = time.perf_counter()
b_d2 = buf(b"".join(pt(remasked, i) + pt(masked, i) for i in range(2 * C)))
assembly += time.perf_counter() - t0
b_diff_sc2 = buf((one + minus) * (2 * C))
o_a = out(2 * C * PB)


def composed_verify_remask():
    chk(lib.mp_msm(h, 2 * C, 2, b_diff_sc2, b_d2, o_a))
    chk(lib.mp_sigma_verify_batch(h, C, 2, b_g, o_a, b_rp, b_fs[REMASK], o_sv))


tc2 = timed(composed_verify_remask)
assert list(o_sv) == list(o_v), "mp_verify_mask_batch(MP_DEAL_REMASK) and its composed form differ"

# ---- (d) remasking under the table's own key
b_k1, b_ki0 = buf(pt(keys, 0)), (ctypes.c_uint32 * C)()
b_g1 = buf((G + pt(keys, 0)) * C)
td = timed(lambda: chk(lib.mp_mask_batch(h, REMASK, 1, b_k1, C, b_ki0, b_m, b_al, b_seeds, o_rm, o_rp, o_st)))
assert not any(o_st)
o_rm2 = out(C * CB)


def composed_remask():
    chk(lib.mp_remask_batch(h, C, b_m, b_al, o_rm2))
    t0 = time.perf_counter()
    rm = bytes(o_rm2)
    d = buf(b"".join(pt(rm, i) + pt(masked, i) for i in range(2 * C)))
    host["assemble"] += time.perf_counter() - t0
    chk(lib.mp_msm(h, 2 * C, 2, b_diff_sc2, d, o_a))
    chk(lib.mp_sigma_prove_batch(h, C, 2, b_g1, o_a, b_al, b_fs[REMASK], b_seeds, o_p2, o_st2))


td2 = timed(composed_remask)
assert bytes(o_rm2) == bytes(o_rm) and bytes(o_p2) == bytes(o_rp) and not any(o_st2), "mp_mask_batch(MP_DEAL_REMASK) and its composed form differ"

# ---- (e) seating
B = K * P
sks = [mp.fr_rand(curve, rng) for _ in range(B)]
pks = t.msm(B, 1, b"".join(sc(x) for x in sks), G * B)
fs_seat = b"".join(eng.blake2s(b"Key Ownership Proof" + b"table %d seat %d" % (l // P, l % P)) for l in range(B))
sproofs, sst = t.sigma_prove_batch(1, G * B, pks, b"".join(sc(x) for x in sks), fs_seat, seeds[:32 * B] if B <= C else os.urandom(32 * B))
assert not any(sst)
b_pk, b_sp, b_sfs, b_GB = buf(pks), buf(sproofs), buf(fs_seat), buf(G * B)
o_agg, o_ps, o_ts = out(K * PB), words(B), words(K)
te = timed(lambda: chk(lib.mp_aggregate_keys_batch(h, K, P, b_pk, b_sp, b_sfs, o_agg, o_ps, o_ts)))
assert not any(o_ps) and not any(o_ts)
b_ones = buf(one * B)
o_agg2, o_ssv = out(K * PB), words(B)


def composed_seating():
    chk(lib.mp_sigma_verify_batch(h, B, 1, b_GB, b_pk, b_sp, b_sfs, o_ssv))
    chk(lib.mp_msm(h, K, P, b_ones, b_pk, o_agg2))


te2 = timed(composed_seating)
assert bytes(o_agg2) == bytes(o_agg) and list(o_ssv) == list(o_ps), "mp_aggregate_keys_batch and its composed form differ"

lines.insert(0, "dealing and seating: %d tables x %d cards = %d lanes under K = %d keys, %d tables x %d seats = %d lanes, curve %s; warm-up + 3 "
                "repetitions, library calls only" % (K, args.cards, C, K, K, P, B, curve))
pair("a", "mp_verify_mask_batch(MASK)", ta, "mp_msm(k = 2) + mp_sigma_verify_batch", ta2, C, "cards")
pair("b", "mp_mask_batch(MASK)", tb, "mp_msm(k = 1) + 2 x mp_msm(k = 2) + mp_sigma_prove_batch", tb2, C, "cards")
pair("c", "mp_verify_mask_batch(REMASK)", tc, "mp_msm(n_msm = 2 C, k = 2) + mp_sigma_verify_batch", tc2, C, "cards")
pair("d", "mp_mask_batch(REMASK), the table's own key", td, "mp_remask_batch + mp_msm(n_msm = 2 C, k = 2) + mp_sigma_prove_batch", td2, C, "cards")
pair("e", "mp_aggregate_keys_batch", te, "mp_sigma_verify_batch(nbases = 1) + mp_msm(k = P)", te2, B, "players")
lines.append("host assembly of the composed forms' statements, not in their figures: %.0f ms for one pass through (a) .. (e) (Python)" % ((assembly + host["all"]) * 1e3))
lines.append("batched / composed: %s   outputs and status words of every pair identical" % "   ".join(ratios))
print("\n".join(lines[-2:]))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("deal_rate: done")
