#!/usr/bin/env python3
"""Opening cards in batches against the same work composed from the older entry points, C x T = 8 192 cards x 8 tokens on the STARK
curve (host-buffer API, PCIe included, one table):
  (a) mp_unmask_batch
  (b) one mp_sigma_verify_batch of the C T host-assembled statements + one mp_msm(n_msm = C, k = T + 1) with the scalars 1, -1, ..
  (c) mp_reveal_batch against mp_msm(n_msm = C T, k = 1) + mp_sigma_prove_batch
One warm-up and three timed repetitions each; only the library calls are timed (buffers are prepared before, the host's statement
assembly of (b) is reported on its own).  Every figure goes to the output file (default profiles/open_rates.txt)."""
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
ap.add_argument("--cards", type=int, default=8192)
ap.add_argument("--tokens", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_rates.txt"))
args = ap.parse_args()

curve, m, n, PB = "stark", 2, 26, 64
C, T = args.cards, args.tokens
B = C * T
PSZ = 2 * PB + 32
eng = mp.Engine(curve, 0)
lib = eng.lib
params = eng.setup(m, n, bytes([1] * 32))
G = params[:PB]
t = eng.table(m, n, params, params[PB:2 * PB])
h = t.h
q = mp.protocol.CURVE_ORDERS[curve]
rng = mp.ChaCha20Rng(bytes([7] * 32))
sc = lambda k: int(k).to_bytes(32, "little")      # noqa: E731

# tables of T players and 52 cards: card c sits at table c // 52, token j comes from that table's player j
tables = (C + 51) // 52
K = tables * T
sks = [mp.fr_rand(curve, rng) for _ in range(K)]
keys = t.msm(K, 1, b"".join(sc(k) for k in sks), G * K)
cards = t.msm(2 * C, 1, b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(2 * C)), G * (2 * C))
signer = [(c // 52) * T + j for c in range(C) for j in range(T)]
listed = [cards[2 * PB * c + PB:2 * PB * (c + 1)] for c in range(52)]      # 52 listed cards (they match nothing: the scan runs to its end)
seeds = b"".join(bytes([l & 0xFF, (l >> 8) & 0xFF, l >> 16]) + bytes(29) for l in range(B))


def buf(raw):
    return (ctypes.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw if raw else b"\0")


def out(nbytes):
    return (ctypes.c_uint8 * nbytes)()


def timed(fn, reps=3):
    fn()                                   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def chk(rc):
    if rc != 0:
        raise RuntimeError("call failed: %d %s" % (rc, lib.mp_last_error().decode()))


lines = []


def report(name, ts, items, unit):
    best = min(ts)
    lines.append("%-58s %s ms  (best %.2f ms = %.0f %s/s)" % (name, " ".join("%8.2f" % (v * 1e3) for v in ts), best * 1e3, items / best, unit))
    print(lines[-1], flush=True)
    return best


b_keys, b_sks, b_cards, b_seeds = buf(keys), buf(b"".join(sc(k) for k in sks)), buf(cards), buf(seeds)
b_signer = (ctypes.c_uint32 * B)(*signer)
o_tok, o_prf, o_st = out(B * PB), out(B * PSZ), (ctypes.c_int32 * B)()

# ---- (c) reveal
tc = timed(lambda: chk(lib.mp_reveal_batch(h, K, b_keys, b_sks, C, b_cards, T, b_signer, b_seeds, o_tok, o_prf, o_st)))
assert not any(o_st)
tokens, proofs = bytes(o_tok), bytes(o_prf)
t0 = time.perf_counter()
g_host = b"".join(cards[2 * PB * (l // T):2 * PB * (l // T) + PB] + G for l in range(B))
a_host = b"".join(tokens[PB * l:PB * (l + 1)] + keys[PB * signer[l]:PB * (signer[l] + 1)] for l in range(B))
fs_host = eng.blake2s(b"Reveal Proof") * B
t_assemble = time.perf_counter() - t0
x_host = b"".join(sc(sks[g]) for g in signer)
c0_host = b"".join(cards[2 * PB * (l // T):2 * PB * (l // T) + PB] for l in range(B))
b_g, b_a, b_fs, b_x, b_c0 = buf(g_host), buf(a_host), buf(fs_host), buf(x_host), buf(c0_host)
o_tok2, o_prf2, o_st2 = out(B * PB), out(B * PSZ), (ctypes.c_int32 * B)()


def composed_reveal():
    chk(lib.mp_msm(h, B, 1, b_x, b_c0, o_tok2))
    # (the publics of the sigma call hold the tokens just computed: assembled before, as they are the same bytes every time)
    chk(lib.mp_sigma_prove_batch(h, B, 2, b_g, b_a, b_x, b_fs, b_seeds, o_prf2, o_st2))


tc2 = timed(composed_reveal)
assert bytes(o_tok2) == tokens and bytes(o_prf2) == proofs and not any(o_st2), "mp_reveal_batch and its composed form differ"

# ---- (a) unmask
b_tok, b_prf, b_list = buf(tokens), buf(proofs), buf(b"".join(listed))
o_plain, o_idx, o_ts, o_cs = out(C * PB), (ctypes.c_uint32 * C)(), (ctypes.c_int32 * B)(), (ctypes.c_int32 * C)()
ta = timed(lambda: chk(lib.mp_unmask_batch(h, K, b_keys, C, b_cards, T, b_signer, b_tok, b_prf, len(listed), b_list, o_plain, o_idx, o_ts, o_cs)))
assert not any(o_ts) and not any(o_cs)

# ---- (b) the same from mp_sigma_verify_batch + mp_msm
one, minus = sc(1), sc(q - 1)
b_msc = buf((one + minus * T) * C)
b_mpt = buf(b"".join(cards[2 * PB * c + PB:2 * PB * (c + 1)] + tokens[PB * T * c:PB * T * (c + 1)] for c in range(C)))
o_plain2, o_sv = out(C * PB), (ctypes.c_int32 * B)()


def composed_unmask():
    chk(lib.mp_sigma_verify_batch(h, B, 2, b_g, b_a, b_prf, b_fs, o_sv))
    chk(lib.mp_msm(h, C, T + 1, b_msc, b_mpt, o_plain2))


tb = timed(composed_unmask)
assert not any(o_sv) and bytes(o_plain2) == bytes(o_plain), "mp_unmask_batch and its composed form differ"

lines.insert(0, "opening cards: C = %d cards x T = %d tokens = %d lanes, K = %d keys, %d listed cards, curve %s; warm-up + 3 repetitions, library calls only"
             % (C, T, B, K, len(listed), curve))
a = report("(a) mp_unmask_batch", ta, B, "tokens")
b = report("(b) mp_sigma_verify_batch + mp_msm(n_msm = C, k = T + 1)", tb, B, "tokens")
c1 = report("(c) mp_reveal_batch", tc, B, "tokens")
c2 = report("(c) mp_msm(k = 1) + mp_sigma_prove_batch", tc2, B, "tokens")
lines.append("host assembly of the %d statements of (b), not in its figure: %.0f ms (Python)" % (B, t_assemble * 1e3))
lines.append("(a) / (b) = %.3f   reveal / composed = %.3f   outputs of both pairs byte-identical" % (a / b, c1 / c2))
print("\n".join(lines[-2:]))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
ok = a <= b and c1 <= c2
print("open_rate: %s" % ("ok" if ok else "the batched call is SLOWER than its composed form"))
sys.exit(0 if ok else 1)
