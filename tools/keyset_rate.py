#!/usr/bin/env python3
"""Key sets whose slots change, on the STARK curve, one MI355X (device buffers are torch tensors; only the library calls are timed):
  (a) mp_keyset_update_dev of 1, 64 and 1 024 slots of a 4 096-slot set (+ mp_sync)
                                               against  mp_keyset_create of all 4 096 keys, the only way to change a key before
  (b) mp_mask_batch_keyset and mp_verify_mask_batch_keyset (MP_DEAL_MASK, host buffers, PCIe included)
                                               against  mp_mask_batch and mp_verify_mask_batch with the keys passed
      1 024 tables of 52 cards, a key per table (the shape of profiles/deal_rates.txt)
  (c) mp_verify_shuffle_chain_ragged_keyset_dev, one index per table
                                               against  mp_verify_shuffle_chain_ragged_dev with the table's key copied once per link
      1 024 tables of 52 cards, 2 .. 10 links each, drawn evenly (the chain shape of profiles/ragged_rates.txt); the chains are made by
      the seeded prover by index, link by link
One warm-up, then --reps alternating repetitions of each leg (taking turns in going first); median, min and max are written.  Status words
of each pair are asserted equal.  No ratio is expected in advance: every figure goes to the output file (default
profiles/keyset_rates.txt).  The create leg of (a) is mp_keyset_create + mp_keyset_destroy: it allocates and frees the whole set's tables."""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=4096)
ap.add_argument("--tables", type=int, default=1024)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyset_rates.txt"))
args = ap.parse_args()

curve, m, n, PB = "stark", 2, 26, 64
N = m * n
dev = "cuda:0"
eng = mp.Engine(curve, 0)
params = eng.setup(m, n, bytes([1] * 32))
G = params[:PB]
rng = mp.ChaCha20Rng(bytes([9] * 32))
sc = lambda k: int(k).to_bytes(32, "little")      # noqa: E731
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def gpu(raw, dtype=torch.uint8):
    return torch.frombuffer(bytearray(raw), dtype=dtype).to(dev)


def points(_, count):
    return boot.msm(count, 1, b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(count)), G * count)


def alternate(name_a, fa, name_b, fb, unit, count_a, count_b):
    fa(), fb()
    ta, tb = [], []
    for r in range(args.reps):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            t0 = time.perf_counter()
            (fa, fb)[which]()
            (ta, tb)[which].append((time.perf_counter() - t0) * 1e3)
    for name, ts, cnt in ((name_a, ta, count_a), (name_b, tb, count_b)):
        med = statistics.median(ts)
        say("%-58s median %9.2f ms  (min %9.2f, max %9.2f; %d %s/s)" % (name, med, min(ts), max(ts), cnt / med * 1e3, unit))
    ratio = statistics.median(ta) / statistics.median(tb)
    say("      ratio %.4f" % ratio)
    return ratio


boot = eng.table(m, n, params, params[PB:2 * PB])      # mp_msm wants a table with a key of its own
t = eng.table(m, n, params, None)
say("key sets: curve %s, one table (m = %d, n = %d); one warm-up, then %d alternating repetitions of each leg (taking turns in going "
    "first), library calls only, device buffers" % (curve, m, n, args.reps))

# ---- (a) the cost of changing keys
K = args.slots
keys = points(t, K)
fresh = points(t, 1024)
ks = t.keyset(keys)
d_fresh, d_st = gpu(fresh), torch.zeros(1024, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
say("(a) a set of %d slots (%.1f GB of tables); slots changed per call, spread over the set" % (K, K * 32 * 255 * PB / 1e9))


def create_all():
    other = t.keyset(keys)
    other.close()


for count in (1, 64, 1024):
    slots = [(i * (K // count)) % K for i in range(count)]

    def update():
        ks.update_dev(slots, d_fresh.data_ptr(), d_st.data_ptr())
        eng.sync()
    alternate("(a)%-5d mp_keyset_update_dev of %d slots + mp_sync" % (count, count), update,
              "(a)%-5d mp_keyset_create of all %d keys (+ destroy)" % (count, K), create_all, "keys", count, K)
    assert not d_st[:count].any().item()
assert ks.live() == K
ks.close()

# ---- (c) chains by index against chains with copied keys
T = args.tables
links = [2 + (k * 9) // T for k in range(T)]
total = sum(links)
tkeys = points(t, T)
ks = t.keyset(tkeys)
DSZ, PSZ = 2 * N * PB, t.proof_bytes
start = points(t, 2 * N)
off = [0]
for L in links:
    off.append(off[-1] + L)
decks = torch.zeros((total + T) * DSZ, dtype=torch.uint8, device=dev)
proofs = torch.zeros(total * PSZ, dtype=torch.uint8, device=dev)
dk = decks.view(total + T, DSZ)
pf = proofs.view(total, PSZ)
dk[[off[k] + k for k in range(T)]] = gpu(start)
for j in range(max(links)):
    rows = [k for k in range(T) if links[k] > j]
    B = len(rows)
    src = dk[[off[k] + k + j for k in rows]].contiguous()
    d_idx = torch.tensor(rows, dtype=torch.int32, device=dev)
    d_seeds = gpu(b"".join(bytes([7, j, k & 0xFF, k >> 8]) + bytes(28) for k in rows))
    od, op = torch.zeros(B * DSZ, dtype=torch.uint8, device=dev), torch.zeros(B * PSZ, dtype=torch.uint8, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t.shuffle_and_remask_batch_seeded_keyset_dev(ks, B, d_idx.data_ptr(), src.data_ptr(), d_seeds.data_ptr(), od.data_ptr(), op.data_ptr(),
                                                 st.data_ptr())
    eng.sync()
    assert not st.any().item()
    dk[[off[k] + k + j + 1 for k in rows]] = od.view(B, DSZ)
    pf[[off[k] + j for k in rows]] = op.view(B, PSZ)
per_link = gpu(b"".join(tkeys[PB * k:PB * (k + 1)] * links[k] for k in range(T)))
d_idx = torch.arange(T, dtype=torch.int32, device=dev)
st_i, st_k = torch.full((total,), 7, dtype=torch.int32, device=dev), torch.full((total,), 7, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
say("(c) chains: %d tables of %d cards, %d links" % (T, N, total))


def by_index():
    t.verify_shuffle_chain_ragged_keyset_dev(ks, links, d_idx.data_ptr(), decks.data_ptr(), proofs.data_ptr(), st_i.data_ptr())
    eng.sync()


def by_keys():
    t.verify_shuffle_chain_ragged_dev(links, per_link.data_ptr(), decks.data_ptr(), proofs.data_ptr(), st_k.data_ptr())
    eng.sync()


alternate("(c)      mp_verify_shuffle_chain_ragged_keyset_dev", by_index, "(c)      mp_verify_shuffle_chain_ragged_dev, keys copied per link", by_keys,
          "links", total, total)
assert not st_i.any().item() and torch.equal(st_i, st_k)

# ---- (b) dealing by index against dealing with the keys passed
CARDS = 52
C = T * CARDS
deck = points(t, CARDS)
plain = deck * T
key_index = [c // CARDS for c in range(C)]
factors = b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(C))
seeds = b"".join(bytes([c & 0xFF, (c >> 8) & 0xFF, c >> 16]) + bytes(29) for c in range(C))
say("(b) dealing: %d tables of %d cards, %d keys" % (T, CARDS, T))
res = {}


def mask_index():
    res["mi"] = t.mask_batch_keyset(ks, 0, key_index, plain, factors, seeds)


def mask_keys():
    res["mk"] = t.mask_batch(0, tkeys, key_index, plain, factors, seeds)


alternate("(b)m     mp_mask_batch_keyset", mask_index, "(b)m     mp_mask_batch", mask_keys, "cards", C, C)
assert res["mi"] == res["mk"] and not any(res["mi"][2])
masked, prfs = res["mi"][0], res["mi"][1]


def verify_index():
    res["vi"] = t.verify_mask_batch_keyset(ks, 0, key_index, plain, masked, prfs)


def verify_keys():
    res["vk"] = t.verify_mask_batch(0, tkeys, key_index, plain, masked, prfs)


alternate("(b)v     mp_verify_mask_batch_keyset", verify_index, "(b)v     mp_verify_mask_batch", verify_keys, "cards", C, C)
assert res["vi"] == res["vk"] and not any(res["vi"])
ks.close()
t.close()
boot.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
