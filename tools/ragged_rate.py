#!/usr/bin/env python3
"""The ragged calls -- cards, tables and chains of different sizes in one call -- against the same work done the way a caller had to do it
before: one uniform call per distinct count, on the same table.  STARK curve, host-buffer API, PCIe included, one table; seat counts
drawn evenly from 2..10:
  opening   about 8 192 cards (the tables of 52 cards of profiles/open_rates.txt; a card takes one token per seat of its table)
            mp_unmask_ragged_batch / mp_reveal_ragged_batch          against  9 x mp_unmask_batch / mp_reveal_batch
  seating   about 1 024 tables      mp_aggregate_keys_ragged_batch   against  9 x mp_aggregate_keys_batch
  chains    about 1 024 tables of 52 cards, one link per seat
                                    mp_verify_shuffle_chain_ragged   against  9 x mp_verify_shuffle_chain, in both decompositions
                                    (mp_set_chain_pieces: w whole, b binary), and on device-resident inputs
                                    mp_verify_shuffle_chain_ragged_dev  against  9 x mp_verify_shuffle_chain_dev (tags d)
(a) mixed counts: the ragged call against the nine uniform calls.  (b) every count equal (6): the ragged call against the one uniform
call -- the cost of the offsets path alone.  The buffers of both legs are prepared before; only the library calls are timed, each of
which ends in a stream synchronise.  After one warm-up of both legs the legs alternate (and take turns in going first), `--reps`
repetitions each; the medians and their ratio are reported, and the outputs of the two legs are asserted equal item by item.  No ratio is expected in advance: every figure,
whichever way it falls, goes to the output file (default profiles/ragged_rates.txt)."""
import argparse
import ctypes
import importlib
import os
import random
import statistics
import sys
import time

import torch  # noqa: F401  (before the library: torch ships a HIP runtime of its own, and the device leg of the chains keeps its buffers in it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mp = importlib.import_module("mental-poker_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--cards", type=int, default=8192)
ap.add_argument("--tables", type=int, default=1024, help="tables of the seating call")
ap.add_argument("--chain-tables", type=int, default=1024)
ap.add_argument("--deck", type=int, default=26, help="n of the deck (m = 2): 26 = 52 cards")
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_rates.txt"))
args = ap.parse_args()

curve, m, n, PB = "stark", 2, args.deck, 64
N = m * n
CB, PSZ, SSZ = 2 * PB, 2 * PB + 32, PB + 32
EQUAL = 6
eng = mp.Engine(curve, 0)
lib = eng.lib
params = eng.setup(m, n, bytes([1] * 32))
G = params[:PB]
t = eng.table(m, n, params, params[PB:2 * PB])
h = t.h
rng = mp.ChaCha20Rng(bytes([11] * 32))
sc = lambda k: int(k).to_bytes(32, "little")      # noqa: E731
seed32 = lambda tag, i: bytes([tag, i & 0xFF, (i >> 8) & 0xFF, (i >> 16) & 0xFF]) + bytes(28)      # noqa: E731


def drawn(count, salt):
    """`count` seat counts, 2..10 evenly, in a fixed random order"""
    v = [2 + i % 9 for i in range(count)]
    random.Random(salt).shuffle(v)
    return v


def buf(raw):
    return (ctypes.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw if raw else b"\0")


def out(nbytes):
    return (ctypes.c_uint8 * max(nbytes, 1))()


def words(count, kind=ctypes.c_int32):
    return (kind * max(count, 1))()


def u32(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


def chk(rc):
    if rc != 0:
        raise RuntimeError("call failed: %d %s" % (rc, lib.mp_last_error().decode()))


def offsets(counts):
    first = [0]
    for c in counts:
        first.append(first[-1] + c)
    return first


def by_count(counts):
    groups = {}
    for i, c in enumerate(counts):
        groups.setdefault(c, []).append(i)
    return sorted(groups.items())


def pick(raw, size, idx):
    return b"".join(raw[size * i:size * (i + 1)] for i in idx)


lines, ratios = [], []


def pair(tag, name_a, leg_a, name_b, leg_b, items, unit):
    """one warm-up of both legs, then the legs alternate, and so does the one that goes first; medians"""
    leg_a()
    leg_b()
    ta, tb = [], []
    for rep in range(args.reps):
        for leg, ts in ((leg_a, ta), (leg_b, tb)) if rep % 2 == 0 else ((leg_b, tb), (leg_a, ta)):      # whoever went second goes first next
            t0 = time.perf_counter()
            leg()
            ts.append(time.perf_counter() - t0)
    ma, mb = statistics.median(ta), statistics.median(tb)
    for name, ts, med in ((name_a, ta, ma), (name_b, tb, mb)):
        lines.append("%-5s %-46s median %8.2f ms  (min %8.2f, max %8.2f; %.0f %s/s)" % (tag, name, med * 1e3, min(ts) * 1e3, max(ts) * 1e3, items / med, unit))
        print(lines[-1], flush=True)
    lines.append("%-5s ratio %.3f" % (tag, ma / mb))
    print(lines[-1], flush=True)
    ratios.append("%s %.3f" % (tag, ma / mb))


# ---------------------------------------------------------------------------------------------------------------- opening
def opening(tag, seats):
    """cards of tables of 52: card c sits at table c // 52 and takes one token from every seat of that table"""
    C = args.cards
    base = offsets(seats)
    K = base[-1]
    counts = [seats[c // 52] for c in range(C)]
    first = offsets(counts)
    B = first[-1]
    signer = [base[c // 52] + j for c in range(C) for j in range(counts[c])]
    sks = b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(K))
    keys = t.msm(K, 1, sks, G * K)
    cards = t.msm(2 * C, 1, b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(2 * C)), G * (2 * C))
    listed = pick(cards, PB, [2 * c + 1 for c in range(52)])      # 52 listed cards (they match nothing: the scan runs to its end)
    seeds = b"".join(seed32(1, l) for l in range(B))
    b_keys, b_sks, b_cards, b_seeds, b_first, b_signer, b_list = buf(keys), buf(sks), buf(cards), buf(seeds), u32(first), u32(signer), buf(listed)
    o_tok, o_prf, o_st = out(B * PB), out(B * PSZ), words(B)
    groups = []
    for T, items in by_count(counts):
        lanes = [l for c in items for l in range(first[c], first[c + 1])]
        groups.append(dict(T=T, items=items, lanes=lanes, cards=buf(pick(cards, CB, items)), signer=u32([signer[l] for l in lanes]),
                           seeds=buf(pick(seeds, 32, lanes)), tok=out(len(lanes) * PB), prf=out(len(lanes) * PSZ), st=words(len(lanes)),
                           plain=out(len(items) * PB), idx=words(len(items), ctypes.c_uint32), ts=words(len(lanes)), cs=words(len(items))))

    def reveal_ragged():
        chk(lib.mp_reveal_ragged_batch(h, K, b_keys, b_sks, C, b_cards, b_first, b_signer, b_seeds, o_tok, o_prf, o_st))

    def reveal_uniform():
        for g in groups:
            chk(lib.mp_reveal_batch(h, K, b_keys, b_sks, len(g["items"]), g["cards"], g["T"], g["signer"], g["seeds"], g["tok"], g["prf"], g["st"]))
    what = "%d cards, %d tokens, %d uniform call%s" % (C, B, len(groups), "s" if len(groups) > 1 else "")
    lines.append("%s opening: %s" % (tag, what))
    pair(tag + "r", "mp_reveal_ragged_batch", reveal_ragged, "%d x mp_reveal_batch" % len(groups), reveal_uniform, B, "tokens")
    tokens, proofs = bytes(o_tok), bytes(o_prf)
    assert not any(o_st)
    for g in groups:
        assert bytes(g["tok"]) == pick(tokens, PB, g["lanes"]) and bytes(g["prf"]) == pick(proofs, PSZ, g["lanes"]) and not any(g["st"]), \
            "mp_reveal_ragged_batch and mp_reveal_batch differ"
        g["tokens"], g["proofs"] = buf(bytes(g["tok"])), buf(bytes(g["prf"]))
    b_tok, b_prf = buf(tokens), buf(proofs)
    o_plain, o_idx, o_ts, o_cs = out(C * PB), words(C, ctypes.c_uint32), words(B), words(C)

    def unmask_ragged():
        chk(lib.mp_unmask_ragged_batch(h, K, b_keys, C, b_cards, b_first, b_signer, b_tok, b_prf, 52, b_list, o_plain, o_idx, o_ts, o_cs))

    def unmask_uniform():
        for g in groups:
            chk(lib.mp_unmask_batch(h, K, b_keys, len(g["items"]), g["cards"], g["T"], g["signer"], g["tokens"], g["proofs"], 52, b_list, g["plain"],
                                    g["idx"], g["ts"], g["cs"]))
    pair(tag + "u", "mp_unmask_ragged_batch", unmask_ragged, "%d x mp_unmask_batch" % len(groups), unmask_uniform, B, "tokens")
    assert not any(o_ts) and not any(o_cs)
    plain, idx = bytes(o_plain), list(o_idx)
    for g in groups:
        assert bytes(g["plain"]) == pick(plain, PB, g["items"]) and list(g["idx"])[:len(g["items"])] == [idx[c] for c in g["items"]] and \
            not any(g["ts"]) and not any(g["cs"]), "mp_unmask_ragged_batch and mp_unmask_batch differ"


# ---------------------------------------------------------------------------------------------------------------- seating
def seating(tag, seats):
    tables = len(seats)
    first = offsets(seats)
    B = first[-1]
    fs = b"".join(eng.blake2s(b"Key Ownership Proof" + b"player %d" % l) for l in range(B))
    keys, _, proofs, st = t.keygen_batch(b"".join(seed32(2, l) for l in range(B)), fs)
    assert not any(st)
    b_keys, b_prf, b_fs, b_first = buf(keys), buf(proofs), buf(fs), u32(first)
    o_keys, o_ps, o_ts = out(tables * PB), words(B), words(tables)
    groups = []
    for P, items in by_count(seats):
        lanes = [l for k in items for l in range(first[k], first[k + 1])]
        groups.append(dict(P=P, items=items, lanes=lanes, keys=buf(pick(keys, PB, lanes)), prf=buf(pick(proofs, SSZ, lanes)), fs=buf(pick(fs, 32, lanes)),
                           out=out(len(items) * PB), ps=words(len(lanes)), ts=words(len(items))))

    def ragged():
        chk(lib.mp_aggregate_keys_ragged_batch(h, tables, b_first, b_keys, b_prf, b_fs, o_keys, o_ps, o_ts))

    def uniform():
        for g in groups:
            chk(lib.mp_aggregate_keys_batch(h, len(g["items"]), g["P"], g["keys"], g["prf"], g["fs"], g["out"], g["ps"], g["ts"]))
    lines.append("%s seating: %d tables, %d players, %d uniform call%s" % (tag, tables, B, len(groups), "s" if len(groups) > 1 else ""))
    pair(tag + "s", "mp_aggregate_keys_ragged_batch", ragged, "%d x mp_aggregate_keys_batch" % len(groups), uniform, B, "players")
    assert not any(o_ps) and not any(o_ts)
    for g in groups:
        assert bytes(g["out"]) == pick(bytes(o_keys), PB, g["items"]) and not any(g["ps"]) and not any(g["ts"]), \
            "mp_aggregate_keys_ragged_batch and mp_aggregate_keys_batch differ"


# ---------------------------------------------------------------------------------------------------------------- chains
def chaining(tag, links):
    """every table starts from the same masked deck; link j of table k is a seeded shuffle of its own"""
    tables = len(links)
    DB = N * CB
    deck0 = t.msm(2 * N, 1, b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(2 * N)), G * (2 * N))
    decks = [[deck0] for _ in range(tables)]
    proofs = [[] for _ in range(tables)]
    for j in range(max(links)):
        idx = [k for k in range(tables) if links[k] > j]
        d, p, st = t.shuffle_and_remask_batch_seeded(b"".join(decks[k][j] for k in idx), b"".join(seed32(3 + j, k) for k in idx))
        assert not any(st)
        for i, k in enumerate(idx):
            decks[k].append(d[DB * i:DB * (i + 1)])
            proofs[k].append(p[t.proof_bytes * i:t.proof_bytes * (i + 1)])
    total = sum(links)
    flat_decks, flat_prf = b"".join(b"".join(d) for d in decks), b"".join(b"".join(p) for p in proofs)
    b_links, b_decks, b_prf = u32(links), buf(flat_decks), buf(flat_prf)
    o_st = words(total)
    groups = []
    for L, items in by_count(links):
        groups.append(dict(L=L, items=items, decks=buf(b"".join(decks[k][j] for j in range(L + 1) for k in items)),
                           prf=buf(b"".join(proofs[k][j] for j in range(L) for k in items)), st=words(L * len(items))))

    def ragged():
        chk(lib.mp_verify_shuffle_chain_ragged(h, tables, b_links, None, b_decks, b_prf, o_st))

    def uniform():
        for g in groups:
            chk(lib.mp_verify_shuffle_chain(h, len(g["items"]), g["L"], None, g["decks"], g["prf"], g["st"]))
    lines.append("%s chains: %d tables of %d cards, %d links, %d uniform call%s" % (tag, tables, N, total, len(groups), "s" if len(groups) > 1 else ""))
    # the mode a table starts with: what the first call's stats say before anybody has set one
    ragged()
    if DEFAULT[0] is None:      # (read on the mixed lengths: where a cut saves no pass, as with equal lengths, the call makes none whatever is set)
        DEFAULT[0] = chain_stats()[7]
    default = DEFAULT[0]
    for mode, name in PIECES:
        chk(lib.mp_set_chain_pieces(h, mode))
        pair(tag + "c" + name[0], "mp_verify_shuffle_chain_ragged, %s%s" % (name, " (default)" if mode == default else ""), ragged,
             "%d x mp_verify_shuffle_chain" % len(groups), uniform, total, "links")
        st = chain_stats()
        lines.append("%-5s %s: cut made %s, %d passes, %d pieces, widest pass %d pieces, %.1f MB gathered on the device, %d bytes staged on the host" %
                     (tag + "c" + name[0], name, PIECES[st[7]][1], st[0], st[1], st[6], st[4] / 1e6, st[5]))
        assert not any(o_st) and not any(v for g in groups for v in g["st"]), "a chain of the rate tool does not verify"
    # device-resident inputs: the ragged call against the uniform device calls on link-major arrays that are there already; every leg ends
    # in mp_sync
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()      # noqa: E731
    d_decks, d_prf = dev(flat_decks), dev(flat_prf)
    d_st = torch.full((total,), 7, dtype=torch.int32, device="cuda")
    for g in groups:
        g["d_decks"], g["d_prf"] = dev(bytes(g["decks"])), dev(bytes(g["prf"]))
        g["d_st"] = torch.full((g["L"] * len(g["items"]),), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def ragged_dev():
        chk(lib.mp_verify_shuffle_chain_ragged_dev(h, tables, b_links, None, d_decks.data_ptr(), d_prf.data_ptr(), d_st.data_ptr()))
        eng.sync()

    def uniform_dev():
        for g in groups:
            chk(lib.mp_verify_shuffle_chain_dev(h, len(g["items"]), g["L"], None, g["d_decks"].data_ptr(), g["d_prf"].data_ptr(), g["d_st"].data_ptr()))
        eng.sync()
    for mode, name in PIECES:
        chk(lib.mp_set_chain_pieces(h, mode))
        pair(tag + "d" + name[0], "mp_verify_shuffle_chain_ragged_dev, %s%s" % (name, " (default)" if mode == default else ""), ragged_dev,
             "%d x mp_verify_shuffle_chain_dev" % len(groups), uniform_dev, total, "links")
        assert not d_st.any().item() and not any(g["d_st"].any().item() for g in groups), "a chain of the rate tool does not verify (device)"
    chk(lib.mp_set_chain_pieces(h, default))


PIECES = ((0, "whole"), (1, "binary"))
DEFAULT = [None]      # the mode a table starts with


def chain_stats():
    out = (ctypes.c_uint64 * 8)()
    chk(lib.mp_chain_ragged_stats(h, out))
    return list(out)


open_tables = (args.cards + 51) // 52
lines.append("ragged calls against one uniform call per distinct count: curve %s, one table (m = %d, n = %d), seat counts 2..10 drawn evenly; "
             "one warm-up, then %d alternating repetitions of each leg (taking turns in going first), library calls only (host buffers, PCIe included)" % (curve, m, n, args.reps))
opening("(a)", drawn(open_tables, 1))
seating("(a)", drawn(args.tables, 2))
chaining("(a)", drawn(args.chain_tables, 3))
opening("(b)", [EQUAL] * open_tables)
seating("(b)", [EQUAL] * args.tables)
chaining("(b)", [EQUAL] * args.chain_tables)
lines.append("ragged / uniform, medians: " + "   ".join(ratios) + "   (r reveal, u unmask, s seating, c chains from host buffers, d chains from device buffers, w / b pieces whole / binary; outputs of every pair identical)")
print(lines[-1])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("ragged_rate: written to %s" % args.out)
