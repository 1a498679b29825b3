#!/usr/bin/env python3
"""The device conversions between wire v1 and arkworks-canonical bytes beside the calls they feed: 65 536 proofs and decks of 52 cards
(m, n) = (2, 26) on the STARK curve and on secp256k1, one table each, device-resident data.
  (a) the four _dev conversions -- mp_proof_serialize_dev, mp_deck_serialize_dev behind the prover, mp_proof_deserialize_dev,
      mp_deck_deserialize_dev in front of the verifier: time per call, points/s, and the time as a fraction of the prove / verify call
  (b) mp_proofs_deserialize_batch (host buffers, page-locked and pageable) against a loop of mp_proof_deserialize over the same bytes
      on 16 host threads -- the only path before the device conversion existed.  The host loop is timed on the first --host-proofs proofs
      of the batch (its square roots take minutes on all of them) and reported as a rate
  (c) the proof decompressor's point rate against tools/decompress_bench.py's (k_decompress on decks) in the same run
One warm-up and --reps timed repetitions each, a host clock around work that ends in mp_sync.  Every figure goes to the output file
(default profiles/canonical_rates.txt)."""
import argparse
import ctypes
import importlib
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: conftest.load_pkg)
mp = importlib.import_module("mental-poker_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--curves", default="stark,secp256k1")
ap.add_argument("--fb-bits", type=int, default=16, help="fixed-base window width of the table whose prove / verify calls are the yardstick")
ap.add_argument("--host-proofs", type=int, default=2048, help="proofs the host loop of mp_proof_deserialize is timed on")
ap.add_argument("--host-threads", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canonical_rates.txt"))
args = ap.parse_args()

m, n = 2, 26
N, B = m * n, args.batch
gpu = torch.device("cuda", 0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(eng, fn, reps):
    fn()
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    eng.sync()
    return (time.perf_counter() - t0) / reps


def run(curve):
    # the yardstick first, in a process of its own: tools/decompress_bench.py as it stands
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "decompress_bench.py"), curve], capture_output=True, text=True, check=True)
    yard = float(re.search(r"([0-9.]+) M points/s", r.stdout).group(1))
    say("[%s] tools/decompress_bench.py: %s" % (curve, r.stdout.strip()))

    eng = mp.Engine(curve, 0)
    lib, cid = eng.lib, mp._native.CURVE_IDS[curve]
    PB, CB = eng.point_bytes, lib.mp_serialized_point_size(cid)
    params = eng.setup(m, n, bytes([1] * 32))
    t = eng.table(m, n, params, params[PB:2 * PB], fb_bits=args.fb_bits)
    ps, cps = lib.mp_proof_size_curve(cid, m, n), lib.mp_serialized_proof_size(cid, m, n)
    ds, cds = 2 * N * PB, lib.mp_serialized_deck_size(cid, N)
    np_, ns_ = 11 * m + 8, 5 * n + 9

    dev = lambda rows, width: torch.empty(rows, width, dtype=torch.uint8, device=gpu)      # noqa: E731
    deck = eng.setup(m, 2 * N - 3, bytes([7] * 32))                                      # 2 N random points: one deck
    d_decks = torch.frombuffer(bytearray(deck), dtype=torch.uint8).to(gpu).repeat(B, 1).contiguous()
    d_seeds = torch.arange(B * 8, dtype=torch.int32, device=gpu).view(torch.uint8).view(B, 32).contiguous()
    d_shuf, d_proofs, d_st = dev(B, ds), dev(B, ps), torch.empty(B, dtype=torch.int32, device=gpu)
    d_cproofs, d_cdecks, d_back_p, d_back_d = dev(B, cps), dev(B, cds), dev(B, ps), dev(B, ds)
    torch.cuda.synchronize()
    ok = lambda: int(d_st.abs().sum().item()) == 0      # noqa: E731

    prove = lambda: t.shuffle_and_remask_batch_seeded_dev(B, None, d_decks.data_ptr(), d_seeds.data_ptr(), d_shuf.data_ptr(),      # noqa: E731
                                                          d_proofs.data_ptr(), d_st.data_ptr())
    verify = lambda: t.verify_shuffle_batch_dev(B, d_decks.data_ptr(), d_shuf.data_ptr(), d_back_p.data_ptr(), d_st.data_ptr())   # noqa: E731
    conv = {
        "mp_proof_serialize_dev": (lambda: eng.proof_serialize_dev(m, n, B, d_proofs.data_ptr(), d_cproofs.data_ptr(), d_st.data_ptr()), np_),
        "mp_deck_serialize_dev": (lambda: eng.deck_serialize_dev(B, N, d_shuf.data_ptr(), d_cdecks.data_ptr(), d_st.data_ptr()), 2 * N),
        "mp_proof_deserialize_dev": (lambda: eng.proof_deserialize_dev(m, n, B, d_cproofs.data_ptr(), d_back_p.data_ptr(), d_st.data_ptr()), np_),
        "mp_deck_deserialize_dev": (lambda: eng.deck_deserialize_dev(B, N, d_cdecks.data_ptr(), d_back_d.data_ptr(), d_st.data_ptr()), 2 * N),
    }
    t_prove = timed(eng, prove, 2)
    assert ok()
    times = {}
    for name, (fn, pts) in conv.items():
        times[name] = timed(eng, fn, args.reps)
        assert ok(), name
    assert torch.equal(d_back_p, d_proofs) and torch.equal(d_back_d, d_shuf)
    t_verify = timed(eng, verify, 2)
    assert ok()
    say("[%s] (m, n) = (%d, %d), %d proofs, fixed-base windows of %d bits: prove %.1f ms (%.0f k proofs/s), verify %.1f ms (%.0f k proofs/s)"
        % (curve, m, n, B, args.fb_bits, 1e3 * t_prove, B / t_prove / 1e3, 1e3 * t_verify, B / t_verify / 1e3))
    for name, (fn, pts) in conv.items():
        feeds, t_feed = ("prove", t_prove) if "_serialize" in name else ("verify", t_verify)
        say("[%s] %-26s %8.3f ms  %7.1f M points/s  %5.2f %% of the %s call" % (curve, name, 1e3 * times[name], B * pts / times[name] / 1e6,
                                                                            100 * times[name] / t_feed, feeds))
    rate = B * np_ / times["mp_proof_deserialize_dev"] / 1e6
    say("[%s] proof decompressor (points and scalars of %d proofs): %.1f M points/s = %.2f of decompress_bench.py's %.1f M points/s"
        % (curve, B, rate, rate / yard, yard))

    # (b) host buffers
    canon = bytes(d_cproofs.cpu().numpy().tobytes())
    want = bytes(d_proofs.cpu().numpy().tobytes())
    for pinned in (True, False):
        t0 = time.perf_counter()
        out, st = eng.proofs_deserialize_batch(m, n, B, canon, pinned=pinned)
        dt = time.perf_counter() - t0
        assert out == want and not any(st)
        say("[%s] mp_proofs_deserialize_batch through the Python binding, %s buffers (its copies into and out of them included): %.1f ms, "
            "%.0f k proofs/s" % (curve, "page-locked" if pinned else "pageable", 1e3 * dt, B / dt / 1e3))
    h_in, h_out, h_st = (lib.mp_host_alloc(k) for k in (len(canon), len(want), 4 * B))
    ctypes.memmove(h_in, canon, len(canon))
    call = lambda: eng._chk(lib.mp_proofs_deserialize_batch(eng.h, m, n, B, h_in, h_out, h_st))      # noqa: E731
    dt = timed(eng, call, args.reps)
    assert ctypes.string_at(h_out, len(want)) == want
    for h in (h_in, h_out, h_st):
        lib.mp_host_free(ctypes.c_void_p(h))
    say("[%s] mp_proofs_deserialize_batch, page-locked buffers, the call alone (upload, conversion, download): %.1f ms, %.0f k proofs/s"
        % (curve, 1e3 * dt, B / dt / 1e3))
    H = min(args.host_proofs, B)
    ser = mp.Serializer(curve)
    rows = [canon[k * cps:(k + 1) * cps] for k in range(H)]
    with ThreadPoolExecutor(args.host_threads) as ex:
        t0 = time.perf_counter()
        got = list(ex.map(lambda b: ser.proof_deserialize(m, n, b), rows))
        dh = time.perf_counter() - t0
    assert b"".join(got) == want[:H * ps]
    say("[%s] loop of mp_proof_deserialize on %d host threads, %d of the same proofs: %.1f ms, %.2f k proofs/s -- the batch form is %.0f x"
        % (curve, args.host_threads, H, 1e3 * dh, H / dh / 1e3, (B / dt) / (H / dh)))
    say()
    t.close()
    eng.close()


for c in args.curves.split(","):
    run(c)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
