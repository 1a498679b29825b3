#!/usr/bin/env python3
"""What drawing the shuffle witnesses on the device costs, on the STARK curve at (m, n) = (2, 26), for batches of 1 024 and 65 536 proofs:
  (a) the sampler alone: mp_sample_secrets_batch_dev(S = P = 52), seeds in HBM, in witnesses/s;
  (b) mp_shuffle_and_remask_batch_seeded_dev against mp_shuffle_and_remask_batch_dev on witnesses that are in HBM already (the
      sampler's own), alternating in one process;
  (c) mp_shuffle_and_remask_batch_seeded against mp_shuffle_and_remask_batch, host buffers, PCIe included, every buffer page-locked
      (mp_host_alloc), alternating in one process.
One warm-up and three timed repetitions each; decks, proofs and status words of each pair are asserted equal.  No figure is expected in
advance and none is an acceptance bar: every one, whichever way it falls, goes to the output file (default profiles/sample_rates.txt) with
the time ratios seeded / unseeded.

Every step (a step = one of a, b, c at one batch size) runs in a child process of its own under a time limit; the first step that fails
or runs out of time ends the run, and nothing is started after it."""
import argparse
import ctypes
import hashlib
import importlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[1024, 65536])
ap.add_argument("--fb-bits", type=int, default=16, help="fixed-base window width of the table")
ap.add_argument("--step", choices=["sampler", "dev", "host"], help="run this one step at --batch (what the driver starts)")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
ap.add_argument("--commit", default=None, help="the commit the figures belong to (default: git rev-parse HEAD)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rates.txt"))
args = ap.parse_args()

curve, m, n, PB = "stark", 2, 26, 64
N = m * n
REPS = 3


def step(kind, B):
    import torch      # (first: its HIP runtime has to be in the process before libmpshuffle.so's)
    mp = importlib.import_module("mental-poker_amd")
    eng = mp.Engine(curve, 0)
    lib = eng.lib
    rng = mp.ChaCha20Rng(bytes([7] * 32))
    sc = lambda k: int(k).to_bytes(32, "little")      # noqa: E731
    params = eng.setup(m, n, bytes([1] * 32))
    G = params[:PB]
    boot = eng.table(m, n, params, params[PB:2 * PB])
    pts = boot.msm(2 * N + 1, 1, b"".join(sc(mp.fr_rand(curve, rng)) for _ in range(2 * N + 1)), G * (2 * N + 1))
    boot.close()
    deck, pk = pts[:2 * N * PB], pts[2 * N * PB:]
    t = eng.table(m, n, params, pk, args.fb_bits)
    psz, dsz = t.proof_bytes, 2 * N * PB
    seeds = b"".join(hashlib.blake2s(b"sample rate seed %d" % b).digest() for b in range(B))
    lines = []

    def chk(rc):
        if rc != 0:
            raise RuntimeError("call failed: %d %s" % (rc, lib.mp_last_error().decode()))

    def report(name, ts, unit="proofs"):
        best = min(ts)
        lines.append("%-66s %s ms  (best %.3f ms = %.0f %s/s)" % (name, " ".join("%9.3f" % (v * 1e3) for v in ts), best * 1e3, B / best, unit))
        return best

    def alternate(unseeded, seeded):
        unseeded()
        seeded()
        tu, ts = [], []
        for _ in range(REPS):
            for fn, acc in ((unseeded, tu), (seeded, ts)):
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        return tu, ts

    if kind in ("sampler", "dev"):
        dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")      # noqa: E731
        d_seeds = dev(seeds)
        d_rho = torch.zeros(B * N * 32, dtype=torch.uint8, device="cuda")
        d_perm = torch.zeros(B * N, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def sample():
            chk(lib.mp_sample_secrets_batch_dev(t.h, B, d_seeds.data_ptr(), N, N, d_rho.data_ptr(), d_perm.data_ptr()))
            eng.sync()
        sample()
    if kind == "sampler":
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            sample()
            ts.append(time.perf_counter() - t0)
        report("(a) B = %6d  mp_sample_secrets_batch_dev(S = P = %d)" % (B, N), ts, "witnesses")
        first = mp.secret_stream(curve, seeds[:32], N, N)
        assert d_perm[:N].cpu().tolist() == first[1] and bytes(d_rho[:N * 32].cpu().numpy().tobytes()) == b"".join(sc(v) for v in first[0]), \
            "the sampler's first witness is not protocol.secret_stream's"
    elif kind == "dev":
        d_decks = dev(deck).repeat(B)
        outs = [[torch.zeros(B * dsz, dtype=torch.uint8, device="cuda"), torch.zeros(B * psz, dtype=torch.uint8, device="cuda"),
                 torch.full((B,), 7, dtype=torch.int32, device="cuda")] for _ in range(2)]
        torch.cuda.synchronize()
        t.reserve(B)

        def unseeded():
            o = outs[0]
            chk(lib.mp_shuffle_and_remask_batch_dev(t.h, B, d_decks.data_ptr(), d_rho.data_ptr(), d_perm.data_ptr(), d_seeds.data_ptr(),
                                                    o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr()))
            eng.sync()

        def seeded():
            o = outs[1]
            chk(lib.mp_shuffle_and_remask_batch_seeded_dev(t.h, B, None, d_decks.data_ptr(), d_seeds.data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                                                           o[2].data_ptr(), None, None))
            eng.sync()
        tu, ts = alternate(unseeded, seeded)
        assert all(torch.equal(a, b) for a, b in zip(*outs)) and not outs[0][2].any().item(), "seeded and unseeded _dev calls differ"
        a = report("(b) B = %6d  mp_shuffle_and_remask_batch_dev, witnesses in HBM" % B, tu)
        b = report("(b) B = %6d  mp_shuffle_and_remask_batch_seeded_dev" % B, ts)
        lines.append("(b) B = %6d  seeded / unseeded = %.4f" % (B, b / a))
    else:
        sc_b, pm = t.sample_secrets_batch(seeds, N, N)

        def pinned(nbytes, raw=None):
            p = lib.mp_host_alloc(nbytes)
            if not p:
                raise RuntimeError("mp_host_alloc failed")
            if raw is not None:
                ctypes.memmove(p, raw, len(raw))
            return p
        h_decks = pinned(B * dsz)
        for b in range(B):
            ctypes.memmove(h_decks + b * dsz, deck, dsz)
        h_rho, h_seeds = pinned(len(sc_b), sc_b), pinned(len(seeds), seeds)
        h_perm = pinned(4 * B * N, bytes((ctypes.c_uint32 * (B * N))(*pm)))
        outs = [[pinned(B * dsz), pinned(B * psz), pinned(4 * B)] for _ in range(2)]

        def unseeded():
            o = outs[0]
            chk(lib.mp_shuffle_and_remask_batch(t.h, B, h_decks, h_rho, h_perm, h_seeds, o[0], o[1], o[2]))

        def seeded():
            o = outs[1]
            chk(lib.mp_shuffle_and_remask_batch_seeded(t.h, B, None, h_decks, h_seeds, o[0], o[1], o[2], None, None))
        tu, ts = alternate(unseeded, seeded)
        for (pa, pb_), nbytes in zip(zip(*outs), (B * dsz, B * psz, 4 * B)):
            assert ctypes.string_at(pa, nbytes) == ctypes.string_at(pb_, nbytes), "seeded and unseeded host-buffer calls differ"
        assert ctypes.string_at(outs[0][2], 4 * B) == bytes(4 * B), "a proof was refused"
        a = report("(c) B = %6d  mp_shuffle_and_remask_batch, page-locked host buffers" % B, tu)
        b = report("(c) B = %6d  mp_shuffle_and_remask_batch_seeded, page-locked host buffers" % B, ts)
        up = (dsz + N * 32 + N * 4 + 32, dsz + 32)
        lines.append("(c) B = %6d  seeded / unseeded = %.4f   (uploads per proof: %d B unseeded, %d B seeded; downloads %d B)" % (B, b / a, up[0], up[1], dsz + psz + 4))
        for o in outs:
            for p in o:
                lib.mp_host_free(p)
        for p in (h_decks, h_rho, h_seeds, h_perm):
            lib.mp_host_free(p)
    if kind == "sampler" and B == args.batches[0]:
        prop = torch.cuda.get_device_properties(0)
        lines.insert(0, "machine: %s (%s, %d CUs, %.0f GB), ROCm/HIP %s, table: fixed-base windows of %d bits" % (
            prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, torch.version.hip, t.fb_bits))
    t.close()
    eng.close()
    print("\n".join(lines), flush=True)


def main():
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"
    lines = ["secrets from seeds (mpshuffle secret stream v1): curve %s, (m, n) = (%d, %d), warm-up + %d repetitions, wall clock around call + "
             "mp_sync; commit %s" % (curve, m, n, REPS, commit)]
    for kind in ("sampler", "dev", "host"):
        for B in args.batches:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--batch", str(B), "--fb-bits", str(args.fb_bits), "--batches"] + \
                  [str(b) for b in args.batches]
            try:
                res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print("sample_rate: step %s at B = %d ran past %d s: stopping here" % (kind, B, args.step_timeout), flush=True)
                return 1
            if res.returncode != 0:      # a fault, an abort or a failed assertion: nothing more is started on the GPU
                print(res.stderr.decode()[-3000:])
                print("sample_rate: step %s at B = %d ended with %d: stopping here" % (kind, B, res.returncode), flush=True)
                return 1
            text = res.stdout.decode().strip()
            print(text, flush=True)
            lines += text.splitlines()
    head = [l for l in lines if l.startswith("machine:")]
    lines = lines[:1] + head + [l for l in lines[1:] if not l.startswith("machine:")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("sample_rate: done")
    return 0


if __name__ == "__main__":
    if args.step:
        step(args.step, args.batch)
    else:
        sys.exit(main())
