"""Cases and runners for the CHUNKED HOST-BUFFER CALLS: mp_shuffle_and_remask_batch, mp_verify_shuffle_batch, their _keys forms and
mp_shuffle_and_remask_batch_seeded all go through prove_batch_host / verify_batch_host (csrc/capi.hip), which cut a call into chunks
by one of three schedules, rotate the two staging sets mp_table::io[2], order three streams with three events per set and apply one
offset per array and chunk.  A wrong offset or a missing wait there returns well-formed bytes of the wrong proof, or a status word of
the wrong lane; no kernel test would notice.  Shared by tests/test_host_pipeline_emu.py (development emulator, CPU: its copies are
synchronous, so it sees offsets and schedules) and tests/test_gpu_host_pipeline.py (gfx950: offsets, schedules and ordering).

Which chunks a call took is never guessed: mp_io_schedule is computed by the code the calls cut their batch with, the Python model
below restates it, run_schedule holds one to the other, and every case takes its chunk edges from mp_io_schedule.

Inputs (Inputs): the proofs of a batch differ from one another in every array the call under test is handed -- prover seeds are
BLAKE2s of a counter, masking factors 31 random bytes (below q on all four curves), permutations come from a seeded numpy generator,
keys from mp_keygen_batch on distinct seeds, and the decks are the output decks of one earlier prove call on four oracle-generated decks
under distinct factors.  Distinctness is asserted on the CPU before the device is asked.  (N = 6 has 720 permutations: batches of up to
180 proofs take distinct ones, the 16 384- and 37 648-proof batches -- whose proofs only feed the VERIFIER, which is handed no
permutation -- cannot.)

Expected bytes: the whole batch goes through ONE device-resident call (*_batch_dev, *_batch_keys_dev, *_seeded_dev), which knows no
chunks; that call is held to the C++ oracle on the first and the last proof of every chunk of the schedule under test (at most 24
oracle proofs per test); every host-buffer call must then return exactly those bytes and status words in every row.  Tampered proofs get
the oracle's word, which must be non-zero (-1 for the coordinate >= p), honest ones 0.

Every run_* function returns (failure messages, number of checks made); the tests assert that the list is empty and that the number is
the one the *_count function next to the runner computes from the MODEL's schedule -- a case list that shrinks fails the test."""
import ctypes
import hashlib
import math
import os
import struct

import numpy as np

import fs_cases as fc
import mp_oracle as po
import shuffle_edge_cases as sec
import wire_defect_cases as wd

BAD_ENCODING, BAD_PERMUTATION = -1, -2                     # include/mpshuffle.h
IO_CHUNK, IO_CHUNK_LARGE = 65536, 131072                   # capi.hip: IO_CHUNK, IO_CHUNK_LARGE
CAPI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mental-poker_amd", "csrc", "capi.hip")
# the lines of capi.hip the model restates: whoever changes one of them changes the model with it (model_is_the_sources)
MODEL_SOURCE = (
    "static size_t io_chunk_of(const mp_table* t, size_t B) { return std::min(B, t->io_chunk ? t->io_chunk : (B >= 2 * IO_CHUNK_LARGE ? IO_CHUNK_LARGE : IO_CHUNK)); }",
    "static const size_t IO_CHUNK = 65536;",
    "static const size_t IO_CHUNK_LARGE = 131072;",
    "if (B < 2 * C || C < 8) {",
    "for (size_t o = 0; o < B; o += C) v.push_back(std::min(C, B - o));",
    "#define MP_EXP_IO_RAMP 1",
    "for (size_t c = C / 8; left; c = std::min(C, (c + c / 2 + 1023) / 1024 * 1024)) {",
    "const size_t take = left >= c + c / 2 ? c : (left <= C ? left : (left + 1) / 2);",
    "const size_t r0 = C / 8, r1 = 3 * C / 8;",
    "for (size_t left = B - 2 * (r0 + r1); left;) {",
    "return io_schedule(B, C, !verify);",
)


# ================================================================================================ a. the model of the three schedules
def model_chunk(B, io_chunk):
    """capi.hip io_chunk_of: the table's mp_set_io_chunk, or by default 65 536, and 131 072 from 262 144 proofs on; never more than B"""
    return min(B, io_chunk if io_chunk else (IO_CHUNK_LARGE if B >= 2 * IO_CHUNK_LARGE else IO_CHUNK))


def model_schedule(B, io_chunk, verify):
    """capi.hip io_schedule(B, C, tail_ramp = !verify) with C = io_chunk_of"""
    C = model_chunk(B, io_chunk)
    if B < 2 * C or C < 8:                                  # "if (B < 2 * C || C < 8)": cut evenly, a ragged last chunk
        return [min(C, B - o) for o in range(0, B, C)]
    if verify:                                              # "if (!tail_ramp)" with MP_EXP_IO_RAMP = 1
        v, left, c = [], B, C // 8                          # "for (size_t c = C / 8; left; ...)"
        while left:
            # "take = left >= c + c / 2 ? c : (left <= C ? left : (left + 1) / 2)"
            take = c if left >= c + c // 2 else (left if left <= C else (left + 1) // 2)
            v.append(take)
            left -= take
            c = min(C, (c + c // 2 + 1023) // 1024 * 1024)  # "c = std::min(C, (c + c / 2 + 1023) / 1024 * 1024)"
        return v
    r0, r1 = C // 8, 3 * C // 8                             # "const size_t r0 = C / 8, r1 = 3 * C / 8;"
    v, left = [r0, r1], B - 2 * (r0 + r1)                   # "for (size_t left = B - 2 * (r0 + r1); left;)"
    while left:
        c = min(C, left)
        v.append(c)
        left -= c
    return v + [r1, r0]


ORIENTATION = (      # the issue's table: (B, C, prover schedule, verifier schedule)
    (20, 8, [1, 3, 8, 4, 3, 1], [1, 8, 6, 5]),
    (16, 8, [1, 3, 8, 3, 1], [1, 8, 7]),
    (37648, 8192, [1024, 3072, 8192, 8192, 8192, 4880, 3072, 1024], [1024, 2048, 3072, 5120, 8192, 8192, 5000, 5000]),
)
SWEEP_LARGE_C = (1024, 4096, 8192, 65536, 131072)
DEFAULT_B = (65535, 65536, 131071, 131072, 262143, 262144, 1000000)


def large_sweep(C):
    return sorted(set(range(2 * C, 6 * C + 1, C // 64)) | {2 * C - 1, 2 * C + 1, 3 * C - 1})


def model_is_the_sources():
    """the lines of capi.hip the model restates, that are not there (any more)"""
    txt = open(CAPI).read()
    return [ln for ln in MODEL_SOURCE if ln not in txt]


def edges(sched):
    """the first and the last row of every chunk"""
    rows, o = [], 0
    for c in sched:
        rows += [o, o + c - 1]
        o += c
    return sorted(set(rows))


def run_schedule(eng, coracle):
    """mp_io_schedule against the model on every (C, B) of the issue, both kinds, and the invariants the staging allocation rests on
    (the sizes sum to B, none is 0, none exceeds min(B, C)) on the library's answer alone"""
    g = coracle.gen_inputs(eng.curve, 2, 3, 7000)
    t = eng.table(2, 3, g["params"], g["pk"])
    fails, checks = [], 0
    cap = 1024
    out = (ctypes.c_size_t * cap)()

    def one(B, C):
        n = 0
        for verify in (0, 1):
            k = t.lib.mp_io_schedule(t.h, B, verify, out, cap)
            got = list(out[:min(k, cap)])
            lim = min(B, C if C else (IO_CHUNK_LARGE if B >= 2 * IO_CHUNK_LARGE else IO_CHUNK))
            if k > cap or sum(got) != B or min(got) < 1 or max(got) > lim:
                fails.append("B = %d, io chunk %d, verify %d: %d chunks %s break sum = B, 0 < size <= %d" % (B, C, verify, k, got[:16], lim))
            want = model_schedule(B, C, bool(verify))
            if got != want:
                fails.append("B = %d, io chunk %d, verify %d: mp_io_schedule gives %s, the model %s" % (B, C, verify, got[:16], want[:16]))
            n += 1
        return n
    try:
        missing = model_is_the_sources()
        if missing:
            fails.append("capi.hip no longer has the lines the model restates: %s" % missing)
        checks += 1
        for B, C, pv, vf in ORIENTATION:
            t.set_io_chunk(C)
            for verify, want in ((False, pv), (True, vf)):
                if t.io_schedule(B, verify) != want or model_schedule(B, C, verify) != want:
                    fails.append("(%d, %d) verify %d: library %s, model %s, the issue's table %s" %
                                 (B, C, verify, t.io_schedule(B, verify), model_schedule(B, C, verify), want))
                checks += 1
        for C in range(1, 71):
            t.set_io_chunk(C)
            for B in range(1, 301):
                checks += one(B, C)
        for C in SWEEP_LARGE_C:
            t.set_io_chunk(C)
            for B in large_sweep(C):
                checks += one(B, C)
        t.set_io_chunk(0)
        for B in DEFAULT_B:
            checks += one(B, 0)
        if t.lib.mp_io_schedule(t.h, 0, 0, out, cap) != 0 or t.lib.mp_io_schedule(None, 5, 0, out, cap) != 0:
            fails.append("mp_io_schedule: B = 0 or a null table must give 0 chunks")
        t.set_io_chunk(8)
        out[2] = 99
        if t.lib.mp_io_schedule(t.h, 20, 0, out, 2) != 6 or list(out[:3]) != [1, 3, 99]:      # writes the first `cap` sizes and no more
            fails.append("mp_io_schedule: cap = 2 must write two sizes and return 6, got %s" % list(out[:3]))
        checks += 2
    finally:
        t.close()
    return fails, checks


def schedule_count():
    return 1 + 2 * len(ORIENTATION) + 2 * 70 * 300 + 2 * sum(len(large_sweep(C)) for C in SWEEP_LARGE_C) + 2 * len(DEFAULT_B) + 2


# ================================================================================================ buffers
class Mem:
    """host buffers of one kind for the raw C calls: pageable numpy arrays, or page-locked memory from mp_host_alloc (only with those
    are the library's copies asynchronous).  free() releases what it handed out: call it in a finally"""

    def __init__(self, lib, pinned):
        self.lib, self.pinned, self.held = lib, pinned, []

    def new(self, count, dtype=np.uint8, fill=0xA5):
        nbytes = count * np.dtype(dtype).itemsize
        if self.pinned:
            p = self.lib.mp_host_alloc(max(nbytes, 1))
            if not p:
                raise MemoryError("mp_host_alloc(%d) failed" % nbytes)
            self.held.append(p)
            a = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p), dtype=dtype)
        else:
            a = np.empty(count, dtype=dtype)
        a[...] = fill
        return a

    def put(self, arr):
        a = self.new(arr.size, arr.dtype)
        a[...] = arr.reshape(-1)
        return a

    def free(self):
        for p in self.held:
            self.lib.mp_host_free(p)
        self.held = []


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _u8(raw):
    return np.frombuffer(raw, dtype=np.uint8)


# ================================================================================================ b. inputs, c. expected bytes
def _distinct(arr, B, what, fails):
    rows = arr.reshape(B, -1)
    if len({hashlib.blake2s(r.tobytes()).digest() for r in rows}) != B:
        fails.append("case list: the %s of the batch are not pairwise distinct" % what)


def _perms(rng, B, N):
    """B permutations of N entries, pairwise distinct where N! allows it comfortably"""
    if B * 4 > math.factorial(min(N, 12)):
        return rng.permuted(np.tile(np.arange(N, dtype=np.uint32), (B, 1)), axis=1)
    seen, out = set(), []
    while len(out) < B:
        p = rng.permutation(N).astype(np.uint32)
        if p.tobytes() not in seen:
            seen.add(p.tobytes())
            out.append(p)
    return np.stack(out)


def _seeds(tag, what, B):
    return _u8(b"".join(hashlib.blake2s(struct.pack("<QQQ", tag, what, b)).digest() for b in range(B))).reshape(B, 32)


def _factors(rng, B, N):
    rho = rng.integers(0, 256, size=(B, N * 32), dtype=np.uint8)
    rho[:, 31::32] = 0                                      # 31 random bytes: below q on all four curves
    return rho


class Inputs:
    """a table and B proofs' worth of inputs that differ in every array, with the expected outputs of ONE device-resident prove call.
    seeded: masking factors and permutations are what the device samples from the prover seeds (mp_shuffle_and_remask_batch_seeded_dev)"""

    def __init__(self, eng, coracle, torch, device, curve, m, n, B, keyed=False, seeded=False, tag=1):
        self.eng, self.co, self.curve, self.m, self.n, self.N, self.B, self.keyed, self.seeded = eng, coracle, curve, m, n, m * n, B, keyed, seeded
        self.dv = sec._Dev(torch, device)
        self.fails = []
        N, pb = self.N, eng.point_bytes
        self.pb, self.dsz = pb, 2 * N * pb
        base = [coracle.gen_inputs(curve, m, n, 7000 + k) for k in range(4)]
        self.params, self.pk = base[0]["params"], base[0]["pk"]
        self.t = eng.table(m, n, self.params, None if keyed else self.pk)
        self.psz = self.t.proof_bytes
        try:
            rng = np.random.default_rng([tag, B, N])
            self.seeds = _seeds(tag, 0, B)
            self.keys = None
            if keyed:
                pks, _, _, st = self.t.keygen_batch(_seeds(tag, 2, B).tobytes())
                assert not any(st)
                self.keys = _u8(pks).reshape(B, pb)
            # the decks: outputs of one earlier prove call on four oracle decks, under factors and permutations of their own
            d0 = _u8(b"".join(base[b % 4]["deck"] for b in range(B))).reshape(B, self.dsz)
            dk, _, st = self.dev_prove(d0, _factors(rng, B, N), _perms(rng, B, N), _seeds(tag, 1, B), self.keys)
            assert not any(st), "the earlier prove call that makes the decks failed"
            self.decks = dk
            if seeded:
                sc, pm = self.t.sample_secrets_batch(self.seeds.tobytes(), N, N)
                self.rho, self.perms = _u8(sc).reshape(B, N * 32), np.array(pm, dtype=np.uint32).reshape(B, N)
                self.exp_decks, self.exp_proofs, self.exp_status, dp, df = self.dev_prove_seeded()
                if dp.tobytes() != self.perms.tobytes() or df.tobytes() != self.rho.tobytes():
                    self.fails.append("the witnesses of mp_shuffle_and_remask_batch_seeded_dev are not those of mp_sample_secrets_batch")
            else:
                self.rho, self.perms = _factors(rng, B, N), _perms(rng, B, N)
                self.exp_decks, self.exp_proofs, self.exp_status = self.dev_prove(self.decks, self.rho, self.perms, self.seeds, self.keys)
            names = [("decks", self.decks), ("prover seeds", self.seeds), ("masking factors", self.rho), ("expected decks", self.exp_decks),
                     ("expected proofs", self.exp_proofs)] + ([("keys", self.keys)] if keyed else [])
            if B * 4 <= math.factorial(min(N, 12)):
                names.append(("permutations", self.perms))
            for what, arr in names:
                _distinct(arr, B, what, self.fails)
            if any(self.exp_status):
                self.fails.append("the device-resident prove call refused honest inputs: %s" % [b for b, v in enumerate(self.exp_status) if v][:8])
        except BaseException:
            self.t.close()
            raise

    def close(self):
        self.t.close()

    def _out(self, B):
        tz = self.dv.torch
        return (tz.full((B * self.dsz,), 0xA5, dtype=tz.uint8, device=self.dv.device),
                tz.full((B * self.psz,), 0xA5, dtype=tz.uint8, device=self.dv.device), self.dv.status(B))

    def _back(self, B, od, op, st):
        self.eng.sync()
        return od.cpu().numpy().reshape(B, self.dsz), op.cpu().numpy().reshape(B, self.psz), st.cpu().tolist()

    def dev_prove(self, decks, rho, perms, seeds, keys=None):
        """one mp_shuffle_and_remask_batch[_keys]_dev call of the whole batch: mp_set_io_chunk has no part in it"""
        B, dv = len(seeds), self.dv
        a = [dv.bytes(x.tobytes()) for x in (decks, rho, perms.astype("<u4"), seeds)]
        od, op, st = self._out(B)
        k = dv.bytes(keys.tobytes()) if keys is not None else None
        dv.sync()
        if k is not None:
            self.t.shuffle_and_remask_batch_keys_dev(B, k.data_ptr(), *(x.data_ptr() for x in a), od.data_ptr(), op.data_ptr(), st.data_ptr())
        else:
            self.t.shuffle_and_remask_batch_dev(B, *(x.data_ptr() for x in a), od.data_ptr(), op.data_ptr(), st.data_ptr())
        return self._back(B, od, op, st)

    def dev_prove_seeded(self):
        B, dv, tz, N = self.B, self.dv, self.dv.torch, self.N
        d, s = dv.bytes(self.decks.tobytes()), dv.bytes(self.seeds.tobytes())
        k = dv.bytes(self.keys.tobytes()) if self.keys is not None else None
        od, op, st = self._out(B)
        pm = tz.zeros((B * N * 4,), dtype=tz.uint8, device=dv.device)
        rf = tz.zeros((B * N * 32,), dtype=tz.uint8, device=dv.device)
        dv.sync()
        self.t.shuffle_and_remask_batch_seeded_dev(B, k.data_ptr() if k is not None else None, d.data_ptr(), s.data_ptr(), od.data_ptr(),
                                                   op.data_ptr(), st.data_ptr(), pm.data_ptr(), rf.data_ptr())
        return self._back(B, od, op, st) + (pm.cpu().numpy().view(np.uint32).reshape(B, N), rf.cpu().numpy().reshape(B, N * 32))

    def dev_verify(self, decks, shuf, proofs, keys=None):
        B, dv = len(decks), self.dv
        a = [dv.bytes(x.tobytes()) for x in (decks, shuf, proofs)]
        k = dv.bytes(keys.tobytes()) if keys is not None else None
        st = dv.status(B)
        dv.sync()
        if k is not None:
            self.t.verify_shuffle_batch_keys_dev(B, k.data_ptr(), *(x.data_ptr() for x in a), st.data_ptr())
        else:
            self.t.verify_shuffle_batch_dev(B, *(x.data_ptr() for x in a), st.data_ptr())
        return a, k, st          # (the caller syncs: under mp_set_pipeline the inputs must stay alive until then)

    def key_of(self, b, keys=None):
        keys = self.keys if keys is None else keys
        return keys[b].tobytes() if keys is not None else self.pk

    def oracle_rows(self, rows, tag):
        """the expected outputs of `rows` are the C++ oracle's -> checks made"""
        def one(b):
            return wd.prove_rc(self.co, self.curve, self.m, self.n, self.params, self.key_of(b), self.decks[b].tobytes(), self.rho[b].tobytes(),
                               [int(v) for v in self.perms[b]], self.seeds[b].tobytes())
        assert len(rows) <= 24, "at most 24 oracle proofs per test"
        for b, (rc, d, p) in zip(rows, sec._pmap(one, rows)):
            if rc != 0 or d != self.exp_decks[b].tobytes() or p != self.exp_proofs[b].tobytes():
                self.fails.append("%s: row %d of the device-resident call is not the oracle's (oracle code %d)" % (tag, b, rc))
        return len(rows)

    # ---- the host-buffer calls under test, through raw pointers
    def host_prove(self, mem, B=None, perms=None):
        B = self.B if B is None else B
        lib, t = self.t.lib, self.t
        perms = self.perms if perms is None else perms
        d, s = mem.put(self.decks[:B]), mem.put(self.seeds[:B])
        k = mem.put(self.keys[:B]) if self.keyed else None
        od, op, st = mem.new(B * self.dsz), mem.new(B * self.psz), mem.new(B, np.int32, 77)
        if self.seeded:
            pm, rf = mem.new(B * self.N, np.uint32, 0xA5A5A5A5), mem.new(B * self.N * 32)
            rc = lib.mp_shuffle_and_remask_batch_seeded(t.h, B, _ptr(k), _ptr(d), _ptr(s), _ptr(od), _ptr(op), _ptr(st), _ptr(pm), _ptr(rf))
        else:
            r, p = mem.put(self.rho[:B]), mem.put(perms[:B].astype(np.uint32))
            if self.keyed:
                rc = lib.mp_shuffle_and_remask_batch_keys(t.h, B, _ptr(k), _ptr(d), _ptr(r), _ptr(p), _ptr(s), _ptr(od), _ptr(op), _ptr(st))
            else:
                rc = lib.mp_shuffle_and_remask_batch(t.h, B, _ptr(d), _ptr(r), _ptr(p), _ptr(s), _ptr(od), _ptr(op), _ptr(st))
        self.eng._chk(rc)
        res = od.reshape(B, self.dsz).copy(), op.reshape(B, self.psz).copy(), st.tolist()
        return res + ((pm.reshape(B, self.N).copy(), rf.reshape(B, self.N * 32).copy()) if self.seeded else ())

    def host_verify(self, mem, shuf, proofs, keys=None, B=None):
        B = self.B if B is None else B
        lib, t = self.t.lib, self.t
        d, s, p = mem.put(self.decks[:B]), mem.put(shuf[:B]), mem.put(proofs[:B])
        st = mem.new(B, np.int32, 77)
        if self.keyed:
            k = mem.put((self.keys if keys is None else keys)[:B])
            rc = lib.mp_verify_shuffle_batch_keys(t.h, B, _ptr(k), _ptr(d), _ptr(s), _ptr(p), _ptr(st))
        else:
            rc = lib.mp_verify_shuffle_batch(t.h, B, _ptr(d), _ptr(s), _ptr(p), _ptr(st))
        self.eng._chk(rc)
        return st.tolist()

    # ---- defects at given rows
    def tampered(self, rows, keys=None):
        """a defect in each of `rows`, the kinds in turn: 0 the last response scalar + 1; 1 the proof of the next of `rows` (of the row
        after it where there is no other): a proof of another statement; 2 cards 0 and 1 of the shuffled deck swapped; 3 the x of the
        proof's first point := p.  Every other row stays honest.  -> (shuffled decks, proofs, expected words: the oracle's, which must
        be -1 for kind 3 and positive for the others, and 0 elsewhere)"""
        q, p, pb, cb = po.CURVES[self.curve].q, po.CURVES[self.curve].p, self.pb, 2 * self.pb
        pts, scs, psz = fc.wire_map(self.m, self.n, pb)
        assert psz == self.psz
        sh, pf = self.exp_decks.copy(), self.exp_proofs.copy()
        for k, b in enumerate(rows):
            kind = k % 4
            if kind == 0:
                o = scs[-1]
                v = (int.from_bytes(pf[b, o:o + 32].tobytes(), "little") + 1) % q
                pf[b, o:o + 32] = _u8(v.to_bytes(32, "little"))
            elif kind == 1:
                other = rows[(k + 1) % len(rows)] if len(rows) > 1 else (b + 1) % self.B
                pf[b] = self.exp_proofs[other]
            elif kind == 2:
                sh[b, :cb], sh[b, cb:2 * cb] = self.exp_decks[b, cb:2 * cb], self.exp_decks[b, :cb]
            else:
                pf[b, pts[0]:pts[0] + pb // 2] = _u8(p.to_bytes(pb // 2, "little"))
        words = sec._pmap(lambda b: self.co.verify_shuffle(self.curve, self.m, self.n, self.params, self.key_of(b, keys), self.decks[b].tobytes(),
                                                           sh[b].tobytes(), pf[b].tobytes()), rows)
        want = [0] * self.B
        for k, (b, o) in enumerate(zip(rows, words)):
            if (o != BAD_ENCODING) if k % 4 == 3 else (o <= 0):
                self.fails.append("case list: defect kind %d in row %d: the oracle says %d" % (k % 4, b, o))
            want[b] = o
        return sh, pf, want


def _rows(fails, tag, got, want, B):
    """row-wise comparison of two (B, size) arrays or two lists of B words -> checks made"""
    if isinstance(got, list):
        bad = [b for b in range(B) if got[b] != want[b]]
        if bad:
            fails.append("%s: rows %s differ (%d in all): got %s, expected %s" % (tag, bad[:8], len(bad), [got[b] for b in bad[:8]], [want[b] for b in bad[:8]]))
    elif got.shape != want[:B].shape or got.tobytes() != want[:B].tobytes():
        bad = np.nonzero((got != want[:B]).any(axis=1))[0]
        hint = []
        for b in bad[:4]:       # whose bytes are they?  (a misplaced chunk returns another row's)
            src = np.nonzero((want == got[b]).all(axis=1))[0]
            hint.append("%d%s" % (b, " (= expected row %d)" % src[0] if len(src) else ""))
        fails.append("%s: %d rows differ, first %s" % (tag, len(bad), ", ".join(hint)))
    return B


def _kinds(kinds):
    return (False, True) if kinds is None else kinds


# ================================================================================================ d. prover cases (with e's honest batches)
def run_prover(eng, coracle, torch, device, curve, m, n, C, B, keyed=False, seeded=False, pinned=None):
    """a host-buffer prove call of B proofs in chunks of C returns the bytes and words of the one device-resident call in every row (and,
    seeded with witnesses, the permutations and factors of mp_sample_secrets_batch); the host-buffer verify call, on ITS schedule, then
    gives 0 in every row; keyed: with the keys rotated by one every row fails, the rows at chunk edges with the oracle's word.  Each
    with pageable and with page-locked buffers."""
    w = Inputs(eng, coracle, torch, device, curve, m, n, B, keyed, seeded)
    fails, checks = w.fails, 0
    tag0 = "%s (%d, %d) B = %d, C = %d%s%s" % (curve, m, n, B, C, ", keyed" if keyed else "", ", seeded" if seeded else "")
    try:
        w.t.set_io_chunk(C)
        ps, vs = w.t.io_schedule(B, False), w.t.io_schedule(B, True)
        if ps != model_schedule(B, C, False) or vs != model_schedule(B, C, True):
            fails.append("%s: mp_io_schedule %s / %s is not the model's" % (tag0, ps, vs))
        checks += w.oracle_rows(edges(ps), tag0)
        if keyed:
            rot = np.roll(w.keys, 1, axis=0)
            vrows = edges(vs)
            rot_words = sec._pmap(lambda b: coracle.verify_shuffle(curve, m, n, w.params, rot[b].tobytes(), w.decks[b].tobytes(),
                                                                   w.exp_decks[b].tobytes(), w.exp_proofs[b].tobytes()), vrows)
            if not all(o > 0 for o in rot_words):
                fails.append("case list: the oracle accepts a proof under its neighbour's key")
        for pinned_ in _kinds(pinned):
            tag = tag0 + (", page-locked" if pinned_ else ", pageable")
            mem = Mem(w.t.lib, pinned_)
            try:
                got = w.host_prove(mem)
                checks += _rows(fails, tag + ": output decks", got[0], w.exp_decks, B)
                checks += _rows(fails, tag + ": proofs", got[1], w.exp_proofs, B)
                checks += _rows(fails, tag + ": prover status", got[2], w.exp_status, B)
                if seeded:
                    checks += _rows(fails, tag + ": returned permutations", got[3], w.perms, B)
                    checks += _rows(fails, tag + ": returned factors", got[4], w.rho, B)
                checks += _rows(fails, tag + ": verifier status", w.host_verify(mem, w.exp_decks, w.exp_proofs), [0] * B, B)
                if keyed:
                    st = w.host_verify(mem, w.exp_decks, w.exp_proofs, rot)
                    if not all(st):
                        fails.append("%s: rows %s pass under their neighbour's key" % (tag, [b for b in range(B) if not st[b]][:8]))
                    if [st[b] for b in vrows] != rot_words:
                        fails.append("%s: rotated keys: the words at the chunk edges are not the oracle's" % tag)
                    checks += B
            finally:
                mem.free()
    finally:
        w.close()
    return fails, checks


def prover_count(C, B, keyed=False, seeded=False, pinned=None):
    return len(edges(model_schedule(B, C, False))) + len(_kinds(pinned)) * B * (4 + (2 if seeded else 0) + (1 if keyed else 0))


def run_bad_witness(eng, coracle, torch, device, curve, m, n, C, B, pinned=None):
    """a non-permutation in the first and the last proof of every chunk: exactly those rows carry MP_ERR_BAD_PERMUTATION, every other
    row the expected bytes and 0"""
    w = Inputs(eng, coracle, torch, device, curve, m, n, B)
    fails, checks = w.fails, 0
    try:
        w.t.set_io_chunk(C)
        rows = edges(w.t.io_schedule(B, False))
        good = [b for b in range(B) if b not in rows]
        checks += w.oracle_rows(sorted({min(B - 1, b + 1) for b in rows} - set(rows)), "bad witnesses")     # the honest neighbours
        perms = w.perms.copy()
        for b in rows:
            perms[b, 1] = perms[b, 0]                       # an entry twice: not a permutation
        want = [BAD_PERMUTATION if b in rows else 0 for b in range(B)]
        for pinned_ in _kinds(pinned):
            tag = "%s (%d, %d) B = %d, C = %d, bad witnesses, %s" % (curve, m, n, B, C, "page-locked" if pinned_ else "pageable")
            mem = Mem(w.t.lib, pinned_)
            try:
                od, op, st = w.host_prove(mem, perms=perms)
                checks += _rows(fails, tag + ": status", st, want, B)
                checks += _rows(fails, tag + ": output decks", od[good], w.exp_decks[good], len(good))
                checks += _rows(fails, tag + ": proofs", op[good], w.exp_proofs[good], len(good))
            finally:
                mem.free()
    finally:
        w.close()
    return fails, checks


def bad_witness_count(C, B, pinned=None):
    rows = edges(model_schedule(B, C, False))
    return len(sorted({min(B - 1, b + 1) for b in rows} - set(rows))) + len(_kinds(pinned)) * (B + 2 * (B - len(rows)))


# ================================================================================================ e. verifier cases
MODES = ("merged", "per equation", "groups of 3")
GROUP_L = 3


def _mode(t, mode, m, n):
    t.set_latency_batch(0)
    t.set_group_adapt(False)
    t.set_merged_verify(mode != "per equation")
    t.set_group_verify(GROUP_L * (4 * m * n + 11 * m + 8) if mode == "groups of 3" else 0, 0)


def run_verifier(eng, coracle, torch, device, curve, m, n, C, B, modes=MODES, pinned=None, keyed=False):
    """proofs of the device prover (the rows at the verifier's chunk edges held to the oracle) through the host-buffer verify call in
    chunks of C: honest batches give 0 everywhere; with a defect in the first and the last proof of every chunk -- the kinds of
    Inputs.tampered in turn, honest proofs between them -- the tampered rows get the oracle's words and every other row 0, under merged
    verification, equation by equation and with group equations forced to 3 proofs, where the chunks of one call take different group
    sizes, or none"""
    w = Inputs(eng, coracle, torch, device, curve, m, n, B, keyed)
    fails, checks = w.fails, 0
    tag0 = "%s (%d, %d) B = %d, C = %d%s" % (curve, m, n, B, C, ", keyed" if keyed else "")
    try:
        w.t.set_io_chunk(C)
        vs = w.t.io_schedule(B, True)
        if vs != model_schedule(B, C, True):
            fails.append("%s: mp_io_schedule %s is not the model's" % (tag0, vs))
        rows = edges(vs)
        checks += w.oracle_rows(rows, tag0)
        sh, pf, want = w.tampered(rows)
        for mode in modes:
            _mode(w.t, mode, m, n)
            if mode == "groups of 3":
                gs = [w.t.group_size(c) for c in vs]
                if not any(gs) or all(gs):
                    fails.append("%s: the chunks %s take groups of %s: at least one grouped and one ungrouped chunk are wanted" % (tag0, vs, gs))
                checks += 1
            for pinned_ in _kinds(pinned):
                tag = "%s, %s, %s" % (tag0, mode, "page-locked" if pinned_ else "pageable")
                mem = Mem(w.t.lib, pinned_)
                try:
                    checks += _rows(fails, tag + ": honest", w.host_verify(mem, w.exp_decks, w.exp_proofs), [0] * B, B)
                    checks += _rows(fails, tag + ": defects at chunk edges", w.host_verify(mem, sh, pf), want, B)
                finally:
                    mem.free()
    finally:
        w.close()
    return fails, checks


def verifier_count(C, B, modes=MODES, pinned=None):
    return len(edges(model_schedule(B, C, True))) + len(modes) * len(_kinds(pinned)) * 2 * B + (1 if "groups of 3" in modes else 0)


def run_pipeline_setting(eng, coracle, torch, device, curve, m, n, C, B, pinned=None):
    """mp_set_pipeline(1) on the table: the host-buffer verify call gives the same words (it is not pipelined, NoPipeline), and a
    device-resident verify call issued afterwards is still deferred -- its per-equation pass has not run when it returns
    (mp_reverified_count stands still) and runs at mp_sync, after which its words are the expected ones"""
    w = Inputs(eng, coracle, torch, device, curve, m, n, B)
    fails, checks = w.fails, 0
    tag = "%s (%d, %d) B = %d, C = %d, pipelined table" % (curve, m, n, B, C)
    try:
        w.t.set_io_chunk(C)
        rows = edges(w.t.io_schedule(B, True))
        sh, pf, want = w.tampered(rows)
        _mode(w.t, "merged", m, n)
        w.t.set_pipeline(1)
        for pinned_ in _kinds(pinned):
            mem = Mem(w.t.lib, pinned_)
            try:
                checks += _rows(fails, tag + ": host-buffer verify", w.host_verify(mem, sh, pf), want, B)
            finally:
                mem.free()
            seen = w.t.reverified_count()
            keep = w.dev_verify(w.decks, sh, pf)
            if w.t.reverified_count() != seen:
                fails.append("%s: the device-resident verify call after the host-buffer one was not deferred" % tag)
            eng.sync()
            if w.t.reverified_count() == seen:
                fails.append("%s: mp_sync ran no per-equation pass for the deferred call" % tag)
            checks += 2 + _rows(fails, tag + ": deferred device-resident verify", keep[2].cpu().tolist(), want, B)
        w.t.set_pipeline(0)
    finally:
        w.close()
    return fails, checks


def pipeline_count(B, pinned=None):
    return len(_kinds(pinned)) * (2 * B + 2)


# ---- shared staging: chain verification in slices gathers into io[0], which the host-buffer calls rotate with io[1]
CHAIN_T, CHAIN_L = 3, 2
STAGING_OPS = ("chain in slices", "host verify, C = 8", "chain in slices", "host prove, C = 9", "host prove, C = 4")


def run_shared_staging(eng, coracle, torch, device, curve, m, n, pinned=None):
    """on ONE table in turn: a chain verification in slices of 2 of 3 tables, a chunked host verify (20 proofs, C = 8, defects at
    the chunk edges), the chain again, a chunked host prove with a larger C than before (19 proofs, C = 9) and a smaller one (11
    proofs, C = 4): every result is what the same call gives on a fresh table, the chain's words name exactly its one bad link and the
    others are the expected bytes"""
    B = 20
    w = Inputs(eng, coracle, torch, device, curve, m, n, B)
    fails, checks = w.fails, 0
    T, L = CHAIN_T, CHAIN_L
    try:
        # T chains of L links on the first T decks; link 1 of table 0 carries table 1's proof
        chain, proofs = [w.decks[:T]], []
        for j in range(L):
            d, p, st = w.dev_prove(chain[j], w.rho[j * T:(j + 1) * T], w.perms[j * T:(j + 1) * T], w.seeds[j * T:(j + 1) * T])
            assert not any(st)
            chain.append(d)
            proofs.append(p.copy())
        proofs[1][0] = proofs[1][1]
        cd, cp = b"".join(x.tobytes() for x in chain), b"".join(x.tobytes() for x in proofs)
        w.t.set_io_chunk(8)
        sh, pf, want = w.tampered(edges(w.t.io_schedule(B, True)))

        def op(w_, t, name, mem):
            save, w_.t = w_.t, t
            try:
                if name == "chain in slices":
                    t.set_chain_slice(T - 1)
                    st = t.verify_shuffle_chain(T, L, cd, cp)
                    if t.chain_last_slice() != T - 1:
                        fails.append("the chain did not run in slices of %d" % (T - 1))
                    return st
                if name == "host verify, C = 8":
                    t.set_io_chunk(8)
                    return w_.host_verify(mem, sh, pf)
                C, Bp = (9, 19) if name == "host prove, C = 9" else (4, 11)
                t.set_io_chunk(C)
                od, opf, st = w_.host_prove(mem, Bp)
                return od.tobytes(), opf.tobytes(), st
            finally:
                w_.t = save
        for pinned_ in _kinds(pinned):
            tag = "%s (%d, %d) shared staging, %s" % (curve, m, n, "page-locked" if pinned_ else "pageable")
            mem = Mem(w.t.lib, pinned_)
            try:
                fresh = []
                for name in STAGING_OPS:
                    t = eng.table(m, n, w.params, w.pk)
                    try:
                        fresh.append(op(w, t, name, mem))
                    finally:
                        t.close()
                t = eng.table(m, n, w.params, w.pk)
                try:
                    for name, ref in zip(STAGING_OPS, fresh):
                        if op(w, t, name, mem) != ref:
                            fails.append("%s: '%s' after the calls before it differs from a fresh table's" % (tag, name))
                        checks += 1
                finally:
                    t.close()
                bad_link = [1 if i == 1 * T + 0 else 0 for i in range(L * T)]
                if [1 if v else 0 for v in fresh[0]] != bad_link or fresh[0][T] <= 0 or fresh[1] != want:
                    fails.append("%s: fresh tables: chain words %s, verify words %s (expected %s)" % (tag, fresh[0], fresh[1], want))
                for (od, opf, st), Bp in ((fresh[3], 19), (fresh[4], 11)):
                    if od != w.exp_decks[:Bp].tobytes() or opf != w.exp_proofs[:Bp].tobytes() or st != [0] * Bp:
                        fails.append("%s: fresh table: the host prove of %d proofs is not the expected bytes" % (tag, Bp))
                checks += 3
            finally:
                mem.free()
    finally:
        w.close()
    return fails, checks


def staging_count(pinned=None):
    return len(_kinds(pinned)) * (len(STAGING_OPS) + 3)
