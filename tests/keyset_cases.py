"""Cases and runners for KEY SETS WHOSE SLOTS CHANGE: mp_keyset_create_empty, mp_keyset_update[_dev], mp_keyset_clear, mp_keyset_live and
what the two _keyset_dev shuffle calls then do with a live and with an empty slot; the seeded prover, ragged chain verification and dealing by index, and seating straight into a set.  Shared by tests/test_keyset_emu.py (the kernel bodies
under the development emulator, CPU) and tests/test_gpu_keyset.py (the gfx950 build) -- same cases, same expectations.

Where the expectations come from.  A slot's content is judged by what it SERVES: a proof made by index is the C++ oracle's bytes
(coracle.shuffle_and_remask) under the key the slot holds at that moment, the oracle's proof under that key verifies by index with word 0,
and a slot that holds nothing gives MP_ERR_BAD_ARGUMENT to the proof that names it, as the index one past the set does.  `Rig.serves` asks
that of every slot it is given plus that index, in ONE mixed batch, so live slots sit between empty ones.  Words that are not the oracle's
are those of an existing key-passing call on the same input (mp_verify_shuffle_batch_keys, mp_shuffle_and_remask_batch_keys_dev).
Defective keys are checked in Python integers before the device sees them (tests/wire_defect_cases.py Pts).

Every run_* function returns (failure messages, number of checks made); the tests assert that the list is empty and that the number is
the one the *_count function next to the runner computes from its arguments alone -- a case list that shrinks fails the test."""
import ctypes

import mp_oracle as po
import shuffle_edge_cases as sec
import trait_cases as tc
import wire_defect_cases as wd

BAD_ENCODING, BAD_ARGUMENT = -1, -3      # include/mpshuffle.h
MN = (2, 3)
CURVES = ("stark", "secp256k1", "bn254", "bls12_377")
UPDATE_COUNTS = (1, 2, 63, 64, 65)
REFUSED_SET = 65
REFUSED_AT = (0, 32, 64)                 # first, a middle and the last position of an update of 65
N_STMT = 4
SENTINEL = 55                            # what shuffle_edge_cases._Dev.status fills with


def defects(curve):
    names = ["the identity", "x := p", "off the curve"]
    if curve in po.COFACTOR:
        names.append("outside the subgroup")
    return names


class World:
    """one curve: parameters, four statements, as many keys as the cases ask for, and the oracle's proofs by (key, statement)"""

    def __init__(self, coracle, curve):
        self.co, self.curve = coracle, curve
        self.m, self.n = MN
        self.N = self.m * self.n
        self.c = wd.Pts(coracle, curve)
        self.gen = [coracle.gen_inputs(curve, self.m, self.n, 7300 + k) for k in range(N_STMT)]
        self.params = self.gen[0]["params"]
        self.dsz, self.psz = len(self.gen[0]["deck"]), coracle.proof_size(self.m, self.n, curve)
        self._keys, self._proofs = {}, {}

    def keys(self, first, count):
        """`count` distinct honest keys, numbered from `first`"""
        todo = [j for j in range(first, first + count) if j not in self._keys]
        for j, g in zip(todo, sec._pmap(lambda j: self.co.gen_inputs(self.curve, self.m, self.n, 7400 + j), todo)):
            self._keys[j] = g["pk"]
        out = [self._keys[j] for j in range(first, first + count)]
        assert len(set(out)) == count
        return out

    def proofs(self, pairs):
        """[(key, statement number)] -> [(shuffled deck, proof)] of the oracle"""
        todo = sorted(set(p for p in pairs if p not in self._proofs))

        def one(p):
            g = self.gen[p[1]]
            return self.co.shuffle_and_remask(self.curve, self.m, self.n, self.params, p[0], g["deck"], g["rho"], g["perm"], g["prover_seed"])
        for p, r in zip(todo, sec._pmap(one, todo)):
            self._proofs[p] = r
        return [self._proofs[p] for p in pairs]

    def defect(self, name, key):
        """a key the set must refuse; each is shown to be what its name says in Python integers"""
        c = self.c
        if name == "the identity":
            return c.inf
        if name == "x := p":
            bad = c.x_is_p(key)
            assert c.xy(bad)[0] >= c.p
            return bad
        if name == "off the curve":
            return c.off_curve(key)
        bad = tc.off_subgroup_points()[0]
        assert c.outside_subgroup(bad)
        return bad

    def near_miss(self):
        """a key next to a refused one that must be ACCEPTED: the curve point with the largest x; where the curve has a cofactor that
        point is not a key (it lies outside the subgroup), and the near miss of the subgroup test is a subgroup point"""
        c = self.c
        if c.cofactor:
            key = self.keys(900, 1)[0]
            assert not c.outside_subgroup(key)
            return key
        key = c.largest_x()
        assert c.xy(key)[0] < c.p and c.cv.is_on_curve(c.xy(key))
        return key


_WORLDS = {}


def world(coracle, curve):
    if curve not in _WORLDS:
        _WORLDS[curve] = World(coracle, curve)
    return _WORLDS[curve]


class Rig:
    """a keyless table of the world's parameters on `eng`, device buffers through torch, and the running list of failures and checks"""

    def __init__(self, eng, coracle, curve, torch, device):
        self.eng, self.w, self.curve = eng, world(coracle, curve), curve
        self.dv = sec._Dev(torch, device)
        self.t = eng.table(self.w.m, self.w.n, self.w.params, None)
        self.fails, self.checks = [], 0

    def close(self):
        self.t.close()
        return self.fails[:40], self.checks

    def check(self, ok, msg, *args):
        self.checks += 1
        if not ok:
            self.fails.append("%s: " % self.curve + (msg % args if args else msg))

    # ---- the calls
    def _inputs(self, B):
        g = [self.w.gen[b % N_STMT] for b in range(B)]
        return (self.dv.bytes(b"".join(x["deck"] for x in g)), self.dv.bytes(b"".join(x["rho"] for x in g)),
                self.dv.ints([v for x in g for v in x["perm"]]), self.dv.bytes(b"".join(x["prover_seed"] for x in g)))

    def _outputs(self, B):
        return self.dv.bytes(bytes(B * self.w.dsz)), self.dv.bytes(bytes(B * self.w.psz)), self.dv.status(B)

    def _cut(self, od, op, st):
        d, p = bytes(od.cpu().numpy().tobytes()), bytes(op.cpu().numpy().tobytes())
        B, dsz, psz = len(st), self.w.dsz, self.w.psz
        return st.cpu().tolist(), [d[dsz * b:dsz * (b + 1)] for b in range(B)], [p[psz * b:psz * (b + 1)] for b in range(B)]

    def prove_queue(self, ks, idx):
        """proof b: statement b % N_STMT by index idx[b]; queued, nothing is waited for -> the buffers (inputs too: they stay alive)"""
        B = len(idx)
        ins, outs, d_idx = self._inputs(B), self._outputs(B), self.dv.ints(idx)
        self.dv.sync()
        self.t.shuffle_and_remask_batch_keyset_dev(ks, B, d_idx.data_ptr(), *(x.data_ptr() for x in ins), *(x.data_ptr() for x in outs))
        return ins, d_idx, outs

    def prove(self, ks, idx):
        held = self.prove_queue(ks, idx)
        self.eng.sync()
        return self._cut(*held[2])

    def prove_keys(self, keys):
        B = len(keys)
        ins, outs, d_keys = self._inputs(B), self._outputs(B), self.dv.bytes(b"".join(keys))
        self.dv.sync()
        self.t.shuffle_and_remask_batch_keys_dev(B, d_keys.data_ptr(), *(x.data_ptr() for x in ins), *(x.data_ptr() for x in outs))
        self.eng.sync()
        return self._cut(*outs)

    def verify_queue(self, ks, idx, shuffled, proofs):
        B = len(idx)
        d_decks = self.dv.bytes(b"".join(self.w.gen[b % N_STMT]["deck"] for b in range(B)))
        d_sh, d_pf, d_idx, st = self.dv.bytes(b"".join(shuffled)), self.dv.bytes(b"".join(proofs)), self.dv.ints(idx), self.dv.status(B)
        self.dv.sync()
        self.t.verify_shuffle_batch_keyset_dev(ks, B, d_idx.data_ptr(), d_decks.data_ptr(), d_sh.data_ptr(), d_pf.data_ptr(), st.data_ptr())
        return (d_decks, d_sh, d_pf, d_idx), st

    def verify(self, ks, idx, shuffled, proofs):
        held, st = self.verify_queue(ks, idx, shuffled, proofs)
        self.eng.sync()
        return st.cpu().tolist()

    def update(self, ks, slots, keys, form):
        """-> status words, through the host form or the device form"""
        if form == "host":
            return ks.update(slots, b"".join(keys))
        d_keys, st = self.dv.bytes(b"".join(keys)), self.dv.status(len(slots))
        self.dv.sync()
        ks.update_dev(slots, d_keys.data_ptr(), st.data_ptr())
        self.eng.sync()
        return st.cpu().tolist()

    def empty_by_every_call(self, ks, cap):
        """a wholly empty set (slot 0's wire key is zero bytes too): every index, and the one past the set, through the seeded prover, the
        chain verifier (one table of one link per index) and the dealing calls by index gives MP_ERR_BAD_ARGUMENT for its item"""
        w, idx = self.w, list(range(cap + 1))
        B = len(idx)
        key = w.keys(0, 1)[0]
        d_decks, d_seeds = self.dv.bytes(w.gen[0]["deck"] * B), self.dv.bytes(bytes([9]) * (32 * B))
        od, op, st = self._outputs(B)
        d_idx = self.dv.ints(idx)
        self.dv.sync()
        self.t.shuffle_and_remask_batch_seeded_keyset_dev(ks, B, d_idx.data_ptr(), d_decks.data_ptr(), d_seeds.data_ptr(), od.data_ptr(),
                                                          op.data_ptr(), st.data_ptr())
        self.eng.sync()
        for i, v in zip(idx, st.cpu().tolist()):
            self.check(v == BAD_ARGUMENT, "empty set of %d: seeded proof by index %d: status %d", cap, i, v)
        shuffled, proof = w.proofs([(key, 0)])[0]
        words = self.t.verify_shuffle_chain_ragged_keyset(ks, [1] * B, idx, (w.gen[0]["deck"] + shuffled) * B, proof * B)
        for i, v in zip(idx, words):
            self.check(v == BAD_ARGUMENT, "empty set of %d: chain of the table on index %d: word %d", cap, i, v)
        one, seeds = (1).to_bytes(32, "little") * B, bytes([7]) * (32 * B)
        out, prf, ds = self.t.mask_batch_keyset(ks, 0, idx, key * B, one, seeds)
        for i, v in zip(idx, ds):
            self.check(v == BAD_ARGUMENT and not any(out) and not any(prf), "empty set of %d: card dealt by index %d: status %d", cap, i, v)
        vs = self.t.verify_mask_batch_keyset(ks, 0, idx, key * B, (key + key) * B, (key + key + one[:32]) * B)
        for i, v in zip(idx, vs):
            self.check(v == BAD_ARGUMENT, "empty set of %d: dealt card verified by index %d: word %d", cap, i, v)

    # ---- what a set serves
    def serves(self, tag, ks, holds, probe=None, keys_dev=False):
        """holds[s] = the key slot s must hold, or None for an empty slot.  One prove batch and one verify batch over the slots of `probe`
        (default: all) and the index one past the set.  2 (len(probe) + 1) + 1 checks, and with keys_dev one more per live slot probed:
        the bytes of mp_shuffle_and_remask_batch_keys_dev with the keys written out"""
        cap = len(holds)
        idx = list(range(cap) if probe is None else probe) + [cap]
        key_of = [holds[s] if s < cap else None for s in idx]
        spare = self.w.keys(0, 1)[0]
        want = self.w.proofs([(k if k is not None else spare, b % N_STMT) for b, k in enumerate(key_of)])
        st, d, p = self.prove(ks, idx)
        for b, s in enumerate(idx):
            if key_of[b] is None:
                self.check(st[b] == BAD_ARGUMENT, "%s: proof by index %d (no key there): status %d, expected MP_ERR_BAD_ARGUMENT", tag, s, st[b])
            else:
                self.check(st[b] == 0 and d[b] == want[b][0] and p[b] == want[b][1],
                           "%s: proof by index %d: status %d, deck %s, proof %s the oracle's under the slot's key", tag, s, st[b],
                           "is" if d[b] == want[b][0] else "IS NOT", "is" if p[b] == want[b][1] else "IS NOT")
        sv = self.verify(ks, idx, [x[0] for x in want], [x[1] for x in want])
        for b, s in enumerate(idx):
            exp = BAD_ARGUMENT if key_of[b] is None else 0
            self.check(sv[b] == exp, "%s: the oracle's proof verified by index %d: word %d, expected %d", tag, s, sv[b], exp)
        n_live = sum(1 for k in holds if k is not None)
        got = ks.live()
        self.check(got == n_live, "%s: mp_keyset_live says %d, %d slots hold a key", tag, got, n_live)
        if keys_dev:
            rows = [b for b, k in enumerate(key_of) if k is not None]
            if rows:
                # statement numbers must match those of the indexed batch: run the whole batch with the spare key in the other rows
                st2, d2, p2 = self.prove_keys([k if k is not None else spare for k in key_of])
                for b in rows:
                    self.check(st2[b] == 0 and d2[b] == d[b] and p2[b] == p[b],
                               "%s: proof by index %d differs from mp_shuffle_and_remask_batch_keys_dev with the key written out", tag, idx[b])


def empty_calls_count(cap):
    return 4 * (cap + 1)


def serves_count(cap, probe=None, live_probed=0):
    return 2 * ((cap if probe is None else probe) + 1) + 1 + live_probed


def _rig(args):
    return Rig(*args)


# ---- 1. empty sets --------------------------------------------------------------------------------------------------------------------
def run_empty(*args):
    """capacities 1 and 5: every index of an empty set gives MP_ERR_BAD_ARGUMENT; with slots 1 and 3 of the larger set filled, their proofs
    are the oracle's between the refused ones"""
    r = _rig(args)
    for cap in (1, 5):
        ks = r.t.keyset_empty(cap)
        r.check(r.t.lib.mp_keyset_size(ks.h) == cap, "an empty set of %d slots has size %d", cap, r.t.lib.mp_keyset_size(ks.h))
        r.serves("empty set of %d" % cap, ks, [None] * cap)
        r.empty_by_every_call(ks, cap)
        if cap == 5:
            keys = r.w.keys(10, 2)
            st = r.update(ks, [3, 1], keys, "host")
            r.check(st == [0, 0], "filling slots 3 and 1 of an empty set: status %s", st)
            r.serves("slots 1 and 3 filled", ks, [None, keys[1], None, keys[0], None], keys_dev=True)
        ks.close()
    return r.close()


def empty_count():
    return 1 + serves_count(1) + empty_calls_count(1) + 1 + serves_count(5) + empty_calls_count(5) + 1 + serves_count(5, live_probed=2)


# ---- 2. fill and use ------------------------------------------------------------------------------------------------------------------
def run_fill(count, form, *args):
    """an empty set of count + 1 slots takes `count` keys in one update, slots in descending order, slot 0 stays empty"""
    r = _rig(args)
    cap = count + 1
    ks = r.t.keyset_empty(cap)
    keys = r.w.keys(20, count)
    slots = [cap - 1 - i for i in range(count)]
    st = r.update(ks, slots, keys, form)
    for i in range(count):
        r.check(st[i] == 0, "update of %d (%s form): key %d has status %d", count, form, i, st[i])
    holds = [None] * cap
    for s, k in zip(slots, keys):
        holds[s] = k
    r.serves("after an update of %d (%s form)" % (count, form), ks, holds, keys_dev=True)
    ks.close()
    return r.close()


def fill_count(count):
    return count + serves_count(count + 1, live_probed=count)


# ---- 3. replace -----------------------------------------------------------------------------------------------------------------------
def run_replace(created, form, *args):
    """five slots under keys A; slot s goes to key B for the first, the last and the middle slot in turn: the next proof by index s is
    the oracle's under B, A's proof no longer verifies by index s (the word of mp_verify_shuffle_batch_keys under B), and the other slots
    still serve their own keys"""
    r = _rig(args)
    cap = 5
    A, Bk = r.w.keys(30, cap), r.w.keys(40, cap)
    if created:
        ks = r.t.keyset(b"".join(A))
    else:
        ks = r.t.keyset_empty(cap)
        st = r.update(ks, list(range(cap)), A, form)
        r.check(st == [0] * cap, "filling the set: status %s", st)
    holds = list(A)
    r.serves("under the first keys", ks, holds)
    for s in (0, cap - 1, 2):
        st = r.update(ks, [s], [Bk[s]], form)
        r.check(st == [0], "replacing slot %d: status %s", s, st)
        old = r.w.proofs([(A[s], 0)])[0]
        holds[s] = Bk[s]
        r.serves("slot %d replaced" % s, ks, holds)
        g = r.w.gen[0]
        want = r.t.verify_shuffle_batch_keys(Bk[s], g["deck"], old[0], old[1])[0]
        got = r.verify(ks, [s], [old[0]], [old[1]])[0]
        r.check(got == want and got > 0, "the proof made under the old key of slot %d, verified by index: word %d, "
                "mp_verify_shuffle_batch_keys under the new key says %d", s, got, want)
    ks.close()
    return r.close()


def replace_count(created):
    return (0 if created else 1) + serves_count(5) + 3 * (1 + serves_count(5) + 1)


# ---- 4. refused keys ------------------------------------------------------------------------------------------------------------------
def _scattered(cap):
    """a permutation of the slots, so that a key's position in the update is not its slot"""
    assert cap % 3
    return [(3 * i + 1) % cap for i in range(cap)]


def run_refused(name, at, form, *args):
    """65 live slots take 65 new keys in one update whose key `at` has the defect: its word is MP_ERR_BAD_ENCODING, its slot is empty
    although it held a key, the other 64 are live under their new keys"""
    r = _rig(args)
    cap = REFUSED_SET
    old, new = r.w.keys(100, cap), r.w.keys(200, cap)
    ks = r.t.keyset(b"".join(old))
    if name == "outside the subgroup":
        r.t.set_subgroup_check(False)      # the set tests the subgroup whatever this says
    slots = _scattered(cap)
    sent = list(new)
    sent[at] = r.w.defect(name, new[at])
    st = r.update(ks, slots, sent, form)
    for i in range(cap):
        exp = BAD_ENCODING if i == at else 0
        r.check(st[i] == exp, "%s at position %d of %d: key %d has status %d, expected %d", name, at, cap, i, st[i], exp)
    holds = [None] * cap
    for i, s in enumerate(slots):
        holds[s] = None if i == at else new[i]
    r.serves("%s at position %d" % (name, at), ks, holds)
    ks.close()
    return r.close()


def refused_count():
    return REFUSED_SET + serves_count(REFUSED_SET)


def run_near_miss(form, *args):
    """the valid encoding next to the refused ones enters the set, and the slot serves the oracle's bytes under it"""
    r = _rig(args)
    keys = r.w.keys(50, 3)
    ks = r.t.keyset(b"".join(keys))
    if r.w.c.cofactor:
        r.t.set_subgroup_check(False)
    near = r.w.near_miss()
    st = r.update(ks, [1], [near], form)
    r.check(st == [0], "the near miss: status %s", st)
    r.serves("the near miss in slot 1", ks, [keys[0], near, keys[2]])
    ks.close()
    return r.close()


def near_miss_count():
    return 1 + serves_count(3)


# ---- 5. malformed slots arrays --------------------------------------------------------------------------------------------------------
BAD_SLOTS = (("a slot twice", [1, 3, 1]), ("the capacity", [0, 5]), ("0xFFFFFFFF", [0xFFFFFFFF]), ("count == 0", []))


def run_bad_slots(*args):
    """the three calls refuse the array as a whole: MP_ERR_BAD_ARGUMENT, a sentinel-filled status / d_status untouched, every slot
    serves what it served before"""
    r = _rig(args)
    cap = 5
    keys, other = r.w.keys(60, cap), r.w.keys(70, 3)
    ks = r.t.keyset(b"".join(keys))
    lib = r.t.lib
    for name, slots in BAD_SLOTS:
        arr = (ctypes.c_uint32 * max(len(slots), 1))(*slots)
        raw = (ctypes.c_uint8 * (3 * r.w.c.pb)).from_buffer_copy(b"".join(other))
        st = (ctypes.c_int32 * 3)(SENTINEL, SENTINEL, SENTINEL)
        rc = lib.mp_keyset_update(ks.h, len(slots), arr, raw, st)
        r.check(rc == BAD_ARGUMENT and list(st) == [SENTINEL] * 3, "mp_keyset_update with %s: returned %d, status %s", name, rc, list(st))
        d_keys, d_st = r.dv.bytes(b"".join(other)), r.dv.status(3)
        r.dv.sync()
        rc = lib.mp_keyset_update_dev(ks.h, len(slots), arr, d_keys.data_ptr(), d_st.data_ptr())
        r.eng.sync()
        r.check(rc == BAD_ARGUMENT and d_st.cpu().tolist() == [SENTINEL] * 3, "mp_keyset_update_dev with %s: returned %d, d_status %s",
                name, rc, d_st.cpu().tolist())
        rc = lib.mp_keyset_clear(ks.h, len(slots), arr)
        r.check(rc == BAD_ARGUMENT, "mp_keyset_clear with %s: returned %d", name, rc)
        r.serves("after the calls with %s" % name, ks, keys)
    ks.close()
    return r.close()


def bad_slots_count():
    return len(BAD_SLOTS) * (3 + serves_count(5))


# ---- 6. clear -------------------------------------------------------------------------------------------------------------------------
def run_clear(form, *args):
    """first and last slot cleared, then the middle one, then the first filled again: after each step the cleared slots are empty and
    their neighbours serve their keys"""
    r = _rig(args)
    cap = 5
    keys = r.w.keys(80, cap)
    ks = r.t.keyset(b"".join(keys))
    holds = list(keys)
    for slots in ([cap - 1, 0], [2]):
        ks.clear(slots)
        for s in slots:
            holds[s] = None
        r.serves("slots %s cleared" % slots, ks, holds)
    again = r.w.keys(90, 1)[0]
    st = r.update(ks, [0], [again], form)
    r.check(st == [0], "filling a cleared slot: status %s", st)
    holds[0] = again
    r.serves("slot 0 filled again", ks, holds)
    ks.clear([1, 3, 0])
    r.serves("every slot cleared", ks, [None] * cap)
    ks.close()
    return r.close()


def clear_count():
    return 4 * serves_count(5) + 1


# ---- 7. ordering (what only a GPU's streams can show) ---------------------------------------------------------------------------------
def run_ordering(*args):
    """prove by index s (queued), mp_keyset_update_dev of s from A to B, prove by index s again, ONE mp_sync: the first bytes are the
    oracle's under A, the second under B.  Then with mp_set_pipeline(t, 1): a verify call of A's proofs by index, the update, mp_sync:
    every word is 0"""
    r = _rig(args)
    cap, s, B = 3, 1, 8
    A, Bk = r.w.keys(110, cap), r.w.keys(120, cap)
    ks = r.t.keyset(b"".join(A))
    d_keys, d_st = r.dv.bytes(Bk[s]), r.dv.status(1)
    r.dv.sync()
    first = r.prove_queue(ks, [s] * B)
    ks.update_dev([s], d_keys.data_ptr(), d_st.data_ptr())
    second = r.prove_queue(ks, [s] * B)
    r.eng.sync()
    r.check(d_st.cpu().tolist() == [0], "the queued update: d_status %s", d_st.cpu().tolist())
    for tag, held, key in (("before", first, A[s]), ("after", second, Bk[s])):
        st, d, p = r._cut(*held[2])
        want = r.w.proofs([(key, b % N_STMT) for b in range(B)])
        for b in range(B):
            r.check(st[b] == 0 and d[b] == want[b][0] and p[b] == want[b][1],
                    "proof %d queued %s the update: status %d, not the oracle's bytes under the key the slot held then", b, tag, st[b])
    # pipelined verification: the screening verdict of the call is still unexamined when the update comes in
    holds = [A[0], Bk[s], A[2]]
    idx = [b % cap for b in range(B)]
    want = r.w.proofs([(holds[i], b % N_STMT) for b, i in enumerate(idx)])
    r.t.set_pipeline(1)
    held, sv = r.verify_queue(ks, idx, [x[0] for x in want], [x[1] for x in want])
    d_keys2, d_st2 = r.dv.bytes(b"".join(r.w.keys(130, cap))), r.dv.status(cap)
    r.dv.sync()
    ks.update_dev(list(range(cap)), d_keys2.data_ptr(), d_st2.data_ptr())
    r.eng.sync()
    r.t.set_pipeline(0)
    words = sv.cpu().tolist()
    for b in range(B):
        r.check(words[b] == 0, "pipelined verify call issued before the update, proof %d: word %d", b, words[b])
    r.check(d_st2.cpu().tolist() == [0] * cap, "the update behind the pipelined call: d_status %s", d_st2.cpu().tolist())
    ks.close()
    return r.close()


def ordering_count():
    return 1 + 2 * 8 + 8 + 1


# ---- 8. one key past a build slice ----------------------------------------------------------------------------------------------------
def run_slice(sl, form, *args):
    """an update of sl + 1 keys, sl = the build slice of the library under test (engine_core.hpp KEYSET_UPDATE_SLICE, or what the emulator's
    make variable lowered it to): the first, the last of the slice and the first of the next (which is the last) serve the oracle's bytes"""
    r = _rig(args)
    cap = sl + 1
    keys = r.w.keys(1000, cap)
    ks = r.t.keyset_empty(cap)
    slots = _scattered(cap) if cap % 3 else [cap - 1 - i for i in range(cap)]
    st = r.update(ks, slots, keys, form)
    r.check(st == [0] * cap, "an update of %d keys: %d status words are not 0", cap, sum(1 for v in st if v))
    holds = [None] * cap
    for s, k in zip(slots, keys):
        holds[s] = k
    at = sorted(set([slots[0], slots[sl - 1], slots[sl], slots[cap - 1]]))
    r.check(len(at) == 3, "positions 0, slice - 1 and slice are three slots")
    r.serves("slice + 1 = %d keys" % cap, ks, holds, probe=at)
    ks.close()
    return r.close()


def slice_count():
    return 2 + serves_count(0, probe=3)


# ---- 10. chains by index --------------------------------------------------------------------------------------------------------------
CHAIN_LINKS = (1, 2, 3, 7)               # 7 = 4 + 2 + 1: three pieces in the binary mode
CHAIN_MODES = (0, 1)                     # MP_CHAIN_PIECES_WHOLE, MP_CHAIN_PIECES_BINARY


def _chains(w, keys):
    """honest chains of CHAIN_LINKS links, table k under keys[k]: the oracle's decks and proofs, table-major"""
    decks, proofs = [], []
    for k, L in enumerate(CHAIN_LINKS):
        d = w.gen[k % N_STMT]["deck"]
        decks.append(d)
        for j in range(L):
            g = w.gen[(k + j) % N_STMT]
            d, p = w.co.shuffle_and_remask(w.curve, w.m, w.n, w.params, keys[k], d, g["rho"], g["perm"], g["prover_seed"])
            decks.append(d)
            proofs.append(p)
    return decks, proofs


def run_chains(modes, which, *args):
    """modes: the piece modes to run; which: the numbers of the three inputs below to run (all of them on the first curve, the last one,
    which holds honest tables too, on the others).  Four tables of 1, 2, 3 and 7 links, each on its own slot of a set of six (slot 4 empty): the words of the host and the _dev form,
    in both piece modes, are those of mp_verify_shuffle_chain_ragged with the key repeated per link -- for honest chains, with one link's
    proof replaced by its neighbour's, and with one table on an index past the set and one on the empty slot, whose links all read
    MP_ERR_BAD_ARGUMENT while the other tables' words stay"""
    r = _rig(args)
    w, links, T = r.w, list(CHAIN_LINKS), len(CHAIN_LINKS)
    total = sum(links)
    keys = w.keys(300, T)
    slot_of = [5, 0, 3, 2]
    holds = [None] * 6
    for k, s in enumerate(slot_of):
        holds[s] = keys[k]
    ks = r.t.keyset_empty(6)
    st = ks.update(slot_of, b"".join(keys))
    r.check(st == [0] * T, "filling the set: status %s", st)
    decks, proofs = _chains(w, keys)
    off = [sum(links[:k]) for k in range(T + 1)]
    per_link = b"".join(keys[k] for k in range(T) for _ in range(links[k]))
    tampered = list(proofs)
    tampered[off[3] + 4] = proofs[off[3] + 5]            # link 4 of the 7-link table: the first link of its second piece
    cases = (("honest chains", proofs, slot_of, ()),
             ("one link's proof replaced", tampered, slot_of, ()),
             ("table 1 past the set, table 2 on the empty slot", proofs, [5, 6, 4, 2], (1, 2)))
    for mode in modes:
        r.t.set_chain_pieces(mode)
        for name, pf, idx, refused in [cases[i] for i in which]:
            want = r.t.verify_shuffle_chain_ragged(links, b"".join(decks), b"".join(pf), keys=per_link)
            if name == "honest chains" and any(want):
                r.fails.append("%s: mp_verify_shuffle_chain_ragged refuses the oracle's chains: %s" % (r.curve, want))
            if pf is tampered and [i for i, v in enumerate(want) if v] != [off[3] + 4]:
                r.fails.append("%s: the tampered link is not the one word that moved: %s" % (r.curve, want))
            for k in refused:
                want[off[k]:off[k + 1]] = [BAD_ARGUMENT] * links[k]
            got_host = r.t.verify_shuffle_chain_ragged_keyset(ks, links, idx, b"".join(decks), b"".join(pf))
            d_decks, d_pf, d_idx, d_st = r.dv.bytes(b"".join(decks)), r.dv.bytes(b"".join(pf)), r.dv.ints(idx), r.dv.status(total)
            r.dv.sync()
            r.t.verify_shuffle_chain_ragged_keyset_dev(ks, links, d_idx.data_ptr(), d_decks.data_ptr(), d_pf.data_ptr(), d_st.data_ptr())
            r.eng.sync()
            for form, got in (("host", got_host), ("_dev", d_st.cpu().tolist())):
                for i in range(total):
                    r.check(got[i] == want[i], "%s, mode %d, %s form: link row %d has word %d, expected %d", name, mode, form, i, got[i], want[i])
    r.t.set_chain_pieces(1)
    ks.close()
    return r.close()


def chains_count(modes, which):
    return 1 + len(modes) * len(which) * 2 * sum(CHAIN_LINKS)


# ---- 11. the seeded prover by index ---------------------------------------------------------------------------------------------------
def run_seeded(*args):
    """mp_shuffle_and_remask_batch_seeded_keyset_dev: the bytes of mp_shuffle_and_remask_batch_seeded_dev with the keys written out, and
    MP_ERR_BAD_ARGUMENT for the proofs on an empty slot and past the set; the first proof is also the oracle's under the sampled witness"""
    r = _rig(args)
    w = r.w
    keys = w.keys(400, 3)
    ks = r.t.keyset_empty(4)
    st = ks.update([3, 0, 1], b"".join(keys))
    r.check(st == [0, 0, 0], "filling the set: status %s", st)
    holds = [keys[1], keys[2], None, keys[0]]
    idx = [0, 3, 2, 1, 4, 3]
    B = len(idx)
    spare = keys[0]
    written = [holds[i] if i < 4 and holds[i] is not None else spare for i in idx]
    seeds = b"".join(bytes([b + 1]) * 32 for b in range(B))
    decks = b"".join(w.gen[b % N_STMT]["deck"] for b in range(B))
    out = []
    for by_index in (False, True):
        d_decks, d_seeds = r.dv.bytes(decks), r.dv.bytes(seeds)
        od, op, ds = r._outputs(B)
        d_perm, d_rho = r.dv.ints([0] * (B * w.N)), r.dv.bytes(bytes(B * w.N * 32))
        d_k = r.dv.ints(idx) if by_index else r.dv.bytes(b"".join(written))
        r.dv.sync()
        if by_index:
            r.t.shuffle_and_remask_batch_seeded_keyset_dev(ks, B, d_k.data_ptr(), d_decks.data_ptr(), d_seeds.data_ptr(), od.data_ptr(),
                                                           op.data_ptr(), ds.data_ptr(), d_perm.data_ptr(), d_rho.data_ptr())
        else:
            r.t.shuffle_and_remask_batch_seeded_dev(B, d_k.data_ptr(), d_decks.data_ptr(), d_seeds.data_ptr(), od.data_ptr(), op.data_ptr(),
                                                    ds.data_ptr(), d_perm.data_ptr(), d_rho.data_ptr())
        r.eng.sync()
        out.append(r._cut(od, op, ds) + (d_perm.cpu().tolist(), bytes(d_rho.cpu().numpy().tobytes())))
    (st0, d0, p0, perm0, rho0), (st1, d1, p1, perm1, rho1) = out
    for b, i in enumerate(idx):
        if i >= 4 or holds[i] is None:
            r.check(st1[b] == BAD_ARGUMENT, "seeded proof %d by index %d (no key there): status %d", b, i, st1[b])
        else:
            r.check(st0[b] == 0 and st1[b] == 0 and d1[b] == d0[b] and p1[b] == p0[b],
                    "seeded proof %d by index %d differs from mp_shuffle_and_remask_batch_seeded_dev with the key written out", b, i)
    r.check(perm1 == perm0 and rho1 == rho0, "the sampled witnesses of the two calls differ")
    N = w.N
    want = w.co.shuffle_and_remask(w.curve, w.m, w.n, w.params, holds[idx[0]], w.gen[0]["deck"], rho1[:32 * N], perm1[:N], seeds[:32])
    r.check((d1[0], p1[0]) == tuple(want), "seeded proof 0 is not the oracle's under the slot's key and the sampled witness")
    ks.close()
    return r.close()


def seeded_count():
    return 1 + 6 + 1 + 1


# ---- 12. dealing by index -------------------------------------------------------------------------------------------------------------
import hashlib  # noqa: E402

import deal_cases as dl  # noqa: E402
import digit_cases as dg  # noqa: E402

DEAL_SHAPES = dl.SHAPES                  # (cards, keys): C = 1, 63, 64, 65, 257
SCREEN_GROUP = 8


def digit_edge_factors(q):
    """factors on the edges of the 8-bit fixed-base digits (tests/digit_cases.py): 0, 1, q - 1, only the top window set, every window
    255, and the 8-bit family with one boundary digit per window, thinned"""
    nwin = dg.windows(q, dg.KIND_FIXED, 8)
    top = 1 << (8 * (nwin - 1))
    all255 = sum(255 << (8 * w) for w in range(nwin)) % q
    fam = dict(dg.families(q, dg.KIND_FIXED, 8))["one boundary digit per window"]
    vals = [0, 1, q - 1, top, all255] + list(fam[::max(1, len(fam) // 24)])
    assert top < q and all(0 <= v < q for v in vals)
    return vals


def _slot_of(j):
    """key j of a dealing batch sits in slot 0 (j = 0) or j + 1: slot 1 stays empty, the last slot holds the last key"""
    return 0 if j == 0 else j + 1


def _deal_set(c, b):
    ks = c.t.keyset_empty(b.K + 1)
    st = ks.update([_slot_of(j) for j in range(b.K)], b"".join(b.keys))
    assert st == [0] * b.K, st
    return ks


def _with_digit_edges(c, b):
    """the generic lanes of the batch take the digit-edge factors in turn; their masked cards and proofs are the oracle's again"""
    vals = digit_edge_factors(c.q)
    k = 0
    for i in range(b.C):
        if b.kinds[i] != "generic":
            continue
        b.factors[i] = vals[k % len(vals)]
        k += 1
        pk = b.keys[b.key_index[i]]
        a0, a1 = c.mul(b.factors[i], c.G), c.mul(b.factors[i], pk)
        b.masked[i] = (c.add(b.inputs[i][0], a0), c.add(b.inputs[i][1], a1))
        b.proofs[i] = c.co.sigma_prove(c.curve, 2, c.G + pk, a0 + a1, c.sc(b.factors[i]), dl.FS[b.kind], b.seeds[i])
    return k


def run_deal(shape_list, eng, coracle, curve, torch, device):
    """mp_mask_batch_keyset / mp_verify_mask_batch_keyset[_dev]: per shape and kind, masked cards and proofs are the oracle's and the bytes
    of mp_mask_batch with the keys written out; the verifier's words are 0 in both forms; with card 0 on the empty slot and the last
    card past the set those two read MP_ERR_BAD_ARGUMENT (zero bytes from the prover) and the others do not move"""
    c = dl.Ctx(eng, coracle, curve)
    dv = sec._Dev(torch, device)
    fails, checks = [], 0
    cb, psz = 2 * c.pb, 2 * c.pb + 32
    for C, K in shape_list:
        for kind in dl.KINDS:
            b = dl.Deal(c, kind, C, K)
            _with_digit_edges(c, b)
            ks = _deal_set(c, b)
            tag = "%s %s by index (%d, %d)" % (curve, dl.KIND_NAME[kind], C, K)
            idx = [_slot_of(j) for j in b.key_index]
            fbytes, sbytes = b"".join(c.sc(r) for r in b.factors), b"".join(b.seeds)
            out, prf, st = c.t.mask_batch_keyset(ks, kind, idx, b.input_bytes(), fbytes, sbytes)
            out2, prf2, st2 = b.prove(c.t)
            dl._diff(fails, tag + " prove", st, [0] * C, b.kinds)
            for i in range(C):
                if out[i * cb:(i + 1) * cb] != b.masked[i][0] + b.masked[i][1] or prf[i * psz:(i + 1) * psz] != b.proofs[i]:
                    fails.append("%s card %d (%s, factor %#x): not the oracle's bytes" % (tag, i, b.kinds[i], b.factors[i]))
            if (out, prf, st) != (out2, prf2, st2):
                fails.append("%s: differs from mp_mask_batch with the keys written out" % tag)
            dl._diff(fails, tag + " verify", c.t.verify_mask_batch_keyset(ks, kind, idx, b.input_bytes(), b.masked_bytes(), b"".join(b.proofs)),
                     [0] * C, b.kinds)
            d = [dv.ints(idx), dv.bytes(b.input_bytes()), dv.bytes(b.masked_bytes()), dv.bytes(b"".join(b.proofs))]
            dst = dv.status(C)
            dv.sync()
            c.t.verify_mask_batch_keyset_dev(ks, kind, C, *(x.data_ptr() for x in d), dst.data_ptr())
            eng.sync()
            dl._diff(fails, tag + " verify, device pointers", dst.cpu().tolist(), [0] * C, b.kinds)
            checks += 5 * C
            # no key there: the empty slot and the index one past the set
            bad = list(idx)
            bad[0], bad[-1] = (1, K + 1) if C > 1 else (K + 1, K + 1)
            want = [dl.BAD_ARGUMENT if i in (0, C - 1) else 0 for i in range(C)]
            out3, prf3, st3 = c.t.mask_batch_keyset(ks, kind, bad, b.input_bytes(), fbytes, sbytes)
            dl._diff(fails, tag + " prove, two cards without a key", st3, want)
            for i in range(C):
                wo, wp = (out[i * cb:(i + 1) * cb], prf[i * psz:(i + 1) * psz]) if want[i] == 0 else (bytes(cb), bytes(psz))
                if out3[i * cb:(i + 1) * cb] != wo or prf3[i * psz:(i + 1) * psz] != wp:
                    fails.append("%s card %d beside cards without a key: output moved" % (tag, i))
            dl._diff(fails, tag + " verify, two cards without a key",
                     c.t.verify_mask_batch_keyset(ks, kind, bad, b.input_bytes(), b.masked_bytes(), b"".join(b.proofs)), want)
            checks += 3 * C
            ks.close()
    c.close()
    return fails, checks


def deal_count(shape_list):
    return sum(2 * 8 * C for C, _ in shape_list)


def run_deal_defects(eng, coracle, curve):
    """the verifier by index with one defect per lane from tests/deal_cases.py defect_list (those that a key in a set can have: a bad key
    cannot enter one), every third lane honest: the words of mp_verify_mask_batch with the keys written out, which are the oracle's
    where it judges -- and the same words under mp_set_sigma_screen"""
    c = dl.Ctx(eng, coracle, curve)
    fails, checks = [], 0
    for kind in dl.KINDS:
        probe = dl.Deal(c, kind, 1, 3, edges=False)
        defects_ = [x for x in dl.defect_list(c, probe) if not x[0].startswith("key ")]
        C = 3 * len(defects_) + 2
        b = dl.Deal(c, kind, C, 3, salt=11, edges=False)
        d = dl._inputs(b)
        want, names = [None] * C, ["honest"] * C
        for k, (name, code, edit, lanes) in enumerate([x for x in dl.defect_list(c, b) if not x[0].startswith("key ")]):
            edit(d, 3 * k + 1)
            for j in range(lanes):
                want[3 * k + 1 + j], names[3 * k + 1 + j] = code, name
        by_key = [len(d["keys"]) if k == -1 else k for k in d["key_index"]]
        by_slot = [b.K + 1 if k == -1 else (k if k > 0xFFFF else _slot_of(k)) for k in d["key_index"]]
        d["key_index"] = by_key
        dl._oracle_words(c, b, d, want)
        keyed = b.verify(c.t, keys=d["keys"], key_index=by_key, inputs=d["inputs"], masked=d["masked"], proofs=d["proofs"])
        tag = "%s %s defects by index" % (curve, dl.KIND_NAME[kind])
        if keyed != want or not (any(v == dl.CHAUM_PEDERSEN for v in want) and any(v == dl.BAD_ENCODING for v in want)
                                 and any(v == dl.BAD_ARGUMENT for v in want) and want[::3] == [0] * len(want[::3])):
            fails.append("%s: the case list does not hold: oracle %s, mp_verify_mask_batch %s" % (tag, want, keyed))
        ks = _deal_set(c, b)
        args = (ks, kind, by_slot, b.input_bytes(d["inputs"]), b.masked_bytes(d["masked"]), b"".join(d["proofs"]))
        dl._diff(fails, tag, c.t.verify_mask_batch_keyset(*args), want, names)
        c.t.set_sigma_screen(SCREEN_GROUP, 1)
        dl._diff(fails, tag + ", screened", c.t.verify_mask_batch_keyset(*args), want, names)
        c.t.set_sigma_screen(0, 0)
        checks += 2 * C
        ks.close()
    c.close()
    return fails, checks


def deal_defects_count(curve):
    return 2 * 2 * (3 * 17 + 2)


# ---- 9. seating into a set ------------------------------------------------------------------------------------------------------------
SEAT_COUNTS = (1, 2, 3, 10, 2)           # the last table: keys pk and -pk


def run_seat(eng, coracle, curve, torch, device):
    """tables of 1, 2, 3 and 10 seats and one whose two keys cancel, a wrong response at the middle seat of the 3-seat table: words and
    out_keys are those of mp_aggregate_keys_ragged_batch; slot_status is 0, the table's word, or MP_ERR_BAD_ENCODING for the identity;
    a shuffle by index under each seated slot is the oracle's under the oracle's sum of the keys, the two other slots are empty though
    they held keys; with out_keys == NULL the same slots result"""
    c = dl.Ctx(eng, coracle, curve)
    dv = sec._Dev(torch, device)
    fails, checks, q = [], 0, c.q
    sks = []
    for k, n in enumerate(SEAT_COUNTS):
        row = [3 + 1000 * k + 7 * j for j in range(n)]
        sks.append([row[0], q - row[0]] if k == 4 else row)
    flat = [x for row in sks for x in row]
    pk = [c.mul(x, c.G) for x in flat]
    raw = [po.KEY_OWN_RNG_SEED + b"seat %d" % l for l in range(len(flat))]
    proofs = [coracle.sigma_prove(curve, 1, c.G, pk[l], c.sc(flat[l]), raw[l], hashlib.blake2s(b"seat into a set %d" % l).digest())
              for l in range(len(flat))]
    bad_lane = 1 + 2 + 1
    proofs[bad_lane] = proofs[bad_lane][:c.pb] + c.sc((int.from_bytes(proofs[bad_lane][c.pb:], "little") + 1) % q)
    fs = b"".join(c.fs_digest(r) for r in raw)
    counts, T = list(SEAT_COUNTS), len(SEAT_COUNTS)
    want_keys, want_ps, want_ts = c.t.aggregate_keys_ragged_batch(counts, b"".join(pk), b"".join(proofs), fs)
    sums = [coracle.msm(curve, c.sc(1) * n, b"".join(pk[sum(counts[:k]):sum(counts[:k]) + n])) for k, n in enumerate(counts)]
    if want_ts != [0, 0, dl.SCHNORR, 0, 0] or sums[4] != c.inf or [want_keys[k * c.pb:(k + 1) * c.pb] for k in (0, 1, 3)] != [sums[k] for k in (0, 1, 3)]:
        fails.append("%s: the case list does not hold: table words %s" % (curve, want_ts))
    want_ss = [0, 0, dl.SCHNORR, 0, BAD_ENCODING]
    slots = [5, 0, 2, 3, 1]
    g = coracle.gen_inputs(curve, dl.M_, dl.N_, 7700)
    old = [c.mul(50 + s, c.G) for s in range(6)]
    for want_out in (True, False):
        ks = c.t.keyset(b"".join(old))                     # every slot holds a key before
        got_keys, ps, ts, ss = ks.seat(counts, slots, b"".join(pk), b"".join(proofs), fs, want_keys=want_out)
        tag = "%s seating into a set%s" % (curve, "" if want_out else ", out_keys == NULL")
        for name, got, want in (("player words", ps, want_ps), ("table words", ts, want_ts), ("slot words", ss, want_ss)):
            if got != want:
                fails.append("%s: %s %s, expected %s" % (tag, name, got, want))
        if want_out and got_keys != want_keys:
            fails.append("%s: out_keys differ from mp_aggregate_keys_ragged_batch" % tag)
        holds = list(old)
        for k, s in enumerate(slots):
            holds[s] = sums[k] if want_ss[k] == 0 else None
        if ks.live() != 4:
            fails.append("%s: %d slots are live, expected 4" % (tag, ks.live()))
        idx = list(range(6)) + [6]
        B = len(idx)
        ins = (dv.bytes(g["deck"] * B), dv.bytes(g["rho"] * B), dv.ints(list(g["perm"]) * B), dv.bytes(g["prover_seed"] * B))
        dsz, psz = len(g["deck"]), coracle.proof_size(dl.M_, dl.N_, curve)
        od, op, st, d_idx = dv.bytes(bytes(B * dsz)), dv.bytes(bytes(B * psz)), dv.status(B), dv.ints(idx)
        dv.sync()
        c.t.shuffle_and_remask_batch_keyset_dev(ks, B, d_idx.data_ptr(), *(x.data_ptr() for x in ins), od.data_ptr(), op.data_ptr(), st.data_ptr())
        eng.sync()
        words, D, P = st.cpu().tolist(), bytes(od.cpu().numpy().tobytes()), bytes(op.cpu().numpy().tobytes())
        for b_, s in enumerate(idx):
            key = holds[s] if s < 6 else None
            if key is None:
                ok = words[b_] == BAD_ARGUMENT
            else:
                wd_, wp_ = coracle.shuffle_and_remask(curve, dl.M_, dl.N_, c.params, key, g["deck"], g["rho"], g["perm"], g["prover_seed"])
                ok = words[b_] == 0 and D[b_ * dsz:(b_ + 1) * dsz] == wd_ and P[b_ * psz:(b_ + 1) * psz] == wp_
            if not ok:
                fails.append("%s: shuffle by index %d: status %d, %s" % (tag, s, words[b_], "no key there" if key is None else "not the oracle's bytes"))
        checks += len(want_ps) + 2 * T + (1 if want_out else 0) + 1 + B
        ks.close()
    c.close()
    return fails, checks


def seat_count():
    return 2 * (sum(SEAT_COUNTS) + 2 * len(SEAT_COUNTS) + 1 + 7) + 1
