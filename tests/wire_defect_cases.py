"""Cases, self-checks and runners for MALFORMED WIRE INPUTS to the shuffle calls: every deck, shuffled deck, proof, masking factor,
permutation and per-proof key arrives as bytes from another player, and a status word of 0 for something that is not a canonical,
on-curve, in-subgroup encoding is the worst failure the library can have.  Shared by tests/test_wire_defect_emu.py (the kernel bodies
under the development emulator, CPU) and tests/test_gpu_wire_defect.py (the gfx950 build) -- same cases, same expectations.

Family A (run_verifier_positions, run_verifier_keys): a defect at every one of the 11m + 8 points and 5n + 9 scalars of a proof, at
every point of both decks and in the per-proof key.  Family B (run_strategies, run_chain, run_validated): the same words under merged
and per-equation verification, group equations with and without refinement, the pipelined lane, chains and mp_set_validated.
Family C (run_prover, run_prover_lone_lane, run_prover_keys): masking factors, deck points, permutations and keys of the prover, on
both permutation checks (k_prove_init_w, k_prove_init).

Where the expectations come from: every malformed copy is shown to the C++ oracle BEFORE the device sees it, and the oracle must
answer -1 (-2 for a non-permutation) -- a case for which it says otherwise is reported as a failure of the case list.  The one
exception are points outside the prime-order subgroup of BLS12-377, which the oracle (it only tests the curve equation) accepts: their
expectation is MP_ERR_BAD_ENCODING by include/mpshuffle.h, and the self-check asserts in Python integers that the point is on the
curve and that [q]P != O.  Near misses (scalar q - 1, the largest x < p that gives a curve point, the all-zero infinity encoding, a
well-formed but wrong element) are VALID encodings: the device's word must be the oracle's, which must be >= 0.  Honest lanes and
well-formed tampered lanes sit between the malformed ones in every batch; their words are the oracle's, and the prover's output for them
is the oracle's bytes.  Output bytes of refused prover lanes are not asserted.

Every run_* function returns (failure messages, number of checks made); the tests assert that the list is empty and that the number is
the one the *_count function next to the runner computes from m, n and the curve alone -- a case list that shrinks fails the test."""
import deal_cases as dc
import fs_cases as fc
import mp_oracle as po
import shuffle_edge_cases as sec
import trait_cases as tc

BAD_ENCODING, BAD_PERMUTATION, INTERNAL = -1, -2, -5       # include/mpshuffle.h
VERIFIER_SHAPES = [("stark", 2, 3), ("bn254", 3, 2), ("secp256k1", 2, 3), ("bls12_377", 2, 3)]
STRATEGY_SHAPES = [("stark", 2, 3), ("bls12_377", 2, 3)]
PROVER_SHAPES = [("stark", 2, 3), ("stark", 2, 32), ("stark", 5, 13), ("stark", 2, 65), ("bls12_377", 2, 3)]   # N = 6, 64, 65, 130, 6
GROUP_L = (3, 65)
LONE_LANE_BATCH = 32769                                    # one proof past engine_base.hpp PROVE_INIT_WAVE_MAX: k_prove_init
MODES = ((0, 1), (0, 4), (8192, 0))                        # (latency batch, transcript lanes): the screened plans under both transcript
#                                                            kernels, and the small-batch plan, which keeps the raw wire words (W)
SUBGROUP_KINDS = ("low-order point", "point before cofactor clearing", "subgroup point + low-order point")


class Pts(tc.Ctx):
    """trait_cases.Ctx for its byte-level point helpers (off_curve, xy, neg), without its table: no engine is needed to build a case"""

    def __init__(self, coracle, curve):
        self.co, self.curve, self.cv = coracle, curve, po.CURVES[curve]
        self.q, self.p, self.pb = self.cv.q, self.cv.p, coracle.point_size(curve)
        self.fb = self.pb // 2
        self.inf = bytes(self.pb)
        self.cofactor = curve in po.COFACTOR

    def x_is_p(self, P):
        return dc._noncanonical(self, P)

    def y_past_p(self, P):
        """y := p + y, or y := p where that does not fit the field's bytes"""
        y = self.xy(P)[1] + self.p
        return P[:self.fb] + (y if y < 1 << (8 * self.fb) else self.p).to_bytes(self.fb, "little")

    def top_bit(self):
        """only the bit above the modulus's top bit set, or None where the field's bytes have no such bit (secp256k1)"""
        v = 1 << self.p.bit_length()
        return v.to_bytes(self.fb, "little") if v < 1 << (8 * self.fb) else None

    def scalar_bits(self):
        """2^BITS of the scalar field, or None where 32 bytes have no such bit (secp256k1)"""
        return 1 << self.q.bit_length() if self.q.bit_length() < 256 else None

    def largest_x(self):
        """the curve point with the largest x < p (x = p - 1 where that gives one), in canonical bytes"""
        cv, x = self.cv, self.p - 1
        with po.curve_ctx(cv):
            while True:
                y = po.fq_sqrt(cv, (x ** 3 + cv.a * x + cv.b) % cv.p)
                if y is not None:
                    assert cv.is_on_curve((x, y))
                    return po.pt_wire((x, y))
                x -= 1

    def outside_subgroup(self, P):
        """in Python integers: P is on the curve and [q]P != O"""
        with po.curve_ctx(self.cv):
            pt = po.pt_from_wire(P)
            return pt is not None and self.cv.is_on_curve(pt) and po.pt_mul_raw(self.cv, self.cv.q, pt) is not None


def _put(b, o, new):
    return b[:o] + new + b[o + len(new):]


def every_fourth(count):
    """every 4th index, starting with the first and always including the last"""
    return sorted(set(range(0, count, 4)) | {count - 1})


def run_ends(m, n):
    """(first, last) index of each of the three scalar runs of fs_cases.wire_map, as indices into its scalar list"""
    ends, o = [], 0
    for cnt in (2 * n + 3, 2 * n + 2, n + 4):
        ends += [o, o + cnt - 1]
        o += cnt
    assert o == 5 * n + 9
    return ends


def prove_rc(coracle, curve, m, n, params, pk, deck, rho, perm, seed):
    """coracle.shuffle_and_remask -> (0, deck, proof), or (the oracle's negative code, None, None)"""
    try:
        return (0,) + coracle.shuffle_and_remask(curve, m, n, params, pk, deck, rho, [v & 0xFFFFFFFF for v in perm], seed)
    except ValueError as e:
        return int(str(e).rsplit(":", 1)[1]), None, None


# ================================================================================================ Family A: verifier, every position
class Lane:
    """one lane of a verifier batch.  kind: "bad" (malformed: the oracle must say -1), "sub" (outside the subgroup: -1 by the header,
    checked in Python integers), "near" (a valid encoding next to an invalid one), "tamper" (well formed and wrong), "honest" """

    def __init__(self, name, kind, deck, shuf, proof, pk=None, group=None):
        self.name, self.kind, self.deck, self.shuf, self.proof, self.pk, self.group = name, kind, deck, shuf, proof, pk, group
        self.want = None


class World:
    """one (curve, m, n): parameters, a key, four honest statements with the oracle's proofs, and the Family-A lanes made from them"""

    def __init__(self, coracle, curve, m, n, seed=9100):
        self.co, self.curve, self.m, self.n, self.N = coracle, curve, m, n, m * n
        self.c = c = Pts(coracle, curve)
        self.gen = [coracle.gen_inputs(curve, m, n, seed + k) for k in range(4)]
        self.params, self.pk = self.gen[0]["params"], self.gen[0]["pk"]
        outs = sec._pmap(lambda g: coracle.shuffle_and_remask(curve, m, n, self.params, self.pk, g["deck"], g["rho"], g["perm"], g["prover_seed"]), self.gen)
        self.honest = [(g["deck"], d, p) for g, (d, p) in zip(self.gen, outs)]
        self.pts, self.scs, self.psz = fc.wire_map(m, n, c.pb)
        assert len(outs[0][1]) == self.psz
        self.key_pts = [self.params[i * c.pb:(i + 1) * c.pb] for i in range(n + 3)]
        self.sub = list(zip(SUBGROUP_KINDS, tc.off_subgroup_points())) if c.cofactor else []
        self.fails = []
        for name, P in self.sub:
            if not c.outside_subgroup(P):
                self.fails.append("%s: the %s is not a curve point outside the subgroup" % (curve, name))
        self.lanes = self._neighbours(self._malformed() + self._near())
        self.fails += self.expect(self.lanes)

    # ---- the statement the defects are made on, and edits of it
    def base(self, k=0):
        return self.honest[k % 4]

    def with_proof_point(self, i, f):
        d, s, p = self.base()
        o = self.pts[i]
        return d, s, _put(p, o, f(p[o:o + self.c.pb]))

    def with_scalar(self, i, v):
        d, s, p = self.base()
        return d, s, _put(p, self.scs[i], int(v).to_bytes(32, "little"))

    def with_deck_point(self, which, i, f):
        d, s, p = self.base()
        o = i * self.c.pb
        return (_put(d, o, f(d[o:o + self.c.pb])), s, p) if which == 0 else (d, _put(s, o, f(s[o:o + self.c.pb])), p)

    def tampered(self, k):
        """well formed and wrong: a proof point replaced by a base of the commitment key (k even), a response scalar + 1 (k odd)"""
        if k % 2 == 0:
            i = (k // 2) % len(self.pts)
            return self.with_proof_point(i, lambda P: next(x for x in self.key_pts[1:] + self.key_pts[:1] if x != P))
        i = (k // 2) % len(self.scs)
        d, s, p = self.base()
        return self.with_scalar(i, (int.from_bytes(p[self.scs[i]:self.scs[i] + 32], "little") + 1) % self.c.q)

    # ---- the lists of the issue
    def _malformed(self):
        c, N, L = self.c, self.N, []
        npt, nsc = len(self.pts), len(self.scs)
        for i in range(npt):
            L.append(Lane("proof point %d, x := p" % i, "bad", *self.with_proof_point(i, c.x_is_p)))
            L.append(Lane("proof point %d off the curve" % i, "bad", *self.with_proof_point(i, c.off_curve)))
        for i in every_fourth(npt):
            L.append(Lane("proof point %d, y := p + y" % i, "bad", *self.with_proof_point(i, c.y_past_p)))
        if c.top_bit():
            L.append(Lane("proof point 0, y := 2^%d" % c.p.bit_length(), "bad", *self.with_proof_point(0, lambda P: P[:c.fb] + c.top_bit())))
        if c.cofactor:
            for i in range(npt):
                L.append(Lane("proof point %d := the %s" % (i, self.sub[0][0]), "sub", *self.with_proof_point(i, lambda P: self.sub[0][1])))
            for i in (0, npt - 1):
                for name, Q in self.sub[1:]:
                    L.append(Lane("proof point %d := a %s" % (i, name), "sub", *self.with_proof_point(i, lambda P, Q=Q: Q)))
        for i in range(nsc):
            L.append(Lane("scalar %d := q" % i, "bad", *self.with_scalar(i, c.q)))
        for i in run_ends(self.m, self.n):
            for name, v in (("q + 1", c.q + 1), ("2^256 - 1", (1 << 256) - 1), ("2^%d" % c.q.bit_length(), c.scalar_bits())):
                if v is not None:
                    L.append(Lane("scalar %d := %s" % (i, name), "bad", *self.with_scalar(i, v)))
        for which, dname in ((0, "input deck"), (1, "shuffled deck")):
            for i in range(2 * N):
                L.append(Lane("%s point %d off the curve" % (dname, i), "bad", *self.with_deck_point(which, i, c.off_curve)))
            for i in (0, 2 * N - 1):
                L.append(Lane("%s point %d, x := p" % (dname, i), "bad", *self.with_deck_point(which, i, c.x_is_p)))
            if c.cofactor:
                for i in range(2 * N):
                    name, Q = self.sub[i % 3]
                    L.append(Lane("%s point %d := a %s" % (dname, i, name), "sub", *self.with_deck_point(which, i, lambda P, Q=Q: Q)))
        # malformed AND a wrong statement: refused as malformed
        d, s, p = self.tampered(1)
        L.append(Lane("a response + 1 and proof point 0, x := p", "bad", d, s, _put(p, self.pts[0], c.x_is_p(p[self.pts[0]:self.pts[0] + c.pb]))))
        d, s, p = self.tampered(0)
        L.append(Lane("a proof point replaced and shuffled deck point 1 off the curve", "bad", d, _put(s, c.pb, c.off_curve(s[c.pb:2 * c.pb])), p))
        return L

    def _near(self):
        c, npt = self.c, len(self.pts)
        big = c.largest_x()
        L = [Lane("scalar 0 := q - 1", "near", *self.with_scalar(0, c.q - 1)),
             Lane("scalar %d := q - 1" % (len(self.scs) - 1), "near", *self.with_scalar(len(self.scs) - 1, c.q - 1)),
             Lane("proof point 0 := infinity", "near", *self.with_proof_point(0, lambda P: c.inf)),
             Lane("proof point %d := infinity" % (npt - 1), "near", *self.with_proof_point(npt - 1, lambda P: c.inf)),
             Lane("shuffled deck point 0 := infinity", "near", *self.with_deck_point(1, 0, lambda P: c.inf)),
             Lane("input deck point %d := infinity" % (2 * self.N - 1), "near", *self.with_deck_point(0, 2 * self.N - 1, lambda P: c.inf)),
             Lane("proof point 1 := a base of the key", "near", *self.tampered(2))]
        # the curve point with the largest x: a valid encoding where the group has prime order; on BLS12-377 it is (shown in Python
        # integers) outside the subgroup, one more bad encoding by the header
        if c.cofactor:
            if not c.outside_subgroup(big):
                self.fails.append("%s: the curve point with the largest x is in the subgroup, the case list calls it outside" % self.curve)
            L.append(Lane("proof point 2 := the curve point with the largest x", "sub", *self.with_proof_point(2, lambda P: big)))
        else:
            L.append(Lane("proof point 2 := the curve point with the largest x", "near", *self.with_proof_point(2, lambda P: big)))
        return L

    def _neighbours(self, lanes):
        """an honest lane (of the four statements in turn) or a tampered one after every four of `lanes`"""
        out, k = [], 0
        for i, ln in enumerate(lanes):
            out.append(ln)
            if i % 4 == 3 or i == len(lanes) - 1:
                out.append(Lane("honest %d" % (k // 2), "honest", *self.base(k // 2)) if k % 2 == 0 else Lane("tampered %d" % (k // 2), "tamper", *self.tampered(k // 2)))
                k += 1
        return out

    def expect(self, lanes, pk=None):
        """the oracle's word for every lane that has none yet, held against the lane's kind BEFORE any device call; fills lane.want
        -> the disagreements (failures of the case list: the caller adds them to the list its test asserts on)"""
        co, memo, fails = self.co, {}, []
        todo = [ln for ln in lanes if ln.want is None]

        def word(ln):
            return co.verify_shuffle(self.curve, self.m, self.n, self.params, ln.pk or pk or self.pk, ln.deck, ln.shuf, ln.proof)
        keys = {(ln.pk, ln.deck, ln.shuf, ln.proof): ln for ln in todo}
        for key, o in zip(keys, sec._pmap(word, list(keys.values()))):
            memo[key] = o
        for ln in todo:
            o = memo[(ln.pk, ln.deck, ln.shuf, ln.proof)]
            ok = {"bad": o == BAD_ENCODING, "sub": o >= 0, "near": o >= 0, "tamper": o > 0, "honest": o == 0}[ln.kind]
            if not ok:
                fails.append("%s (%d, %d) case list: %s lane '%s': the oracle says %d" % (self.curve, self.m, self.n, ln.kind, ln.name, o))
            ln.want = BAD_ENCODING if ln.kind in ("bad", "sub") else o
        return fails


def malformed_count(curve, m, n):
    """lanes of World._malformed + World._near, from the lists of the issue"""
    cv = po.CURVES[curve]
    fb = 8 * ((cv.p.bit_length() + 63) // 64)
    npt, nsc, N, cof = 11 * m + 8, 5 * n + 9, m * n, curve in po.COFACTOR
    pts = 2 * npt + len(every_fourth(npt)) + (1 if cv.p.bit_length() < 8 * fb else 0) + ((npt + 4) if cof else 0)
    scs = nsc + 6 * (2 + (1 if cv.q.bit_length() < 256 else 0))
    decks = 2 * (2 * N + 2 + (2 * N if cof else 0))
    return pts + scs + decks + 2 + 8          # (two lanes that are malformed and wrong, eight near misses)


def lanes_count(curve, m, n):
    k = malformed_count(curve, m, n)
    return k + (k + 3) // 4


_WORLDS = {}


def world(coracle, curve, m, n):
    """the lanes of a shape and the oracle's words, made once and shared by the tests (nothing changes them)"""
    key = (curve, m, n)
    if key not in _WORLDS:
        _WORLDS[key] = World(coracle, curve, m, n)
    return _WORLDS[key]


def _cat(lanes, what):
    return b"".join(getattr(ln, what) for ln in lanes)


def _diff(fails, tag, lanes, got, want=None):
    for b, ln in enumerate(lanes):
        w = ln.want if want is None else want[b]
        if got[b] != w:
            fails.append("%s: lane %d (%s): status %d, expected %d" % (tag, b, ln.name, got[b], w))
    return len(lanes)


def run_verifier_positions(eng, coracle, curve, m, n):
    """all Family-A lanes of the shape in one batch per mode of MODES: every word is the expected one"""
    w = world(coracle, curve, m, n)
    lanes = w.lanes
    fails, checks = list(w.fails), 0
    if len(w.lanes) != lanes_count(curve, m, n):
        fails.append("%s (%d, %d): %d lanes, the lists of the issue give %d" % (curve, m, n, len(w.lanes), lanes_count(curve, m, n)))
    t = eng.table(m, n, w.params, w.pk)
    try:
        t.set_merged_verify(True)
        for lb, tl in MODES:
            t.set_latency_batch(lb)
            t.set_transcript_lanes(tl)
            got = t.verify_shuffle_batch(_cat(lanes, "deck"), _cat(lanes, "shuf"), _cat(lanes, "proof"))
            checks += _diff(fails, "%s (%d, %d), latency batch %d, %d-lane transcripts" % (curve, m, n, lb, tl), lanes, got)
    finally:
        t.close()
    return fails, checks


def positions_count(curve, m, n):
    return len(MODES) * lanes_count(curve, m, n)


def key_lanes(w):
    """per-proof keys: honest proofs under their own key, a proof under its neighbour's key, and the bad keys"""
    c, co = w.c, w.co
    if hasattr(w, "_key_lanes"):
        return w._key_lanes
    L = []
    own = []
    for k in range(3):
        g = co.gen_inputs(w.curve, w.m, w.n, 9200 + k)
        d, p = co.shuffle_and_remask(w.curve, w.m, w.n, w.params, g["pk"], g["deck"], g["rho"], g["perm"], g["prover_seed"])
        own.append((g["pk"], g["deck"], d, p))
    pk, deck, sh, pf = own[0]
    bad = [("key off the curve", "bad", c.off_curve(pk)), ("key, x := p", "bad", c.x_is_p(pk)), ("key, y := p + y", "bad", c.y_past_p(pk))]
    bad += [("key := a %s" % name, "sub", Q) for name, Q in w.sub]
    for k, (name, kind, key) in enumerate(bad):
        L.append(Lane(name, kind, deck, sh, pf, pk=key))
        o = own[(k + 1) % 3]
        L.append(Lane("honest key %d" % k, "honest", o[1], o[2], o[3], pk=o[0]) if k % 2 == 0 else
                 Lane("the neighbour's key", "tamper", o[1], o[2], o[3], pk=own[(k + 2) % 3][0]))
    w._key_lanes = L, w.expect(L)
    return w._key_lanes


def run_verifier_keys(eng, coracle, curve, m, n, torch, device):
    """mp_verify_shuffle_batch_keys (host and device pointers) with a bad key in some lanes; mp_keyset_create refuses a set that
    holds one of them, as a call-level error, and accepts the set without it"""
    w = world(coracle, curve, m, n)
    L, key_fails = key_lanes(w)
    fails, checks = w.fails + key_fails, 0
    dv = sec._Dev(torch, device)
    t = eng.table(m, n, w.params, None)
    try:
        args = (_cat(L, "pk"), _cat(L, "deck"), _cat(L, "shuf"), _cat(L, "proof"))
        for lb in (0, 8192):
            t.set_latency_batch(lb)
            checks += _diff(fails, "%s (%d, %d) keys, latency batch %d" % (curve, m, n, lb), L, t.verify_shuffle_batch_keys(*args))
            d = [dv.bytes(a) for a in args]
            st = dv.status(len(L))
            dv.sync()
            t.verify_shuffle_batch_keys_dev(len(L), *(x.data_ptr() for x in d), st.data_ptr())
            eng.sync()
            checks += _diff(fails, "%s (%d, %d) keys, device pointers, latency batch %d" % (curve, m, n, lb), L, st.cpu().tolist())
        good = [ln.pk for ln in L if ln.kind in ("honest", "tamper")]
        for ln in [x for x in L if x.kind in ("bad", "sub")]:
            for at in (0, len(good)):
                try:
                    t.keyset(b"".join(good[:at] + [ln.pk] + good[at:])).close()
                    fails.append("%s: a key set with '%s' at %d was accepted" % (curve, ln.name, at))
                except Exception as e:      # noqa: BLE001 (the binding's NativeError: the call's own status word)
                    if getattr(e, "code", None) != BAD_ENCODING:
                        fails.append("%s: a key set with '%s' at %d: %r, expected MP_ERR_BAD_ENCODING" % (curve, ln.name, at, e))
                checks += 1
        t.keyset(b"".join(good)).close()
        checks += 1
    finally:
        t.close()
    return fails, checks


def keys_count(curve):
    bad = 3 + (3 if curve in po.COFACTOR else 0)
    return 4 * 2 * bad + 2 * bad + 1


# ================================================================================================ Family B: the same words under every strategy
def strategy_batch(w, L):
    """the Family-A lanes of w laid out for group equations of L members (lane b is member b / T of group b mod T): group g < M has
    exactly one malformed member, at member position g mod L; group M a malformed and a tampered one; group M + 1 only a tampered one;
    three honest groups follow.  -> (lanes, T, groups with a member whose word is positive, honest groups, failures of the case list)"""
    bad = [ln for ln in w.lanes if ln.kind in ("bad", "sub", "near")]
    M = len(bad)
    T = M + 5
    grid = [[None] * T for _ in range(L)]
    for g, ln in enumerate(bad):
        grid[g % L][g] = ln
    grid[0][M], grid[L - 1][M] = bad[0], Lane("tampered", "tamper", *w.tampered(0))
    grid[1 % L][M + 1] = Lane("tampered", "tamper", *w.tampered(1))
    k = 0
    for j in range(L):
        for g in range(T):
            if grid[j][g] is None:
                grid[j][g] = Lane("honest %d" % (k % 4), "honest", *w.base(k))
                k += 1
    lanes = [grid[j][g] for j in range(L) for g in range(T)]
    case_fails = w.expect(lanes)
    # Groups that MUST take the per-equation pass: those with a member whose word is positive (only that pass can name its check).  A
    # group whose only odd member is refused may take it or not: the engine loads infinity / zero for what it refuses, so that group's
    # equation fails as well and its members are looked at again (as built, every group but the honest ones), but an engine that left
    # refused lanes out of their equation would be as right.  Hence a lower bound from these groups, an upper bound from the honest ones.
    failing ={g for g in range(T) if any(grid[j][g].want > 0 for j in range(L))}
    return lanes, T, failing, {M + 2, M + 3, M + 4}, case_fails


def run_strategies(eng, coracle, curve, m, n, torch, device, group_l=GROUP_L):
    """the Family-A words under merged and per-equation verification, group equations of L members with and without refinement, and
    the pipelined lane: the words are the expected ones -- those of the per-equation verifier -- in every lane, none is left at
    MP_ERR_INTERNAL, and the per-equation pass looks at the failing groups' members and at none of the honest groups'"""
    w = world(coracle, curve, m, n)
    fails, checks = list(w.fails), 0
    per = 4 * m * n + 11 * m + 8
    dv = sec._Dev(torch, device)
    t = eng.table(m, n, w.params, w.pk)
    tag0 = "%s (%d, %d)" % (curve, m, n)
    try:
        t.set_group_adapt(False)
        for L in group_l:
            lanes, T, failing, honest, case_fails = strategy_batch(w, L)
            fails += case_fails
            B = len(lanes)
            args = (_cat(lanes, "deck"), _cat(lanes, "shuf"), _cat(lanes, "proof"))
            t.set_latency_batch(0)
            t.set_group_verify(0, 0)
            t.set_merged_verify(False)
            ref = t.verify_shuffle_batch(*args)
            checks += _diff(fails, "%s, %d lanes, equation by equation" % (tag0, B), lanes, ref)
            t.set_merged_verify(True)
            checks += _diff(fails, "%s, %d lanes, merged" % (tag0, B), lanes, t.verify_shuffle_batch(*args))
            t.set_group_verify(L * per, 0)
            if t.group_size(B) != L:
                fails.append("%s: group_size(%d) is %d, not %d" % (tag0, B, t.group_size(B), L))
            for refine, name in (((0, 1 << 30), "no refinement"), ((0, 0), "default refinement")):
                t.set_group_refine(*refine)
                before = t.reverified_count()
                got = t.verify_shuffle_batch(*args)
                looked = t.reverified_count() - before
                tag = "%s, groups of %d, %s" % (tag0, L, name)
                checks += _diff(fails, tag, lanes, got, ref)
                if INTERNAL in got:
                    fails.append("%s: lanes %s are left at MP_ERR_INTERNAL" % (tag, [b for b, v in enumerate(got) if v == INTERNAL][:8]))
                if refine[1] and not L * len(failing) <= looked <= B - L * len(honest):
                    fails.append("%s: %d proofs took the per-equation pass; the failing groups have %d members, the honest ones %d of %d" %
                                 (tag, looked, L * len(failing), L * len(honest), B))
                if not refine[1] and not len(failing) <= looked <= B - L * len(honest):
                    fails.append("%s: %d proofs took the per-equation pass" % (tag, looked))
                checks += 2
            t.set_group_refine(0, 0)
            # device pointers, pipelined: two calls in flight, the words read after the sync
            t.set_pipeline(1)
            d = [dv.bytes(a) for a in args]
            hon = [w.base(b) for b in range(B)]
            e = [dv.bytes(b"".join(h[i] for h in hon)) for i in range(3)]
            st, st2 = dv.status(B), dv.status(B)
            dv.sync()
            t.verify_shuffle_batch_dev(B, *(x.data_ptr() for x in d), st.data_ptr())
            t.verify_shuffle_batch_dev(B, *(x.data_ptr() for x in e), st2.data_ptr())
            eng.sync()
            t.set_pipeline(0)
            checks += _diff(fails, "%s, groups of %d, pipelined" % (tag0, L), lanes, st.cpu().tolist(), ref)
            if st2.cpu().tolist() != [0] * B:
                fails.append("%s, groups of %d, pipelined: the honest batch behind the malformed one has words %s" %
                             (tag0, L, [(b, v) for b, v in enumerate(st2.cpu().tolist()) if v][:8]))
            checks += 1
    finally:
        t.close()
    return fails, checks


def strategies_count(curve, m, n, group_l=GROUP_L):
    bad = malformed_count(curve, m, n)
    return sum(5 * L * (bad + 5) + 5 for L in group_l)


CHAIN_T, CHAIN_L = 3, 4


def run_chain(eng, coracle, curve, m, n):
    """mp_verify_shuffle_chain, 3 tables x 4 links, alone and with 3 tables per equation: table 0 has an off-curve point in the first,
    a middle (the second) and the last deck of its chain, table 1 an out-of-range scalar in its last link's proof and, alone, a bad
    inner deck, which refuses the link it enters and the link that made it and no other; table 2 is untouched.  The words are those of mp_verify_shuffle_batch on the same links,
    and the oracle's"""
    w = world(coracle, curve, m, n)
    c, co, T, L = w.c, coracle, CHAIN_T, CHAIN_L
    fails, checks = list(w.fails), 0
    chain, proofs = [[w.gen[k]["deck"] for k in range(T)]], []
    for j in range(L):
        outs = [co.shuffle_and_remask(curve, m, n, w.params, w.pk, chain[j][k], w.gen[(j + k) % 4]["rho"], w.gen[(j + k + 1) % 4]["perm"],
                                      bytes([j, k]) + w.gen[0]["prover_seed"][2:]) for k in range(T)]
        chain.append([o[0] for o in outs])
        proofs.append([o[1] for o in outs])
    pb, N = c.pb, w.N
    for j, k, i in ((0, 0, 0), (1, 0, N), (L, 0, 2 * N - 1), (1, 1, 1)):
        chain[j][k] = _put(chain[j][k], i * pb, c.off_curve(chain[j][k][i * pb:(i + 1) * pb]))
    proofs[3][1] = _put(proofs[3][1], w.scs[-1], c.q.to_bytes(32, "little"))
    exp = [co.verify_shuffle(curve, m, n, w.params, w.pk, chain[j][k], chain[j + 1][k], proofs[j][k]) for j in range(L) for k in range(T)]
    # decks 0, 1 and 4 of table 0 refuse its links 0, 1 and 3; deck 1 of table 1 its links 0 and 1, the scalar its link 3: link 2 of
    # either table stays 0 between refused neighbours -- a bad deck refuses the two links that touch it and no other
    want = [BAD_ENCODING if k < 2 and j != 2 else 0 for j in range(L) for k in range(T)]
    if exp != want:
        fails.append("%s chains, case list: the oracle's words are %s, expected %s" % (curve, exp, want))
    decks, pf = b"".join(b"".join(r) for r in chain), b"".join(b"".join(r) for r in proofs)
    t = eng.table(m, n, w.params, w.pk)
    try:
        t.set_latency_batch(0)
        dsz = len(chain[0][0])
        ref = t.verify_shuffle_batch(decks[:L * T * dsz], decks[T * dsz:], pf)
        if ref != want:
            fails.append("%s chains, link by link: words %s, expected %s" % (curve, ref, want))
        checks += L * T
        for group in (0, 3):
            t.set_chain_group(group)
            got = t.verify_shuffle_chain(T, L, decks, pf)
            if got != want:
                fails.append("%s chains, %d tables per equation: words %s, expected %s" % (curve, group, got, want))
            checks += L * T
        t.set_chain_group(0)
    finally:
        t.close()
    return fails, checks


def chain_count():
    return 3 * CHAIN_T * CHAIN_L


def run_validated(eng, coracle, torch, device, curve="bls12_377", m=2, n=3):
    """mp_set_validated on BLS12-377, each flag alone and all three: a point outside the subgroup at the first and last slot of a
    flagged range (decks; in a proof, at every point, whichever slot it takes) is no longer refused -- the word is the oracle's --,
    the same point in every range without a flag, and in the per-proof key, is still -1, and so are an off-curve point and x := p at
    the same places under every flag.  mp_deck_validate_dev gives -1 exactly for the decks that hold a bad point of any kind"""
    w = world(coracle, curve, m, n)
    c, N, npt = w.c, w.N, len(w.pts)
    fails, checks = list(w.fails), 0
    Q = w.sub[2][1]                      # a subgroup point + the low-order point
    kinds = (("off the subgroup", lambda P: Q), ("off the curve", c.off_curve), ("x := p", c.x_is_p))
    places = [("deck", 1, i) for i in (0, 2 * N - 1)] + [("shuffled", 2, i) for i in (0, 2 * N - 1)] + [("proof", 4, i) for i in range(npt)]
    lanes = []
    for rng_name, flag, i in places:
        for kname, f in kinds:
            args = w.with_proof_point(i, f) if flag == 4 else w.with_deck_point(flag - 1, i, f)
            ln = Lane("%s point %d %s" % (rng_name, i, kname), "sub" if f is kinds[0][1] else "bad", *args, pk=w.pk)
            ln.flag = flag if f is kinds[0][1] else 0
            lanes.append(ln)
    for kname, f in kinds:
        ln = Lane("key %s" % kname, "sub" if f is kinds[0][1] else "bad", *w.base(), pk=f(w.pk))
        ln.flag = 0
        lanes.append(ln)
    lanes = w._neighbours(lanes)
    for ln in lanes:
        ln.pk = ln.pk or w.pk
        ln.flag = getattr(ln, "flag", 0)
    fails += w.expect(lanes)
    oracle = sec._pmap(lambda ln: coracle.verify_shuffle(curve, m, n, w.params, ln.pk, ln.deck, ln.shuf, ln.proof), lanes)
    args = (_cat(lanes, "pk"), _cat(lanes, "deck"), _cat(lanes, "shuf"), _cat(lanes, "proof"))
    dv = sec._Dev(torch, device)
    t = eng.table(m, n, w.params, None)
    try:
        t.set_latency_batch(0)
        for flags in (0, 1, 2, 4, 7):
            t.set_validated(flags)
            want = [oracle[b] if ln.flag & flags else ln.want for b, ln in enumerate(lanes)]
            if flags and not any(wv != ln.want for wv, ln in zip(want, lanes)):
                fails.append("validated %d: no lane changes its expectation" % flags)
            checks += _diff(fails, "%s (%d, %d), validated %d" % (curve, m, n, flags), lanes, t.verify_shuffle_batch_keys(*args), want)
        t.set_validated(0)
        for what in ("deck", "shuf"):
            d, st = dv.bytes(_cat(lanes, what)), dv.status(len(lanes))
            dv.sync()
            t.deck_validate_dev(len(lanes), d.data_ptr(), st.data_ptr())
            eng.sync()
            rng_name = "deck point" if what == "deck" else "shuffled point"
            want = [BAD_ENCODING if ln.name.startswith(rng_name) else 0 for ln in lanes]
            checks += _diff(fails, "%s mp_deck_validate_dev, %s" % (curve, what), lanes, st.cpu().tolist(), want)
    finally:
        t.set_subgroup_check(True)
        t.set_validated(0)
        t.close()
    return fails, checks


def validated_count(m=2, n=3):
    k = 3 * (4 + 11 * m + 8) + 3
    return 7 * (k + (k + 3) // 4)


# ================================================================================================ Family C: prover
def bad_permutations(N):
    """(name, permutation) of the issue's list: each is refused with MP_ERR_BAD_PERMUTATION.  Lane i of k_prove_init_w reads positions
    i, i + 64, ...: the duplicate pairs fall in one lane's stride, in neighbouring lanes, and on the first and last position"""
    ident = list(range(N))

    def put(pairs):
        p = list(ident)
        for i, v in pairs:
            p[i] = v
        return p
    out = [("value N at position %d" % i, put([(i, N)])) for i in sorted({0, 63, 64, N - 1}) if i < N]
    out += [("value 0xFFFFFFFF", put([(N // 2, 0xFFFFFFFF)])), ("value 0x80000000", put([(N // 2, 0x80000000)]))]
    out += [("positions %d and %d equal" % (i, i + 64), put([(i + 64, ident[i])])) for i in sorted({0, N - 65}) if 0 <= i and i + 64 < N]
    out += [("positions %d and %d equal" % (i, i + 1), put([(i + 1, ident[i])])) for i in sorted({0, 63, N - 2}) if i + 1 < N]
    out += [("positions 0 and %d equal" % (N - 1), put([(N - 1, 0)])), ("all zeros", [0] * N),
            ("every value twice, the upper half missing", [i // 2 for i in range(N)])]
    return out


def permutations_count(N):
    return (len([i for i in {0, 63, 64, N - 1} if i < N]) + 2 + len([i for i in {0, N - 65} if 0 <= i and i + 64 < N]) +
            len([i for i in {0, 63, N - 2} if i + 1 < N]) + 3)


class PLane:
    def __init__(self, name, kind, deck, rho, perm, seed, pk=None):
        self.name, self.kind, self.deck, self.rho, self.perm, self.seed, self.pk = name, kind, deck, rho, perm, seed, pk
        self.want, self.out = None, None


class ProverWorld:
    """the Family-C lanes of one (curve, m, n): every lane's expectation is the oracle's return code, its output the oracle's bytes"""

    def __init__(self, coracle, curve, m, n, seed=9300):
        self.co, self.curve, self.m, self.n, self.N = coracle, curve, m, n, m * n
        self.c = c = Pts(coracle, curve)
        N = self.N
        self.gen = [coracle.gen_inputs(curve, m, n, seed + k) for k in range(6)]
        self.params, self.pk = self.gen[0]["params"], self.gen[0]["pk"]
        self.sub = list(zip(SUBGROUP_KINDS, tc.off_subgroup_points())) if c.cofactor else []
        self.fails = [] if all(c.outside_subgroup(P) for _, P in self.sub) else ["%s: a point of off_subgroup_points is in the subgroup" % curve]
        g = self.gen[0]
        sc = lambda v: int(v).to_bytes(32, "little")
        mk = lambda name, kind, deck=g["deck"], rho=g["rho"], perm=g["perm"]: PLane(name, kind, deck, rho, list(perm), g["prover_seed"])
        self.rho_perm = [mk("rho[%d] := q" % i, "bad", rho=_put(g["rho"], 32 * i, sc(c.q))) for i in range(N)]
        self.rho_perm += [mk("rho[%d] := 2^256 - 1" % i, "bad", rho=_put(g["rho"], 32 * i, sc((1 << 256) - 1))) for i in (0, N - 1)]
        self.rho_perm += [mk(name, "perm", perm=p) for name, p in bad_permutations(N)]
        pt = lambda i, f: _put(g["deck"], i * c.pb, f(g["deck"][i * c.pb:(i + 1) * c.pb]))
        L = list(self.rho_perm)
        big = c.largest_x()
        if c.cofactor and not c.outside_subgroup(big):
            self.fails.append("%s: the curve point with the largest x is in the subgroup, the case list calls it outside" % curve)
        L += [mk("deck point %d off the curve" % i, "bad", deck=pt(i, c.off_curve)) for i in range(2 * N)]
        L += [mk("deck point %d, x := p" % i, "bad", deck=pt(i, c.x_is_p)) for i in (0, 2 * N - 1)]
        if c.cofactor:
            L += [mk("deck point %d := a %s" % (i, self.sub[i % 3][0]), "sub", deck=pt(i, lambda P, i=i: self.sub[i % 3][1])) for i in range(2 * N)]
        L += [mk("rho[0] := q and positions 0 and 1 equal", "both", rho=_put(g["rho"], 0, sc(c.q)), perm=[0, 0] + list(range(2, N))),
              mk("rho[%d] := q - 1" % (N - 1), "near", rho=_put(g["rho"], 32 * (N - 1), sc(c.q - 1))),
              mk("deck point 0 := infinity", "near", deck=pt(0, lambda P: c.inf)),
              mk("deck point 1 := the curve point with the largest x", "sub" if c.cofactor else "near", deck=pt(1, lambda P: big)),
              mk("the identity", "near", perm=range(N)), mk("the reversal", "near", perm=range(N - 1, -1, -1))]
        self.lanes = self.neighbours(L)
        self.fails += self.expect(self.lanes)

    def honest(self, k):
        g = self.gen[k % 6]
        return PLane("honest %d" % (k % 6), "honest", g["deck"], g["rho"], list(g["perm"]), g["prover_seed"])

    def neighbours(self, lanes):
        out = []
        for i, ln in enumerate(lanes):
            out.append(ln)
            if i % 4 == 3 or i == len(lanes) - 1:
                out.append(self.honest(i // 4))
        return out

    def expect(self, lanes, pk=None):
        """as World.expect, with the oracle's prover: fills lane.want and lane.out -> the disagreements"""
        memo, fails = {}, []
        todo = {(ln.pk, ln.deck, ln.rho, tuple(ln.perm), ln.seed): ln for ln in lanes if ln.want is None}
        res = sec._pmap(lambda ln: prove_rc(self.co, self.curve, self.m, self.n, self.params, ln.pk or pk or self.pk, ln.deck, ln.rho, ln.perm, ln.seed),
                        list(todo.values()))
        for key, r in zip(todo, res):
            memo[key] = r
        for ln in lanes:
            if ln.want is not None:
                continue
            rc, d, p = memo[(ln.pk, ln.deck, ln.rho, tuple(ln.perm), ln.seed)]
            # "sub": the oracle, which tests the curve equation alone, has PARSED the point -- neither -1 nor -2.  With a KEY of the wrong
            # order it then cannot finish (-3: [rho mod q] pk is not [rho] pk, and its prover's own check of the multi-exponentiation
            # witness throws); with such a deck point it proves.  That the point is outside the subgroup was shown in Python integers
            ok = {"bad": rc == BAD_ENCODING, "perm": rc == BAD_PERMUTATION, "both": rc in (BAD_ENCODING, BAD_PERMUTATION), "sub": rc in (0, -3),
                  "near": rc == 0, "honest": rc == 0}[ln.kind]
            if not ok:
                fails.append("%s (%d, %d) case list: %s lane '%s': the oracle says %d" % (self.curve, self.m, self.n, ln.kind, ln.name, rc))
            # a lane with a bad scalar AND a bad permutation may report either (kernels_proto.hpp status_fail)
            ln.want = {"bad": (BAD_ENCODING,), "sub": (BAD_ENCODING,), "perm": (BAD_PERMUTATION,), "both": (BAD_ENCODING, BAD_PERMUTATION)}.get(ln.kind, (0,))
            ln.out = (d, p) if ln.want == (0,) else None
        return fails


def prover_lanes_count(curve, m, n):
    N, cof = m * n, curve in po.COFACTOR
    k = N + 2 + permutations_count(N) + 2 * N + 2 + (2 * N if cof else 0) + 6
    return k + (k + 3) // 4


_PWORLDS = {}


def prover_world(coracle, curve, m, n):
    key = (curve, m, n)
    if key not in _PWORLDS:
        _PWORLDS[key] = ProverWorld(coracle, curve, m, n)
    return _PWORLDS[key]


def _compare_prover(fails, tag, lanes, out, dsz, psz):
    d, p, st = out
    for b, ln in enumerate(lanes):
        if st[b] not in ln.want:
            fails.append("%s: lane %d (%s): status %d, expected %s" % (tag, b, ln.name, st[b], " or ".join(map(str, ln.want))))
        elif ln.out and (d[b * dsz:(b + 1) * dsz], p[b * psz:(b + 1) * psz]) != ln.out:
            fails.append("%s: lane %d (%s): the output differs from the oracle's" % (tag, b, ln.name))
    return len(lanes)


def _proved(eng, fails, tag, kernel, call):
    """call() with the profile on: `kernel` made the permutation check, the other form did not run"""
    eng.profile_enable(True)
    out = call()
    rep = eng.profile_report()
    eng.profile_enable(False)
    other = "k_prove_init" if kernel == "k_prove_init_w" else "k_prove_init_w"
    if kernel not in rep or other in rep:
        fails.append("%s: expected %s, the profile has %s" % (tag, kernel, sorted(k for k in rep if k.startswith("k_prove_init"))))
    return out


def run_prover(eng, coracle, curve, m, n):
    """the Family-C lanes in one mp_shuffle_and_remask_batch call, on the wave form of the permutation check, with the prover's two
    streams and with one: status words, and the oracle's bytes on every lane that is not refused"""
    w = prover_world(coracle, curve, m, n)
    fails, checks = list(w.fails), 0
    lanes = w.lanes
    if len(lanes) != prover_lanes_count(curve, m, n):
        fails.append("%s (%d, %d): %d prover lanes, the lists of the issue give %d" % (curve, m, n, len(lanes), prover_lanes_count(curve, m, n)))
    dsz, psz = len(lanes[0].deck), coracle.proof_size(m, n, curve)
    args = (_cat(lanes, "deck"), _cat(lanes, "rho"), [v for ln in lanes for v in ln.perm], _cat(lanes, "seed"))
    t = eng.table(m, n, w.params, w.pk)
    try:
        for lb in (8192, 0):
            t.set_latency_batch(lb)
            tag = "%s (%d, %d) prover, latency batch %d" % (curve, m, n, lb)
            out = _proved(eng, fails, tag, "k_prove_init_w", lambda: t.shuffle_and_remask_batch(*args))
            checks += _compare_prover(fails, tag, lanes, out, dsz, psz) + 1
    finally:
        t.close()
    return fails, checks


def prover_count(curve, m, n):
    return 2 * (prover_lanes_count(curve, m, n) + 1)


def run_prover_lone_lane(eng, coracle, curve="stark", m=2, n=3):
    """one call of 32 769 six-card proofs, the batch size from which one lane per proof checks the permutation (k_prove_init): every
    permutation and masking-factor defect of the N = 6 list once in the first 64 lanes and once in the last 64, six honest inputs in
    turn between them; the honest lanes' outputs are the oracle's bytes"""
    w = prover_world(coracle, curve, m, n)
    fails = list(w.fails)
    B, K = LONE_LANE_BATCH, len(w.rho_perm)
    assert K <= 64
    six = [w.honest(k) for k in range(6)]
    fails += w.expect(six)
    lanes = [six[b % 6] for b in range(B)]
    for k, ln in enumerate(w.rho_perm):                     # (lanes of w.lanes: their expectations are made already)
        lanes[(5 * k + 2) % 64] = ln
        lanes[B - 64 + (5 * k + 3) % 64] = ln
    dsz, psz = len(lanes[0].deck), coracle.proof_size(m, n, curve)
    args = (_cat(lanes, "deck"), _cat(lanes, "rho"), [v & 0xFFFFFFFF for ln in lanes for v in ln.perm], _cat(lanes, "seed"))
    t = eng.table(m, n, w.params, w.pk)
    try:
        tag = "%s (%d, %d) prover, %d proofs" % (curve, m, n, B)
        out = _proved(eng, fails, tag, "k_prove_init", lambda: t.shuffle_and_remask_batch(*args))
        checks = _compare_prover(fails, tag, lanes, out, dsz, psz) + 1
    finally:
        t.close()
    if sum(1 for ln in lanes if ln.kind != "honest") != 2 * K:
        fails.append("%d defect lanes in the batch, expected %d" % (sum(1 for ln in lanes if ln.kind != "honest"), 2 * K))
    return fails, checks


def lone_lane_count():
    return LONE_LANE_BATCH + 1


def run_prover_keys(eng, coracle, curve, m, n):
    """the keyed and the seeded prover with a bad key in some lanes: -1 there, the oracle's bytes in the lanes between"""
    w = prover_world(coracle, curve, m, n)
    c, co = w.c, coracle
    fails, checks = list(w.fails), 0
    keys = [co.gen_inputs(curve, m, n, 9400 + k)["pk"] for k in range(3)]
    bad = [("key off the curve", "bad", c.off_curve(keys[0])), ("key, x := p", "bad", c.x_is_p(keys[0]))] + [("key := a %s" % s, "sub", Q) for s, Q in w.sub]
    lanes = []
    for k, (name, kind, key) in enumerate(bad):
        g = w.gen[k % 6]
        lanes.append(PLane(name, kind, g["deck"], g["rho"], list(g["perm"]), g["prover_seed"], pk=key))
        h = w.honest(k + 1)
        h.pk = keys[k % 3]
        lanes.append(h)
    fails += w.expect(lanes)
    dsz, psz = len(lanes[0].deck), co.proof_size(m, n, curve)
    t = eng.table(m, n, w.params, None)
    try:
        for lb in (8192, 0):
            t.set_latency_batch(lb)
            tag = "%s (%d, %d) keyed prover, latency batch %d" % (curve, m, n, lb)
            out = t.shuffle_and_remask_batch_keys(_cat(lanes, "pk"), _cat(lanes, "deck"), _cat(lanes, "rho"), [v for ln in lanes for v in ln.perm], _cat(lanes, "seed"))
            checks += _compare_prover(fails, tag, lanes, out, dsz, psz)
        # seeded: the witness is drawn on the device from the lane's seed, which is also the prover seed; the oracle proves from what
        # the call reports it drew
        t.set_latency_batch(8192)
        d, p, st, perms, rho = t.shuffle_and_remask_batch_seeded(_cat(lanes, "deck"), _cat(lanes, "seed"), keys=_cat(lanes, "pk"), witness=True)
        N = w.N
        for b, ln in enumerate(lanes):
            tag = "%s (%d, %d) seeded prover, lane %d (%s)" % (curve, m, n, b, ln.name)
            if ln.kind != "honest":
                if st[b] != BAD_ENCODING:
                    fails.append("%s: status %d, expected -1" % (tag, st[b]))
            else:
                rc, od, op = prove_rc(co, curve, m, n, w.params, ln.pk, ln.deck, rho[32 * N * b:32 * N * (b + 1)], perms[N * b:N * (b + 1)], ln.seed)
                if st[b] != 0 or rc != 0 or (d[b * dsz:(b + 1) * dsz], p[b * psz:(b + 1) * psz]) != (od, op):
                    fails.append("%s: status %d, the oracle's %d, outputs %s" % (tag, st[b], rc, "differ" if rc == 0 and st[b] == 0 else "not compared"))
            checks += 1
    finally:
        t.close()
    return fails, checks


def prover_keys_count(curve):
    return 3 * 2 * (2 + (3 if curve in po.COFACTOR else 0))
