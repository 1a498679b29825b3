"""Cases, references and checks for the part of the trait that is not the shuffle argument: the batched sigma protocols (mp_sigma_prove_batch,
mp_sigma_verify_batch: Schnorr identification with one base, Chaum-Pedersen with two), mp_remask_batch and mp_commit_batch, on every curve.
Shared by tests/test_cabi_and_host.py (the kernel bodies under the development emulator, CPU) and tests/test_gpu_protocol.py (the gfx950
build) -- same cases, same expectations, exact equality with the C++ oracle (and, for one batch, with the Python oracle as well).

Every run_* function takes an engine (_native.Engine), the coracle module and a curve name, and returns (failure messages, number of
checks made); the tests assert that the list is empty.

mp_oracle keeps the coordinate width in a global: whatever touches po.pt_wire and the like here runs inside po.curve_ctx(cv).  Statements
are built with coracle.msm (the Python oracle's pt_mul would dominate the run time, on BLS12-377 above all)."""
import functools
import hashlib
import random

import mp_oracle as po

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
BATCHES = (1, 63, 64, 65, 257)           # around one wave and around one block of 256 lanes
PO_BATCH = 65                            # the batch that is also compared with the Python oracle
M_, N_ = 2, 5                            # the table the calls go through (the sigma calls use none of its bases)
BAD_ENCODING = -1                        # MP_ERR_BAD_ENCODING (include/mpshuffle.h)


def fs_inits(i):
    """the bytes the four protocol steps seed their FiatShamirRng with [REF mod.rs:80-83]; the key-ownership one carries the player's
    public information, of a length that changes from lane to lane"""
    return [po.KEY_OWN_RNG_SEED + b"player public info"[:i % 19] + bytes([i & 0xFF]), po.MASKING_RNG_SEED, po.REMASKING_RNG_SEED, po.REVEAL_RNG_SEED]


def edge_scalars(q):
    return [0, 1, 2, q - 1, (q - 1) // 2, (q + 1) // 2]


class Ctx:
    """one curve: a table, a pool of subgroup points with known logarithms to the first of them, and the oracle's group operations on bytes"""

    def __init__(self, eng, coracle, curve):
        self.eng, self.co, self.curve = eng, coracle, curve
        self.cv = po.CURVES[curve]
        self.q, self.p, self.pb = self.cv.q, self.cv.p, eng.point_bytes
        self.fb = self.pb // 2
        assert coracle.point_size(curve) == self.pb
        self.gi = coracle.gen_inputs(curve, M_, N_, 61)
        self.params, self.pk = self.gi["params"], self.gi["pk"]
        self.G = self.params[:self.pb]
        self.t = eng.table(M_, N_, self.params, self.pk)
        self.inf = bytes(self.pb)
        rng = random.Random(97 + self.cv.cid)
        self.pool_k = [1] + [rng.randrange(2, self.q) for _ in range(15)]
        self.pool = [self.mul(k, self.G) for k in self.pool_k]

    def close(self):
        self.t.close()

    def sc(self, k):
        return int(k).to_bytes(32, "little")

    def mul(self, k, P):
        return self.co.msm(self.curve, self.sc(k % self.q), P)

    def add(self, P, Q):
        return self.co.msm(self.curve, self.sc(1) * 2, P + Q)

    def neg(self, P):
        if P == self.inf:
            return P
        y = int.from_bytes(P[self.fb:], "little")
        return P[:self.fb] + ((self.p - y) % self.p).to_bytes(self.fb, "little")

    def xy(self, P):
        return int.from_bytes(P[:self.fb], "little"), int.from_bytes(P[self.fb:], "little")

    def off_curve(self, P):
        """one bit of x flipped: canonical coordinates of a point that is not on the curve"""
        bad = bytes([P[0] ^ 1]) + P[1:]
        x, y = self.xy(bad)
        assert x < self.p and not self.cv.is_on_curve((x, y))
        return bad

    def fs_digest(self, raw):
        return hashlib.blake2s(raw).digest()      # what the engine takes: Blake2s of the bytes the oracle takes


class Lane:
    """one proof: statement, witness, transcript seed bytes and prover seed"""

    def __init__(self, c, nb, g, x, fs, seed):
        self.nb, self.g, self.x, self.fs, self.seed = nb, list(g), x, fs, seed
        self.a = [c.mul(x, gi) for gi in g]
        self.proof = None

    def prove(self, c):
        self.proof = c.co.sigma_prove(c.curve, self.nb, b"".join(self.g), b"".join(self.a), c.sc(self.x), self.fs, self.seed)
        return self.proof


def honest_lanes(c, nb, B, salt=0):
    """witnesses cycle through 0, 1, 2, q - 1, (q - 1) / 2, (q + 1) / 2 and two random values (0: every public is the point at infinity,
    which is absorbed into the transcript; 1 and q - 1: a = +-g, the exceptional additions inside the verifier's MSM); from three lanes
    on, lane 1 has g_1 = g_0 and lane 2 has g_1 = -g_0; from five lanes on, lanes 3 and 4 share witness, transcript seed and prover seed
    and differ only in the statement.  fs_init and prover seed change from lane to lane."""
    rng = random.Random(1000 * B + 10 * nb + salt + c.cv.cid)
    E = edge_scalars(c.q)
    lanes = []
    for i in range(B):
        k = (i + B) % 8
        x = E[k] if k < 6 else rng.randrange(3, c.q - 1)
        g = [c.pool[(i + 7 * j + B) % len(c.pool)] for j in range(nb)]
        if nb == 2 and g[1] == g[0]:
            g[1] = c.pool[(i + B + 1) % len(c.pool)]
        if nb == 2 and B >= 3 and i == 1:
            g[1] = g[0]
        if nb == 2 and B >= 3 and i == 2:
            g[1] = c.neg(g[0])
        fs = fs_inits(i + salt)[(i + B) % 4]
        seed = hashlib.blake2s(b"prover seed %d %d %d" % (B, nb, i)).digest()
        if B >= 5 and i == 4:
            prev = lanes[3]
            x, fs, seed = prev.x, prev.fs, prev.seed
            # one base: g' = 5 g; two bases: the same g_0 and another g_1.  A repeated nonce would show as A' = 5 A / as A_0' = A_0
            g = [c.mul(5, prev.g[0])] if nb == 1 else [prev.g[0], c.mul(5, prev.g[1])]
        lanes.append(Lane(c, nb, g, x, fs, seed))
    return lanes


def _cat(lanes, what):
    return b"".join(b"".join(getattr(l, what)) for l in lanes)


def prove_batch(c, nb, lanes):
    return c.t.sigma_prove_batch(nb, _cat(lanes, "g"), _cat(lanes, "a"), b"".join(c.sc(l.x) for l in lanes),
                                 b"".join(c.fs_digest(l.fs) for l in lanes), b"".join(l.seed for l in lanes))


def verify_batch(c, nb, rows):
    """rows: (g bytes, a bytes, proof bytes, fs bytes) per lane"""
    return c.t.sigma_verify_batch(nb, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[2] for r in rows),
                                  b"".join(c.fs_digest(r[3]) for r in rows))


def run_sigma_honest(eng, coracle, curve):
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    for nb in (1, 2):
        psz = nb * c.pb + 32
        for B in BATCHES:
            lanes = honest_lanes(c, nb, B)
            want = [l.prove(c) for l in lanes]
            got, st = prove_batch(c, nb, lanes)
            tag = "%s nbases %d batch %d" % (curve, nb, B)
            if st != [0] * B:
                fails.append("%s: prove status %s" % (tag, [(i, v) for i, v in enumerate(st) if v]))
            for i, l in enumerate(lanes):
                if got[i * psz:(i + 1) * psz] != want[i]:
                    fails.append("%s lane %d (witness %#x): proof differs from the C++ oracle's" % (tag, i, l.x))
            sv = verify_batch(c, nb, [(b"".join(l.g), b"".join(l.a), want[i], l.fs) for i, l in enumerate(lanes)])
            if sv != [0] * B:
                fails.append("%s: verify status %s" % (tag, [(i, v) for i, v in enumerate(sv) if v]))
            checks += 3 * B
            if B >= 5:
                A3, A4 = want[3][:c.pb], want[4][:c.pb]
                if (c.mul(5, A3) if nb == 1 else A3) == A4:
                    fails.append("%s: lanes 3 and 4 (one seed, two statements) used the same nonce" % tag)
                checks += 1
            if B == PO_BATCH:      # the third restatement: the Python oracle
                with po.curve_ctx(c.cv):
                    for i, l in enumerate(lanes):
                        g, a = [po.pt_from_wire(v) for v in l.g], [po.pt_from_wire(v) for v in l.a]
                        if po.sigma_proof_bytes(po.sigma_prove(c.cv, g, a, l.x, l.fs, l.seed)) != got[i * psz:(i + 1) * psz]:
                            fails.append("%s lane %d (witness %#x): proof differs from the Python oracle's" % (tag, i, l.x))
                checks += B
    c.close()
    return fails, checks


def _defects(c, nb):
    """(name, off_curve, edit) -- edit(g, a, A, z, fs) changes the lists in place and returns (z bytes, fs)"""
    q, pb = c.q, c.pb
    spare = [c.pool[13], c.pool[14]]
    out = []

    def scalar(name, f):
        out.append((name, False, lambda g, a, A, z, fs: (f(int.from_bytes(z, "little")).to_bytes(32, "little"), fs)))

    def point(name, which, i, f, off=False):
        def edit(g, a, A, z, fs):
            v = {"g": g, "a": a, "A": A}[which]
            v[i] = f(v[i])
            return z, fs
        out.append((name, off, edit))

    scalar("z + 1", lambda z: (z + 1) % q)
    if 2 * q - 1 < 1 << 256:                                   # z + q fits in 32 bytes for every z
        scalar("z + q", lambda z: z + q)
    scalar("z = ff..ff", lambda z: (1 << 256) - 1)
    for i in range(nb):
        point("A_%d replaced" % i, "A", i, lambda P, i=i: spare[i])
    point("A_0 = infinity", "A", 0, lambda P: c.inf)
    if nb == 2:
        def swap(g, a, A, z, fs):
            A[0], A[1] = A[1], A[0]
            return z, fs
        out.append(("A_0 and A_1 swapped", False, swap))
    for i in range(nb):
        point("a_%d replaced" % i, "a", i, lambda P, i=i: spare[i])
    point("a_0 = infinity", "a", 0, lambda P: c.inf)
    for i in range(nb):
        point("g_%d replaced" % i, "g", i, lambda P, i=i: spare[i])
    point("g_0 = infinity", "g", 0, lambda P: c.inf)
    out.append(("fs_init of another protocol step", False,
                lambda g, a, A, z, fs: (z, po.MASKING_RNG_SEED if fs != po.MASKING_RNG_SEED else po.REVEAL_RNG_SEED)))
    for which in ("g", "a", "A"):
        point("%s_%d off the curve" % (which, nb - 1), which, nb - 1, c.off_curve, off=True)
    return out


def _apply(c, nb, lane, edit):
    g, a = list(lane.g), list(lane.a)
    A = [lane.proof[c.pb * i:c.pb * (i + 1)] for i in range(nb)]
    z, fs = edit(g, a, A, lane.proof[c.pb * nb:], lane.fs)
    return b"".join(g), b"".join(a), b"".join(A) + z, fs


def run_sigma_rejections(eng, coracle, curve):
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    for nb in (1, 2):
        defects = _defects(c, nb)
        B = len(defects) + 2
        # random witnesses and distinct bases: every defect is a defect (with witness 0, replacing g_i would change nothing that the
        # equations see but the challenge)
        rng = random.Random(7 + nb + c.cv.cid)
        lanes = [Lane(c, nb, [c.pool[(i + 5 * j) % 12] for j in range(nb)], rng.randrange(3, c.q - 1), fs_inits(i)[i % 4],
                      hashlib.blake2s(b"rejections %d %d" % (nb, i)).digest()) for i in range(B)]
        for l in lanes:
            l.prove(c)
        ident = lambda g, a, A, z, fs: (z, fs)
        rows, want, names = [], [], []
        for i, l in enumerate(lanes):
            name, off, edit = ("honest", False, ident) if i in (0, B - 1) else defects[i - 1]
            row = _apply(c, nb, l, edit)
            rows.append(row)
            names.append(name)
            verdict = coracle.sigma_verify(curve, nb, *row)
            # A point off the curve: the engine documents MP_ERR_BAD_ENCODING for it, which is also what the shuffle verifier's tests
            # expect of a deck point off the curve (the C++ oracle refuses it as well since pt_from_wire in oracle/c/shuffle.hpp tests
            # the curve equation; before, it called such a point a failed equation).
            want.append(BAD_ENCODING if off else verdict)
            if (verdict == 0) != (name == "honest"):
                fails.append("%s nbases %d: the oracle says %d for the case '%s'" % (curve, nb, verdict, name))
        got = verify_batch(c, nb, rows)
        for i in range(B):
            if got[i] != want[i]:
                fails.append("%s nbases %d lane %d (%s): status %d, expected %d" % (curve, nb, i, names[i], got[i], want[i]))
        checks += B
        # ---- the prover: a witness >= q, a base off the curve and (BLS12-377) a base outside the subgroup, between honest lanes
        bad = {1: "witness >= q", 3: "base off the curve"}
        if curve == "bls12_377":
            bad[5] = "base outside the subgroup"
        P = max(bad) + 2
        pl = lanes[:P]
        gb = [list(l.g) for l in pl]
        gb[3][nb - 1] = c.off_curve(gb[3][nb - 1])
        if 5 in bad:
            gb[5][0] = off_subgroup_points()[2]
        xs = [c.sc(c.q if i == 1 else l.x) for i, l in enumerate(pl)]
        got, st = c.t.sigma_prove_batch(nb, b"".join(b"".join(g) for g in gb), _cat(pl, "a"), b"".join(xs),
                                        b"".join(c.fs_digest(l.fs) for l in pl), b"".join(l.seed for l in pl))
        psz = nb * c.pb + 32
        for i, l in enumerate(pl):
            if i in bad:
                if not st[i] < 0:
                    fails.append("%s nbases %d prove lane %d (%s): status %d, expected a negative one" % (curve, nb, i, bad[i], st[i]))
            elif st[i] != 0 or got[i * psz:(i + 1) * psz] != l.proof:
                fails.append("%s nbases %d prove lane %d (honest, next to a refused one): status %d, proof %s" %
                             (curve, nb, i, st[i], "equal" if got[i * psz:(i + 1) * psz] == l.proof else "differs from the oracle's"))
        checks += P
    c.close()
    return fails, checks


@functools.lru_cache(maxsize=None)
def off_subgroup_points():
    """BLS12-377 G1 points on the curve and outside the prime-order subgroup, as
    tests/test_cabi_and_host.py::test_points_outside_the_prime_order_subgroup_are_rejected builds them: a point of low order, a curve
    point before cofactor clearing, and a subgroup point plus the low-order one"""
    cv = po.CURVES["bls12_377"]
    with po.curve_ctx(cv):
        x = 5
        while True:
            y = po.fq_sqrt(cv, (x ** 3 + cv.b) % cv.p)
            if y is not None and po.pt_mul_raw(cv, cv.q, (x, y)) is not None:
                break
            x += 1
        low = po.pt_mul_raw(cv, cv.q, (x, y))
        assert cv.is_on_curve(low) and po.pt_mul_raw(cv, po.COFACTOR["bls12_377"], low) is None
        return po.pt_wire(low), po.pt_wire((x, y)), po.pt_wire(po.pt_add(cv, low, cv.G))


def run_sigma_subgroup(eng, coracle, curve="bls12_377"):
    """each kind of point outside the subgroup as g_0, as a_1 and as A_0 of a Chaum-Pedersen batch, between honest lanes: refused as a bad
    encoding, and only those lanes; with the table's subgroup test off (the caller vouches for its points) the oracle's verdict"""
    assert curve == "bls12_377"
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    nb = 2
    kinds = list(zip(("low-order point", "point before cofactor clearing", "subgroup point + low-order point"), off_subgroup_points()))
    places = [("g", 0), ("a", 1), ("A", 0)]
    B = 2 * len(kinds) * len(places) + 1
    rng = random.Random(5)
    lanes = [Lane(c, nb, [c.pool[(i + 5 * j) % 12] for j in range(nb)], rng.randrange(3, c.q - 1), fs_inits(i)[1 + i % 3],
                  hashlib.blake2s(b"subgroup %d" % i).digest()) for i in range(B)]
    rows, names, bad_lanes = [], [], []
    for i, l in enumerate(lanes):
        l.prove(c)
        edit, name = (lambda g, a, A, z, fs: (z, fs)), "honest"
        if i % 2 == 1:
            (kname, pt), (which, k) = kinds[(i // 2) // len(places)], places[(i // 2) % len(places)]
            name = "%s as %s_%d" % (kname, which, k)

            def edit(g, a, A, z, fs, pt=pt, which=which, k=k):
                {"g": g, "a": a, "A": A}[which][k] = pt
                return z, fs
            bad_lanes.append(i)
        rows.append(_apply(c, nb, l, edit))
        names.append(name)
    got = verify_batch(c, nb, rows)
    for i in range(B):
        want = BAD_ENCODING if i in bad_lanes else 0
        if got[i] != want:
            fails.append("%s verify lane %d (%s): status %d, expected %d" % (curve, i, names[i], got[i], want))
    checks += B
    # the prover: a bad base (lane 1 + 6 k: g_0) or a bad public (lane 3 + 6 k: a_1); lanes whose bad point is a commitment are left out
    pl = [i for i in range(B) if i not in bad_lanes or names[i].split(" as ")[1] != "A_0"]
    gotp, st = c.t.sigma_prove_batch(nb, b"".join(rows[i][0] for i in pl), b"".join(rows[i][1] for i in pl), b"".join(c.sc(lanes[i].x) for i in pl),
                                     b"".join(c.fs_digest(lanes[i].fs) for i in pl), b"".join(lanes[i].seed for i in pl))
    psz = nb * c.pb + 32
    for j, i in enumerate(pl):
        if i in bad_lanes:
            if not st[j] < 0:
                fails.append("%s prove lane %d (%s): status %d, expected a negative one" % (curve, i, names[i], st[j]))
        elif st[j] != 0 or gotp[j * psz:(j + 1) * psz] != lanes[i].proof:
            fails.append("%s prove lane %d (honest): status %d, proof %s" % (curve, i, st[j], "equal" if gotp[j * psz:(j + 1) * psz] == lanes[i].proof
                                                                           else "differs from the oracle's"))
    checks += len(pl)
    c.t.set_subgroup_check(False)
    try:
        got = verify_batch(c, nb, rows)
    finally:
        c.t.set_subgroup_check(True)
    for i in range(B):
        want = coracle.sigma_verify(curve, nb, *rows[i])
        if got[i] != want:
            fails.append("%s verify lane %d (%s), subgroup test off: status %d, the oracle says %d" % (curve, i, names[i], got[i], want))
    checks += B
    c.close()
    return fails, checks


def run_remask(eng, coracle, curve):
    """mp_remask_batch against the oracle's remask, card by card: factors alternate between 0, 1, 2, q - 1, (q - 1) / 2, (q + 1) / 2 and
    random values; cards with the first half, the second half and both halves at infinity, and the card (G, pk) itself under the
    factors 1 and q - 1 (a doubling and a cancellation to infinity inside the fixed-base path)"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    E = edge_scalars(c.q)
    cb = 2 * c.pb
    for count in (1, 63, 65, 257):
        rng = random.Random(300 + count + c.cv.cid)
        cards, factors, kinds = [], [], []
        for i in range(count):
            k = (i + count) % 6
            c0, c1 = c.pool[(i + count) % 16], c.pool[(3 * i + 5) % 16]
            rho = E[(i // 2) % 6] if i % 2 == 0 else rng.randrange(3, c.q - 1)
            if k == 1:
                c0 = c.inf
            elif k == 2:
                c1 = c.inf
            elif k == 3:
                c0 = c1 = c.inf
            elif k in (4, 5):
                c0, c1, rho = c.G, c.pk, (1 if k == 4 else c.q - 1)
            cards.append(c0 + c1)
            factors.append(rho)
            kinds.append(("generic", "first half at infinity", "second half at infinity", "both halves at infinity", "(G, pk) + 1 (G, pk)",
                          "(G, pk) - (G, pk)")[k])
        fb = b"".join(c.sc(v) for v in factors)
        got = c.t.remask_batch(b"".join(cards), fb)
        want = coracle.remask_deck(curve, c.G, c.pk, b"".join(cards), fb)
        if count >= 6 and not any(want[cb * i:cb * (i + 1)] == bytes(cb) for i in range(count) if kinds[i] == "(G, pk) - (G, pk)"):
            fails.append("%s remask: the cancellation case does not cancel" % curve)
        for i in range(count):
            if got[cb * i:cb * (i + 1)] != want[cb * i:cb * (i + 1)]:
                fails.append("%s remask count %d card %d (%s, factor %#x): differs from the oracle's" % (curve, count, i, kinds[i], factors[i]))
        checks += count
    c.close()
    return fails, checks


def run_commit(eng, coracle, curve):
    """mp_commit_batch against the oracle's Pedersen commitment: (count, length) = (1, n), (1, 1), (5, n - 1), (65, n), (3, 0); values and
    blinders include 0, 1 and q - 1, and row 1 of every call of several rows is all zero: the point at infinity"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    n = N_
    E = [0, 1, c.q - 1]
    for count, length in ((1, n), (1, 1), (5, n - 1), (65, n), (3, 0)):
        rng = random.Random(500 + 10 * count + length + c.cv.cid)
        vals, rs = [], []
        for i in range(count):
            row = [E[(i + l) % 3] if (i + l) % 2 == 0 else rng.randrange(c.q) for l in range(length)]
            r = E[i % 3] if i % 4 < 3 else rng.randrange(c.q)
            if i == 1:
                row, r = [0] * length, 0
            vals.append(row)
            rs.append(r)
        got = c.t.commit_batch(count, length, b"".join(c.sc(v) for row in vals for v in row), b"".join(c.sc(r) for r in rs))
        for i in range(count):
            want = coracle.commit(curve, n, c.params, b"".join(c.sc(v) for v in vals[i]), c.sc(rs[i]))
            if not any(vals[i]) and rs[i] == 0 and want != c.inf:
                fails.append("%s commit: the all-zero row is not the point at infinity in the oracle" % curve)
            if got[c.pb * i:c.pb * (i + 1)] != want:
                fails.append("%s commit count %d length %d row %d (values %s, r %#x): differs from the oracle's" %
                             (curve, count, length, i, " ".join("%#x" % v for v in vals[i]), rs[i]))
        checks += count
    c.close()
    return fails, checks
