"""Compressed points with PRESCRIBED structure for the decompression tests (tests/decompress_cases.py): inputs that random multiples of G
reach with probability 16^-j or never.  Everything here is Python integers and oracle/py -- no product code, none of the kernel's tables.

How a point is made to order: choose y, set r = y^2, solve x^3 + a x + b = r for x (`cubic_roots`: gcd with X^p - X, then equal-degree
splitting; about two targets in three have a root) and retry y when there is none.  With p - 1 = 2^S q (q odd), z the smallest
non-residue and g = z^q (order 2^S), the square root kernels walk the discrete logarithm E of t = rhs^q to base g in k = S / w windows
of w bits (w = 4 if 4 | S, else 2 if 2 | S, else 1 -- the kernel's rule, restated from its description, not read from the library).
y = g^f o with o = rand^(2^S) of odd order gives rhs^q = g^(2 f q), so f = (E / 2) q^-1 mod 2^(S-1) prescribes every digit of E (E even:
a square); rhs = g^f o with f = E q^-1 for odd E prescribes the digits of a NON-residue for which the cubic still has a root x.

Families (the `fam` field of an entry):
  a   first non-zero window i for every i, and rhs of odd order (every digit 0): the device walk keeps u = 1 with all R[.][0] products,
      host Tonelli-Shanks leaves its loop early with M - i - 1 large
  b   digit patterns: all digits maximal, all 1, one non-zero digit at each window, alternating 0 / max, e_0 = 2 only, and a systematic
      sweep e_i = (s + i) mod 2^w that hits every (window, digit) pair.  A square has e_0 even, so the residue forms clear bit 0 of e_0
      and the exact odd patterns are in family c
  c   non-residues with a root x: every odd e_0, higher digits all zero / random, all-maximal, all-1
  d   y at the sign rule's edges: y and p - y first differ in a chosen 32-bit limb (y = (p-1)/2 - d 2^(32 i)), y in {1, 2, p-1, p-2}
  e   x at the edges and every malformed form: smallest / largest x on the curve, 0, p - 1, x >= p (p, p+1, p + x_good, 2^(8L-2) - 1,
      each spare bit below the flags), infinity with each single bit of x set, infinity with the sign flag
  r   (BLS12-377) random points of the prime-order subgroup
  t   (BLS12-377) torsion: the three points of order 2 (rhs = 0), (0, +-1) of order 3, a point of every small prime order dividing the
      cofactor, subgroup-plus-torsion mixtures -- all refused
On BLS12-377 (cofactor != 1) a point with prescribed y is almost never in the prime-order subgroup, so families a and b are NOT
observable there (the decoders refuse such a point whatever the square root gave): the digit coverage on that field comes from random
subgroup points, counted by the reference discrete logarithm, and families c, d, e are kept (d through the compress direction).

Expected verdicts and bytes come from the oracle (ark_canonical.dec_point / enc_point); for constructed points they also come from the
construction, and `_Builder` asserts that the two agree."""
import random
import time

import ark_canonical as ac
import mp_oracle as po


# ---- polynomials over F_p: coefficient lists, low degree first ------------------------------------------------------------------------
def _trim(f):
    while f and f[-1] == 0:
        f.pop()
    return f


def _pdivmod(f, m, p):
    f, dm = list(f), len(m) - 1
    inv = pow(m[-1], -1, p)
    quo = [0] * max(len(f) - dm, 0)
    for i in range(len(f) - 1, dm - 1, -1):
        c = f[i] * inv % p
        quo[i - dm] = c
        if c:
            for j in range(dm + 1):
                f[i - dm + j] = (f[i - dm + j] - c * m[j]) % p
    return _trim(quo), _trim(f[:dm])


def _pmulmod(f, g, m, p):
    h = [0] * (len(f) + len(g) - 1) if f and g else []
    for i, a in enumerate(f):
        for j, b in enumerate(g):
            h[i + j] = (h[i + j] + a * b) % p
    return _pdivmod(h, m, p)[1]


def _ppowmod(f, e, m, p):
    r, f = [1], _pdivmod(f, m, p)[1]
    for bit in bin(e)[2:]:
        r = _pmulmod(r, r, m, p)
        if bit == "1":
            r = _pmulmod(r, f, m, p)
    return r


def _pgcd(f, g, p):
    f, g = _trim(list(f)), _trim(list(g))
    while g:
        f, g = g, _pdivmod(f, g, p)[1]
    inv = pow(f[-1], -1, p) if f else 0
    return [c * inv % p for c in f]


def _linear_roots(m, p, rng):
    """roots of a monic product of distinct linear factors"""
    if len(m) <= 1:
        return []
    if len(m) == 2:
        return [(-m[0]) % p]
    while True:
        s = rng.randrange(p)
        h = _ppowmod([s, 1], (p - 1) // 2, m, p)
        h = _trim([(h[0] - 1) % p] + h[1:]) if h else [p - 1]
        d = _pgcd(m, h, p)
        if 1 < len(d) < len(m):
            return _linear_roots(d, p, rng) + _linear_roots(_pdivmod(m, d, p)[0], p, rng)


def cubic_roots(cv, r, rng=None):
    """all x in F_p with x^3 + a x + b = r"""
    p = cv.p
    m = [(cv.b - r) % p, cv.a % p, 0, 1]
    xp = _ppowmod([0, 1], p, m, p) + [0, 0]
    xp[1] = (xp[1] - 1) % p
    return sorted(_linear_roots(_pgcd(m, _trim(xp), p), p, rng or random.Random(r)))


# ---- the 2-Sylow subgroup of F_p^* -----------------------------------------------------------------------------------------------------
class Sylow:
    def __init__(self, p):
        self.p, self.S, self.q = p, 0, p - 1
        while self.q % 2 == 0:
            self.S, self.q = self.S + 1, self.q // 2
        z = 2
        while pow(z, (p - 1) // 2, p) != p - 1:
            z += 1
        self.g = pow(z, self.q, p)
        self.w = 4 if self.S % 4 == 0 else (2 if self.S % 2 == 0 else 1)
        self.k, self.nd = self.S // self.w, 1 << self.w
        self.qinv = pow(self.q, -1, 1 << self.S)
        ginv = pow(self.g, -1, p)
        self._ginv_pow = [pow(ginv, 1 << b, p) for b in range(self.S)]

    def dlog(self, a):
        """E in [0, 2^S) with (a^q) = g^E, one bit at a time: bit b of E is set iff (t g^-(E mod 2^b))^(2^(S-1-b)) != 1"""
        p, cur, E = self.p, pow(a, self.q, self.p), 0
        for b in range(self.S):
            if pow(cur, 1 << (self.S - 1 - b), p) != 1:
                E |= 1 << b
                cur = cur * self._ginv_pow[b] % p
        assert cur == 1
        return E

    def digits(self, E):
        return [(E >> (self.w * i)) & (self.nd - 1) for i in range(self.k)]

    def from_digits(self, ds):
        return sum(d << (self.w * i) for i, d in enumerate(ds))

    def odd_order(self, rng):
        return pow(rng.randrange(2, self.p), 1 << self.S, self.p)


def first_nonzero(ds):
    return next((i for i, d in enumerate(ds) if d), None)


def first_diff_limb(y, p, nw, bits=32):
    """the highest limb in which y and p - y differ (the limb that decides `y > -y`)"""
    m = (1 << bits) - 1
    return next(i for i in range(nw - 1, -1, -1) if (y >> (bits * i)) & m != ((p - y) >> (bits * i)) & m)


def possible_diff_limbs(p, nw, bits=32):
    """The limbs that CAN be the first difference of y and p - y (0 < y < p).  If the limbs at and above `lvl` agree, the low parts sum
    to (p mod B^lvl) + c B^lvl with c the carry the equal high limbs need (2 T + c = p >> (bits lvl)).  At limb lvl - 1 the two digits
    sum to V = (that sum >> bits (lvl-1)) - c', c' the carry out of the lower limbs: they can differ iff 1 <= V <= 2 B - 3 and can be
    equal iff V is even.  (On the STARK prime 2^251 + 17 2^192 + 1 this leaves limbs 7, 6, 5 and 0: limbs 1 .. 4 of p are zero and
    force y and p - y to agree there once they agree above.)"""
    B, res, states, seen = 1 << bits, set(), [(nw, 0)], set()
    while states:
        lvl, c = states.pop()
        if (lvl, c) in seen or lvl == 0:
            continue
        seen.add((lvl, c))
        ssum = p % B ** lvl + c * B ** lvl
        for c2 in (0, 1):
            lowmax = 2 * (B ** (lvl - 1) - 1)
            low = ssum % B ** (lvl - 1) + c2 * B ** (lvl - 1)
            V = (ssum >> (bits * (lvl - 1))) - c2
            if low > lowmax or V < 0 or V > 2 * (B - 1):
                continue
            if 1 <= V <= 2 * B - 3:
                res.add(lvl - 1)
            if V % 2 == 0:
                states.append((lvl - 1, c2))
    return res


# ---- the pool -------------------------------------------------------------------------------------------------------------------------
class Entry:
    __slots__ = ("enc", "fam", "note", "ok", "wire", "P", "x", "E")

    def __repr__(self):
        return "<%s %s %s %s>" % (self.fam, self.note, "ok" if self.ok else "refused", self.enc.hex())


class _Builder:
    def __init__(self, cv, seed):
        self.cv, self.sy, self.rng, self.L, self.out = cv, Sylow(cv.p), random.Random(seed), ac.compressed_len(cv), []
        self.nw = cv.fq_bytes // 4

    def rhs(self, x):
        cv = self.cv
        return (x * x * x + cv.a * x + cv.b) % cv.p

    def raw(self, enc, fam, note, P=None):
        """an encoding whose verdict is the oracle decoder's; P = the curve point it stands for, if it stands for one"""
        cv, e = self.cv, Entry()
        e.enc, e.fam, e.note, e.P, e.x, e.E = bytes(enc), fam, note, P, None, None
        try:
            Q = ac.dec_point(cv, e.enc)
            e.ok, e.wire = True, po.pt_wire(Q)
            if P is not None:
                assert Q == P, ("oracle and construction disagree", e)
        except ac.DecodeError:
            e.ok, e.wire = False, bytes(po.point_bytes())
        # does this input reach a square root?  (canonical x, no infinity flag, rhs != 0)
        x = int.from_bytes(enc[:-1] + bytes([enc[-1] & 0x3F]), "little")
        if not enc[-1] & 0x40 and x < cv.p and self.rhs(x):
            e.x, e.E = x, self.sy.dlog(self.rhs(x))
        self.out.append(e)
        return e

    def point(self, P, fam, note, must=None):
        """both encodings of +-P = (x, +-y), P on the curve"""
        cv = self.cv
        assert cv.is_on_curve(P)
        for Q in (P, po.pt_neg(cv, P)) if P[1] else (P,):
            e = self.raw(ac.enc_point(cv, Q), fam, note, Q)
            assert must is None or e.ok == must, e
        return e

    def refused(self, enc, fam, note):
        e = self.raw(enc, fam, note)
        assert not e.ok, ("the oracle decoder accepts a case meant to be refused", e)

    def x_for_rhs(self, r):
        xs = cubic_roots(self.cv, r, self.rng)
        return self.rng.choice(xs) if xs else None

    def with_log(self, E, fam, note, must=None):
        """a point (residue, E even) or a refused x (non-residue, E odd) whose rhs^q = g^E"""
        sy, p = self.sy, self.cv.p
        while True:
            o = sy.odd_order(self.rng)
            if E % 2 == 0:
                y = pow(sy.g, (E // 2) * sy.qinv % (1 << sy.S), p) * o % p
                x = self.x_for_rhs(y * y % p)
                if x is not None:
                    e = self.point((x, y), fam, note, must)
                    assert e.E == E, (e, E)
                    return
            else:
                x = self.x_for_rhs(pow(sy.g, E * sy.qinv % (1 << sy.S), p) * o % p)
                if x is not None:
                    for flag in (0, 0x80):
                        enc = bytearray(x.to_bytes(self.L, "little"))
                        enc[-1] |= flag
                        self.refused(enc, fam, note)
                        assert self.out[-1].E == E
                    return

    def rand_digits(self, lo):
        """random digits for the windows lo .. k-1 (zeros below)"""
        sy = self.sy
        return [0] * lo + [self.rng.randrange(sy.nd) for _ in range(sy.k - lo)]


def _family_a(b, must):
    sy = b.sy
    for i in range(sy.k):
        if i == 0 and sy.w == 1:
            continue                                         # a square has e_0 even: with 1-bit windows window 0 is always 0
        for n in range(4):
            ds = b.rand_digits(i)
            ds[i] = 2 * b.rng.randrange(1, sy.nd // 2) if i == 0 else b.rng.randrange(1, sy.nd)
            b.with_log(sy.from_digits(ds), "a", "first non-zero window %d" % i, must)
    for n in range(4):
        b.with_log(0, "a", "odd order: every digit 0", must)


def _family_b(b, must):
    sy, mx = b.sy, b.sy.nd - 1
    even0 = lambda ds: [ds[0] & ~1] + ds[1:]
    b.with_log(sy.from_digits(even0([mx] * sy.k)), "b", "all digits maximal (e_0 even)", must)
    b.with_log(sy.from_digits(even0([1] * sy.k)), "b", "all digits 1 (e_0 = 0)", must)
    for i in range(sy.k):
        d = 2 * b.rng.randrange(1, sy.nd // 2) if i == 0 and sy.w > 1 else (0 if i == 0 else b.rng.randrange(1, sy.nd))
        b.with_log(d << (sy.w * i), "b", "single non-zero digit at window %d" % i, must)
    for ph in (0, 1):
        b.with_log(sy.from_digits(even0([mx if (i + ph) % 2 else 0 for i in range(sy.k)])), "b", "alternating 0 / max, phase %d" % ph, must)
    if sy.w > 1:
        b.with_log(2, "b", "e_0 = 2 only", must)
    for s in range(sy.nd):                                   # every (window >= 1, digit) twice, every even e_0 at least twice
        for rep in range(2):
            ds = [(2 * s) % sy.nd] + [(s + i) % sy.nd for i in range(1, sy.k)]
            b.with_log(sy.from_digits(even0(ds)), "b", "sweep s = %d" % s)


def _family_c(b):
    sy, mx = b.sy, b.sy.nd - 1
    odd = list(range(1, sy.nd, 2))
    per = max(64 // len(odd), 2)                             # 32 x-values = 64 encodings in all
    for d in odd:
        for n in range(per // 2):
            ds = b.rand_digits(1) if n % 2 else [0] * sy.k
            ds[0] = d
            b.with_log(sy.from_digits(ds), "c", "non-residue, e_0 = %d, higher digits %s" % (d, "random" if n % 2 else "0"))
    b.with_log(sy.from_digits([mx] * sy.k), "c", "non-residue, all digits maximal")
    b.with_log(sy.from_digits([1] * sy.k), "c", "non-residue, all digits 1")


def _family_d(b):
    cv, p, nw = b.cv, b.cv.p, b.nw
    for i in range(nw):
        # y = (p-1)/2 - D and p - y = (p+1)/2 + D: D = 0, 1, 2 .. for the lowest limb; steps of half a limb plus a few units above it
        # (a modulus whose limbs are all ones, as secp256k1's, leaves only D near 2^(32 i - 1) without a carry into the limbs above)
        # six points per limb: whichever root the square root returns first, some point has the other one as its answer
        cands = range(64) if i == 0 else (d << (32 * i - 1) | e for d in range(1, 65) for e in range(8))
        found = 0
        for D in cands:
            y = (p - 1) // 2 - D
            if i == 0 and first_diff_limb(y, p, nw) != 0:
                # y and p - y agree above limb 0 only for D below the first borrow out of limb 0 (the carry into limb 1 is fixed by
                # the parity of p >> 32): the candidates are exhausted and none of them is on the curve
                if not found:
                    EMPTY_LIMBS.setdefault(cv.name, set()).add(0)
                break
            x = b.x_for_rhs(y * y % p) if y > 0 and first_diff_limb(y, p, nw) == i else None
            if x is not None:
                b.point((x, y), "d", "y = (p-1)/2 - 0x%x: first difference in limb %d" % (D, i))
                found += 1
                if found == 6:
                    break
    for y in (1, 2):
        x = b.x_for_rhs(y * y % p)
        if x is not None:
            b.point((x, y), "d", "y = +-%d" % y)


def _family_e(b):
    cv, p, L = b.cv, b.cv.p, b.L
    top = 8 * L - 2                                          # bits of x in the encoding
    enc = lambda v, flag=0: v.to_bytes(L, "little")[:-1] + bytes([(v >> (8 * (L - 1))) | flag])
    on_curve = lambda x: po.fq_sqrt(cv, b.rhs(x)) is not None
    lo = next(x for x in range(p) if on_curve(x))
    hi = next(x for x in range(p - 1, 0, -1) if on_curve(x))
    for x, note in ((lo, "smallest x on the curve"), (hi, "largest x on the curve"), (0, "x = 0"), (p - 1, "x = p - 1")):
        for flag in (0, 0x80):
            b.raw(enc(x, flag), "e", note)
    xg = next(x for x in range(1, p) if on_curve(x))
    for v, note in ((p, "x = p"), (p + 1, "x = p + 1"), (p + xg, "x = p + (a small x on the curve)"), (p + cv.G[0], "x = p + G.x"),
                    ((1 << top) - 1, "x = 2^(8L-2) - 1")):
        if v < 1 << top:
            for flag in (0, 0x80):
                b.refused(enc(v, flag), "e", note)
    for bit in range(p.bit_length(), top):                   # spare bits below the flags, one at a time, on good points
        for P in (cv.G, po.pt_neg(cv, cv.G)):
            b.refused(enc(P[0] | 1 << bit, 0x80 if P[1] > p - P[1] else 0), "e", "spare bit %d set on a good point" % bit)
        b.refused(enc(1 << bit), "e", "x = 2^%d" % bit)
    if 8 * (L - 1) >= p.bit_length():                        # a whole spare byte (secp256k1): x in [p, 2^256) in the bytes below it
        for v in (p, p + xg, (1 << 8 * (L - 1)) - 1):
            b.refused(enc(v), "e", "x >= p below the spare byte")
    b.raw(ac.enc_point(cv, None), "e", "infinity")
    assert b.out[-1].ok
    b.refused(enc(0, 0xC0), "e", "infinity with the sign flag")
    for bit in range(top):
        b.refused(enc(1 << bit, 0x40), "e", "infinity with bit %d of x set" % bit)


def _small_prime_factors(n, bound=1 << 12):
    return [l for l in range(2, bound) if n % l == 0 and all(l % d for d in range(2, int(l ** 0.5) + 1))]


def _family_rt(b, n_random):
    cv, p, h = b.cv, b.cv.p, po.COFACTOR[b.cv.name]
    for _ in range(n_random):
        b.point(po.pt_mul(cv, b.rng.randrange(1, cv.q), cv.G), "r", "random subgroup point", True)
    for x in cubic_roots(cv, 0, b.rng):                       # rhs = 0: the points of order 2, y = 0
        for flag in (0, 0x80):
            e = bytearray(x.to_bytes(b.L, "little"))
            e[-1] |= flag
            b.refused(e, "t", "order 2 (rhs = 0)")
    assert sum(1 for e in b.out if e.note.startswith("order 2")) == 6, "x^3 + a x + b has three roots on this curve"
    for flag in (0, 0x80):
        b.refused(bytes(b.L - 1) + bytes([flag]), "t", "(0, +-1): order 3")
    for l in _small_prime_factors(h):
        v = 0
        while (h // l ** v) % l == 0:
            v += 1
        while True:
            x = b.rng.randrange(p)
            y = po.fq_sqrt(cv, b.rhs(x))
            T = po.pt_mul_raw(cv, (h // l ** v) * cv.q, (x, y)) if y is not None else None
            if T is not None:
                break
        while po.pt_mul_raw(cv, l, T) is not None:
            T = po.pt_mul_raw(cv, l, T)
        b.point(T, "t", "order %d" % l, False)
        b.point(po.pt_add(cv, T, po.pt_mul(cv, b.rng.randrange(1, cv.q), cv.G)), "t", "subgroup point + a point of order %d" % l, False)


_POOLS = {}
BUILD_SECONDS = {}
EMPTY_LIMBS = {}          # curve -> limbs that can decide `y > -y` for integers but, provably, for no point of the curve (family d)


def pool(curve, n_random=200):
    """the pool of a curve (built once per process): a list of Entry"""
    key = (curve, n_random)
    if key not in _POOLS:
        cv, t0 = po.CURVES[curve], time.time()
        with po.curve_ctx(cv):
            b = _Builder(cv, 0xDEC0 + cv.cid)
            prime_order = cv.name not in po.COFACTOR
            if prime_order:
                _family_a(b, True)
                _family_b(b, True)
            _family_c(b)
            _family_d(b)
            _family_e(b)
            if not prime_order:
                _family_rt(b, n_random)
        _POOLS[key], BUILD_SECONDS[key] = b.out, time.time() - t0
    return _POOLS[key]


def coverage(curve, entries):
    """what the entries reach, from the reference discrete logarithm alone"""
    cv = po.CURVES[curve]
    sy, nw = Sylow(cv.p), cv.fq_bytes // 4
    cov = dict(first=set(), first_enc={}, ghalf={}, rr={}, limbs=set(), limbs_decoded=set(), fams={}, odd_e0=set(), refused_nonres=0)
    for e in entries:
        cov["fams"].setdefault(e.fam, set()).add(e.note)
        if e.P is not None and e.P[1]:
            cov["limbs"].add(first_diff_limb(e.P[1], cv.p, nw))
            if e.ok:
                cov["limbs_decoded"].add(first_diff_limb(e.P[1], cv.p, nw))
        if e.E is None:
            continue
        ds = sy.digits(e.E)
        if e.E % 2 == 0 and e.ok:
            cov["first"].add(first_nonzero(ds))
            cov["first_enc"].setdefault(first_nonzero(ds), set()).add((e.x, e.enc[-1] & 0x80))
        if e.E % 2:
            cov["odd_e0"].add(ds[0])
            cov["refused_nonres"] += 1
        for i, d in enumerate(ds):
            cov["ghalf"][(i, d)] = cov["ghalf"].get((i, d), 0) + 1
            for c in range(2, sy.k - i + 1):                 # window i' = c - 1 + i multiplies by R[c][e_i]
                cov["rr"][(c, d)] = cov["rr"].get((c, d), 0) + 1
    return cov


def assert_coverage(curve, entries):
    """the full sets the pool is built for: a property that is checked, not hoped for"""
    cv = po.CURVES[curve]
    sy, nw, cov = Sylow(cv.p), cv.fq_bytes // 4, coverage(curve, entries)
    prime_order = cv.name not in po.COFACTOR
    possible = possible_diff_limbs(cv.p, nw) - EMPTY_LIMBS.get(cv.name, set())
    pairs = {(i, d) for i in range(sy.k) for d in range(sy.nd)}
    assert {kk for kk, n in cov["ghalf"].items() if n >= 2} == pairs, sorted(pairs - set(cov["ghalf"]))
    rr = {(c, d) for c in range(2, sy.k + 1) for d in range(sy.nd)}
    assert {kk for kk, n in cov["rr"].items() if n >= 2} == rr
    assert cov["odd_e0"] == set(range(1, sy.nd, 2)) and cov["refused_nonres"] >= 64
    if prime_order:
        want = {i for i in range(sy.k) if i or sy.w > 1} | {None}
        assert cov["first"] == want, sorted(want - cov["first"], key=str)
        for i, encs in cov["first_enc"].items():            # at least four x values, each with both sign flags
            assert len({x for x, _ in encs}) >= 4 and all((x, fl ^ 0x80) in encs for x, fl in encs), (i, encs)
        assert cov["limbs_decoded"] == possible, (cov["limbs_decoded"], possible)
    else:
        assert {"order 2 (rhs = 0)", "(0, +-1): order 3"} <= cov["fams"]["t"]
        for l in _small_prime_factors(po.COFACTOR[cv.name]):
            assert {"order %d" % l, "subgroup point + a point of order %d" % l} <= cov["fams"]["t"]
    assert cov["limbs"] == possible, (cov["limbs"], possible)
    notes = cov["fams"]["e"]
    for want in ("smallest x on the curve", "largest x on the curve", "x = 0", "x = p - 1", "x = p", "x = p + 1", "x = 2^(8L-2) - 1",
                 "infinity", "infinity with the sign flag", "infinity with bit 0 of x set"):
        assert want in notes, want
    assert sum(1 for n in notes if n.startswith("infinity with bit")) == 8 * ac.compressed_len(cv) - 2
    return cov
