"""Cases, references and checks for the split bucket pipeline (kernels_bucket.hpp: k_bucket_sort, k_bucket_acc, k_bucket_list,
k_bucket_reduce, k_bucket_final) at its structural edges, through the public mp_msm with mp_set_bucket_min / _bits / _split.  Shared by
tests/test_bucket_split_emu.py (the kernel bodies under the development emulator, CPU) and tests/test_gpu_bucket_split.py (gfx950) --
same constructions, same expectations, the canonical result point compared byte for byte.

The rules the cases lean on (kernels_bucket.hpp): terms are sorted in chunks of BK_CHUNK, so a bucket is G = ceil(kpad / chunk) short
runs; an item -- one window of one MSM -- is summed in list mode when the largest bucket of any of its chunks exceeds
T = 8 (chunk / 2^(c-1)) + 32, else in bucket mode by `units` waves of NBP = 64 x 4 buckets each; list mode cuts every run into 64
equal shares; the reduction works in quarters of Q buckets; above 4 096 buckets the sort's counters are packed 16-bit halves.  The
expressions are copied by hand below and tied to the source text (geometry_is_the_engines).

Points: every case draws from 12 distinct points of eng.setup, their negatives and the point at infinity, so the expected result of
a K-term MSM is an MSM of 12 terms with the scalars folded per point modulo q (signs included): the C++ oracle's, and for the first
case of every family and width the Python oracle's big-integer group law too.
Scalars: built from intended digits -- the window under test is written into random bits so that the signed digit of
digit_cases.model_bucket comes out as intended (the two bits below the window are cleared: no carry comes in; the value stays below
q / 2: no flip unless asked for).  self_check() recomputes every (window, chunk) histogram of |digit| from that model and asserts that
the case reaches the edge it is named for: a construction that silently missed its edge fails there, without an engine.

Not reachable through the public entry points today, and not tested: a phase whose bucket jobs have different chunk counts (the
`g >= bk_chunks(job.kpad)` return of k_bucket_sort) -- mp_msm builds one job per call, the verifier's equations of a pass are equal.

Every family runs at every width of its curve (WIDTHS): the constructions are vectorised and none had to be cut for time.

Every run_* function returns (failure messages, number of checks); no case is skipped or excused."""
import os

import numpy as np

import digit_cases as dc
import mp_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_GPU = 24576               # BK_CHUNK of the shipped engine
CHUNK_EMU = 1024                # the second emulator library (tools/hostemu: make CHUNK=1024)
CHUNKS_MAX = 24
LDS_CAPS = (64 * 1024, 160 * 1024)   # bytes of LDS a workgroup may be offered: what rt.hpp assumes when the device does not say, and a CDNA4 CU's
FAMILIES = ("A", "B", "C", "D", "E", "F", "G")
# curve -> window widths.  12 bits and more are the split pipeline by default (11 on BLS12-377); set_bucket_split(min(c, 12)) puts the
# narrower ones there as well
WIDTHS = {"stark": (10, 12, 13, 14), "bls12_377": (11, 13), "secp256k1": (12,)}
NPTS = 12
INF = 2 * NPTS                  # point index: 0 .. 11 the pool, 12 .. 23 their negatives, 24 the point at infinity
M64 = (1 << 64) - 1

# ---- the engine's geometry, copied by hand ------------------------------------------------------------------------------------------
GEOMETRY_SOURCE = {
    "mental-poker_amd/csrc/kernels_bucket.hpp": (
        "#define MP_EXP_BK_CHUNK 24576",
        "static const uint32_t BK_CHUNK = MP_EXP_BK_CHUNK;",
        "static const uint32_t BK_CHUNKS_MAX = 24;",
        "MP_HD uint32_t bk_buckets(uint32_t c) { return 1u << (c - 1); }",
        "#define MP_EXP_BK_UNIT_NB 4",
        "MP_HD uint32_t bk_unit_nb(uint32_t c) { return bk_buckets(c) >= 64u * MP_EXP_BK_UNIT_NB ? (uint32_t)MP_EXP_BK_UNIT_NB : bk_buckets(c) / 64u; }",
        "MP_HD uint32_t bk_units(uint32_t c) { return bk_buckets(c) / (64u * bk_unit_nb(c)); }",
        "MP_HD uint32_t bk_chunks(uint32_t kpad) { return (kpad + BK_CHUNK - 1u) / BK_CHUNK; }",
        "MP_HD bool bk_crowded(uint32_t largest, uint32_t c) { return largest > 8u * (BK_CHUNK / bk_buckets(c)) + 32u; }",
        "MP_HD bool bk_sort_packed(uint32_t c) { return bk_buckets(c) > 4096u; }",
        "const uint32_t NBK = bk_buckets(a.bits), Q = NBK >> 2, NB = Q >> 6;",
        "const uint32_t i = wave / a.wpb, lane_wave = wave % a.wpb, per = (a.wgs + 7u) / 8u;",
        "  return std::max(gmax * (nbp + 2u) / 2u + nbp + nbp + 64u * pw, 64u * xw);",
    ),
    "mental-poker_amd/csrc/engine_core.hpp": (
        "const uint32_t acc_lds = bk_acc_lds_words(c, gmax, XW, G_::PW), wpb = rt::waves_per_block(acc_lds), wgs = (items * units + wpb - 1) / wpb;",
        'ctx->prof.begin("k_bucket_sort", s, (uint64_t)items * gmax);',
    ),
    "mental-poker_amd/csrc/layout.hpp": (
        "const uint32_t kpad = (uint32_t)((v_.size() + 63) / 64 * 64);",
    ),
    "mental-poker_amd/csrc/rt.hpp": (
        "      b = 64 * 1024;",
        "  const size_t bytes = lds_words * 4, cap = lds_per_workgroup();",
        "  uint32_t wpb = 4;",
        "  while (wpb > 1 && wpb * bytes > cap / 2) wpb >>= 1;",
    ),
    "tools/hostemu/rt.hpp": (
        "inline uint32_t waves_per_block(size_t) { return 4; }",
    ),
    "tools/hostemu/Makefile": (
        "DEFS := -DMP_EXP_BK_CHUNK=$(CHUNK)",
        "LIB := libmpemu_chunk$(CHUNK).so",
    ),
}


def geometry_is_the_engines():
    """-> the lines of GEOMETRY_SOURCE that the source no longer has (none: Geo below is the engine's arithmetic)"""
    missing = []
    for name, lines in GEOMETRY_SOURCE.items():
        with open(os.path.join(ROOT, name)) as f:
            text = f.read()
        missing += ["%s: %s" % (name, ln) for ln in lines if ln not in text]
    return missing


class Geo:
    def __init__(self, c, chunk):
        self.c, self.chunk = c, chunk
        self.NBK = 1 << (c - 1)                            # bk_buckets
        self.T = 8 * (chunk // self.NBK) + 32              # bk_crowded: list mode above this
        self.NBP = 64 * min(4, self.NBK // 64)             # 64 x bk_unit_nb
        self.units = self.NBK // self.NBP                  # bk_units
        self.Q = self.NBK // 4                             # k_bucket_reduce's quarters
        self.packed = self.NBK > 4096                      # bk_sort_packed

    def waves_per_workgroup(self, curve, G, cap):
        """units per workgroup of the k_bucket_acc launch: rt.hpp waves_per_block(bk_acc_lds_words(c, gmax, XW, PW)) with `cap` bytes of
        LDS per workgroup; cap = None: the emulator's, always 4"""
        if cap is None:
            return 4
        fw = 14 if curve == "bls12_377" else 9             # 29-bit limbs of a base-field element; a point is 2, an XYZZ sum 4 of them
        words = max(G * (self.NBP + 2) // 2 + 2 * self.NBP + 64 * 2 * fw, 64 * 4 * fw)
        wpb = 4
        while wpb > 1 and wpb * words * 4 > cap // 2:
            wpb >>= 1
        return wpb

    def chunks(self, K):
        return -(-(-(-K // 64) * 64) // self.chunk)        # bk_chunks(kpad), kpad = K rounded up to 64


# ---- scalars from intended digits ---------------------------------------------------------------------------------------------------
def _mask_limbs(v):
    return [np.uint64((v >> (64 * i)) & M64) for i in range(4)]


def _set_bits(l, pos, n, val):
    """bits [pos, pos + n) of every row := val (uint64 array, < 2^n)"""
    i, sh, m = pos >> 6, pos & 63, (1 << n) - 1
    l[:, i] = (l[:, i] & np.uint64(~(m << sh) & M64)) | (val << np.uint64(sh))
    if sh + n > 64:
        l[:, i + 1] = (l[:, i + 1] & np.uint64(~(m >> (64 - sh)) & M64)) | (val >> np.uint64(64 - sh))


def q_minus(l, q):
    """q - k on rows of four 64-bit limbs (0 < k < q)"""
    ql = _mask_limbs(q)
    out = np.empty_like(l)
    borrow = np.zeros(len(l), dtype=bool)
    for i in range(4):
        a = l[:, i]
        d = ql[i] - a
        nb = (a > ql[i]) | ((d == 0) & borrow)
        out[:, i] = d - borrow.astype(np.uint64)
        borrow = nb
    assert not borrow.any()
    return out


def to_ints(l):
    raw = np.ascontiguousarray(l, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def from_ints(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).copy()


class Maker:
    """scalars of one (group order, width, chunk)"""

    def __init__(self, curve, c, chunk, seed):
        self.curve, self.q, self.c = curve, dc.order(curve), c
        self.g = Geo(c, chunk)
        self.bits = self.q.bit_length()
        self.nwin = dc.windows(self.q, dc.KIND_BUCKET, c)
        self.rs = np.random.RandomState((seed * 1000003 + c * 131 + chunk) % (1 << 32))
        self.half = (self.q - 1) // 2

    def _raw(self, K, nbits):
        l = self.rs.randint(0, 1 << 63, size=(K, 4), dtype=np.uint64) ^ (self.rs.randint(0, 2, size=(K, 4), dtype=np.uint64) << np.uint64(63))
        keep = _mask_limbs((1 << nbits) - 1)
        for i in range(4):
            l[:, i] &= keep[i]
        return l

    def random(self, K):
        """uniform below 2^(bits - 1) < q, every third one negated: both recodings (k and q - k) on every curve"""
        l = self._raw(K, self.bits - 1)
        l[:, 0] |= (l == 0).all(axis=1).astype(np.uint64)      # (never zero)
        rows = np.arange(K) % 3 == 2
        if rows.any():
            l[rows] = q_minus(l[rows], self.q)
        return l

    def top_cap(self):
        """the largest digit the top window takes under digits(): d 2^s <= (q - 1) / 2"""
        return self.half >> (self.c * (self.nwin - 1))

    def digits(self, w, d, flips=None):
        """one scalar per entry of d (signed digits, |d| <= 2^(c-1) - 1 or -2^(c-1); the top window: 0 .. top_cap()): window w holds
        that digit in the sense of digit_cases.model_bucket, the other windows are random.  flips: rows that become q - k, whose
        digits are stored negated"""
        d = np.asarray(d, dtype=np.int64)
        K, c, NBK = len(d), self.c, self.g.NBK
        top = w == self.nwin - 1
        assert d.min() >= (0 if top else -NBK) and d.max() <= (self.top_cap() if top else NBK - 1), (w, int(d.min()), int(d.max()))
        l = self._raw(K, self.bits - 2)                    # below (q - 1) / 2 on every curve: no flip
        raw = (d & ((1 << c) - 1)).astype(np.uint64)
        s = c * w
        if w == 0:
            _set_bits(l, 0, c, raw)
        elif not top:
            _set_bits(l, s - 2, c + 2, raw << np.uint64(2))      # (the window below stays under 2^(c-2): no carry comes in)
        else:
            keep = _mask_limbs((1 << (s - 2)) - 1)
            for i in range(4):
                l[:, i] &= keep[i]
            _set_bits(l, s, min(c, 256 - s), raw)
            for v in np.unique(d):
                room = self.half - (int(v) << s)
                assert room > 0
                lb = room.bit_length() - 1                 # the low part stays below 2^lb <= room
                if v and lb < s - 2:
                    rows = d == v
                    m = _mask_limbs(((1 << lb) - 1) | (((1 << 256) - 1) >> s << s))
                    for i in range(4):
                        l[rows, i] &= m[i]
        l[:, 0] |= (l == 0).all(axis=1).astype(np.uint64)
        if flips is not None and flips.any():
            l[flips] = q_minus(l[flips], self.q)
        return l

    def spread(self, K, w, avoid=()):
        """background digits of window w: random over all buckets and both signs (the top window: a few of every value it takes,
        then zeros), never a bucket of `avoid`"""
        NBK = self.g.NBK
        if w == self.nwin - 1:
            cap, T = self.top_cap(), self.g.T
            j = np.arange(K) % self.g.chunk
            d = np.where(j < (T // 2) * (cap + 1), j % (cap + 1), 0).astype(np.int64)
        else:
            d = self.rs.randint(-NBK, NBK, size=K).astype(np.int64)
        for b in avoid:
            d[np.abs(d) == b] = 0
        return d


class Case:
    """one call: `msms` MSMs of K terms each -- (scalar limbs [K][4], point index [K]) -- and the edge that MSM `at`, window `w`
    is built to reach: mode ('list' / 'bucket'), largest (bucket of any chunk, exactly), G, tu {chunk: terms with a non-zero
    digit}, nonempty (exactly these buckets), runs {bucket: terms per chunk}, modes {msm: mode}, inf (the result is infinity)"""

    def __init__(self, name, c, msms, w=None, at=0, intended=None, **edge):
        self.name, self.c, self.msms, self.w, self.at, self.intended, self.edge = name, c, msms, w, at, intended, edge
        self.K = len(msms[0][1])
        assert all(len(p) == self.K and len(l) == self.K for l, p in msms)


def _pts_random(mk, K):
    return mk.rs.randint(0, 2 * NPTS + 1, size=K)


def _place(mk, K, where, d_crowd, w, avoid):
    """background digits with d_crowd written at the positions `where`"""
    d = mk.spread(K, w, avoid)
    d[np.asarray(where)] = d_crowd
    return d


def _positions(mk, lo, hi, n):
    return lo + mk.rs.permutation(hi - lo)[:n]


def _window_positions(mk):
    return (("window 0", 0), ("middle window", mk.nwin // 2), ("top window", mk.nwin - 1))


def _target(mk, w):
    """the digit a crowd sits on: 1 in the top window (the one value every curve and width has there), a negative one in window 0"""
    if w == mk.nwin - 1:
        return 1
    return -77 if w == 0 else mk.g.NBK // 2 + 3


def _one(mk, name, w, d, pidx=None, flips=None, **edge):
    l = mk.digits(w, d, flips)
    want = np.asarray(d, dtype=np.int64)
    if flips is not None:
        want = np.where(flips, -want, want)
    return Case(name, mk.c, [(l, _pts_random(mk, len(d)) if pidx is None else np.asarray(pidx))], w=w, intended=want, **edge)


# ---- the families -------------------------------------------------------------------------------------------------------------------
def family_A(curve, c, chunk, below_chunk_only=False):
    mk = Maker(curve, c, chunk, 1)
    q, ch = mk.q, chunk
    Ks = [1, 7, 8, 9, 63, 64, 65, ch - 1, ch, ch + 1, ch + 8, 2 * ch - 1, 2 * ch, 2 * ch + 1]
    if below_chunk_only:
        Ks = [k for k in Ks if k <= ch]                    # one run per bucket: up to a full chunk of 24 576 terms
    front = from_ints([0, 1, q - 1])

    def msm(K):
        l = mk.random(K)
        l[:min(K, 3)] = front[:min(K, 3)]
        return l, _pts_random(mk, K)
    cases = []
    for K in Ks:
        if K == 1:      # (the smallest bucket_min is 1.  0, 1 and q - 1 as one-term MSMs of one call)
            cases.append(Case("A K = 1 x 3: 0, 1, q - 1", c, [(front[j:j + 1].copy(), np.array([j])) for j in range(3)], G=1))
        else:
            cases.append(Case("A K = %d" % K, c, [msm(K)], G=mk.g.chunks(K)))
    for K in [k for k in (9, ch + 1, 2 * ch + 1) if k in Ks]:
        cases.append(Case("A K = %d x 3" % K, c, [msm(K) for _ in range(3)], G=mk.g.chunks(K)))
    return cases


def family_B(curve, c, chunk):
    mk = Maker(curve, c, chunk, 2)
    T, ch = mk.g.T, chunk
    cases = []
    for wname, w in _window_positions(mk):
        b = _target(mk, w)
        ab = (abs(b),)
        K = 2 * T + 9
        cases.append(_one(mk, "B %s: T terms on one digit" % wname, w, _place(mk, K, _positions(mk, 0, K, T), b, w, ab),
                          mode="bucket", largest=T, G=1, runs={abs(b): [T]}))
        cases.append(_one(mk, "B %s: T + 1 terms on one digit" % wname, w, _place(mk, K, _positions(mk, 0, K, T + 1), b, w, ab),
                          mode="list", largest=T + 1, G=1, runs={abs(b): [T + 1]}))
        K = ch + T
        n0 = T // 2 + 1
        where = np.concatenate([_positions(mk, 0, ch, n0), _positions(mk, ch, K, T + 1 - n0)])
        cases.append(_one(mk, "B %s: T + 1 terms of one digit over two chunks" % wname, w, _place(mk, K, where, b, w, ab),
                          mode="bucket", G=2, runs={abs(b): [n0, T + 1 - n0]}))
        K = 2 * ch + 9
        for what, head, tail_zero in (("the crowd only in chunk 1 of 3", None, False), ("... chunk 2 all zero digits", None, True),
                                      ("... chunk 0 with 1 non-zero digit", 1, False), ("... chunk 0 with 5 non-zero digits", 5, False)):
            d = _place(mk, K, _positions(mk, ch, 2 * ch, T + 1), b, w, ab)
            tu = {}
            if tail_zero:
                d[2 * ch:] = 0
                tu[2] = 0
            if head is not None:
                keep = _positions(mk, 0, ch, head)
                vals = np.array([3, -2, 5, 2, -3][:head]) if w != mk.nwin - 1 else np.array([1] * head)
                d[:ch] = 0
                d[keep] = vals
                tu[0] = head
            # (the crowd's bucket holds nothing outside chunk 1 -- but in the top window, where chunk 0's few digits can only be 1s)
            runs = {abs(b): [head if head and w == mk.nwin - 1 else 0, T + 1, 0]}
            cases.append(_one(mk, "B %s: %s" % (wname, what), w, d, mode="list", largest=T + 1, G=3, tu=tu, runs=runs))
    return cases


def family_C(curve, c, chunk):
    mk = Maker(curve, c, chunk, 3)
    T, NBK, ch = mk.g.T, mk.g.NBK, chunk
    w = mk.nwin // 2
    b = _target(mk, w)
    K = T + 8
    cases = [_one(mk, "C all terms on one digit", w, np.full(K, b), mode="list", largest=K, G=1, nonempty={b})]
    # (halves as equal as they can be with the boundary between the two buckets INSIDE a share: with n terms on each digit it falls between
    # the shares of lanes 31 and 32, and with shares of one term it falls between two shares wherever it is -- so 3 terms per share and more)
    n_up = max(T + 1, 3 * 32)
    n_low = next(n for n in range(n_up + 1, 2 * n_up) if all(((n + n_up) * lane) >> 6 != n for lane in range(65)))
    K = n_low + n_up
    lower = mk.rs.permutation(K) < n_low
    cases.append(_one(mk, "C two adjacent digits, half each", w, np.where(lower, b, b + 1), mode="list", largest=n_low, G=1,
                      nonempty={b, b + 1}, span=1))
    cases.append(_one(mk, "C digits 1 and 2^(c-1) only", w, np.where(lower, 1, -NBK), mode="list", largest=n_low, G=1,
                      nonempty={1, NBK}, span=NBK - 1))
    K = 2 * NBK
    n_sp = K // 4
    d = np.full(K, b)
    where = np.arange(n_sp) * 4 + 1
    sp = 1 + (np.arange(n_sp) * (NBK - 1)) // (n_sp - 1)                     # 1 .. 2^(c-1), both ends included
    d[where] = np.where(sp == NBK, -NBK, np.where(np.arange(n_sp) % 2 == 0, sp, -sp))
    d[where[sp == b]] = b
    cases.append(_one(mk, "C a crowd beside K / 4 terms spread over all buckets", w, d, mode="list", G=mk.g.chunks(K), span=2))
    if mk.g.units < 3:      # (c = 10: two units) three runs on two units: unit 0 takes runs 0 and 2
        K = 2 * ch + 64
        cases.append(_one(mk, "C G > units: crowded in every chunk", w, np.full(K, b), mode="list", G=3, nonempty={b}, more_chunks_than_units=True,
                          runs={b: [ch, ch, 64]}))
    K = T + 8
    cases.append(_one(mk, "C every term the same point", w, np.full(K, b), pidx=np.zeros(K, dtype=np.int64), mode="list", largest=K, G=1))
    cases.append(_one(mk, "C points alternating P, -P", w, np.full(K, b), pidx=np.where(np.arange(K) % 2 == 0, 3, NPTS + 3), mode="list",
                      largest=K, G=1))
    return cases


def family_D(curve, c, chunk, one_chunk_only=False):
    mk = Maker(curve, c, chunk, 4)
    g = mk.g
    T, NBK, NBP, units, Q, ch = g.T, g.NBK, g.NBP, g.units, g.Q, chunk
    w = mk.nwin // 2
    every = np.arange(1, NBK + 1)
    every = np.where(every == NBK, -NBK, every)            # (the last bucket below the top window is the negative digit)
    cases = [_one(mk, "D every bucket once, ONE point", w, every, pidx=np.full(NBK, 5), mode="bucket", largest=1, G=g.chunks(NBK),
                  nonempty=set(range(1, NBK + 1))),
             _one(mk, "D every bucket once, 12 points in rotation", w, every, pidx=np.arange(NBK) % NPTS, mode="bucket", largest=1,
                  G=g.chunks(NBK), nonempty=set(range(1, NBK + 1))),
             _one(mk, "D only bucket 1", w, np.where(np.arange(T) % 3 == 1, -1, 1), mode="bucket", largest=T, G=1, nonempty={1}),
             _one(mk, "D only bucket 2^(c-1)", w, np.full(T, -NBK), mode="bucket", largest=T, G=1, nonempty={NBK})]
    for p in sorted({1, units - 1}):
        four = [Q, Q + 1, NBP * p, NBP * p + 1]
        d = np.array([(v if i % 2 == 0 else -v) for i in range(6) for v in four])
        cases.append(_one(mk, "D only the buckets Q, Q + 1, NBP p, NBP p + 1 (p = %d)" % p, w, d, mode="bucket",
                          largest=6 * max(four.count(v) for v in four), G=1, nonempty=set(four)))      # (c = 11: Q = NBP, the pairs coincide for p = 1)
    u = units // 2
    d = 1 + u * NBP + mk.rs.randint(0, NBP, size=3 * NBP)
    d = np.where(d == NBK, -NBK, d)
    cases.append(_one(mk, "D all terms inside one unit", w, d, mode="bucket", G=1, inside=(1 + u * NBP, (u + 1) * NBP)))
    lane, n = 37, min(T, 20)
    first = 1 + (units - 1) * NBP + 4 * lane
    cases.append(_one(mk, "D one lane's four buckets hold everything", w, np.array([first + j for j in range(4)] * n), mode="bucket", largest=n, G=1,
                      nonempty={first, first + 1, first + 2, first + 3}))
    d = np.repeat(np.arange(1, NBP + 1), 2)
    cases.append(_one(mk, "D all buckets of a unit hold the same count", w, d[mk.rs.permutation(len(d))], mode="bucket", largest=2, G=1,
                      nonempty=set(range(1, NBP + 1))))
    if not one_chunk_only:
        K = 2 * ch + 9
        b = _target(mk, w)
        for what, per in (("one term in every chunk", [1, 1, 1]), ("terms only in the last chunk", [0, 0, 5]), ("terms only in the first chunk", [5, 0, 0])):
            where = np.concatenate([_positions(mk, g0 * ch, min(K, (g0 + 1) * ch), n) for g0, n in enumerate(per)])
            cases.append(_one(mk, "D a bucket with %s" % what, w, _place(mk, K, where, b, w, (b,)), mode="bucket", G=3, runs={b: per}))
    return cases


def family_E(curve, c, chunk):
    mk = Maker(curve, c, chunk, 5)
    T, NBK = mk.g.T, mk.g.NBK
    w = mk.nwin // 2
    b = _target(mk, w)
    P, N, O = 7, NPTS + 7, INF
    seqs = (("P, P", [P, P], None), ("P, P, P", [P, P, P], None), ("P, -P, P", [P, N, P], None), ("O, P, O", [O, P, O], None),
            ("-P under a negative digit", [P, N], [1, -1]))
    cases = []
    for what, seq, signs in seqs:
        # bucket mode: the sequence alone in bucket b, 64 other terms around it
        K = 64 + len(seq)
        where = _positions(mk, 0, K, len(seq))
        d = mk.spread(K, w, (b,))
        d[where] = [b * s for s in (signs or [1] * len(seq))]
        pidx = _pts_random(mk, K)
        pidx[where] = seq
        cases.append(_one(mk, "E bucket mode: %s" % what, w, d, pidx=pidx, mode="bucket", largest=None, G=1, runs={b: [len(seq)]}))
        # list mode: every term on bucket b, the sequence over and over: every share is made of it
        K = T + 8
        rep = np.arange(K) % len(seq)
        d = np.array([b * s for s in (signs or [1] * len(seq))])[rep]
        cases.append(_one(mk, "E list mode: %s" % what, w, d, pidx=np.array(seq)[rep], mode="list", largest=K, G=1, nonempty={b}))
    # s on P and q - s on P: the same |digit| in every window, the two terms cancel in every bucket they meet in -- the whole MSM is O
    for mode, K in (("bucket", 64), ("list", 2 * (T // 2 + 4))):
        half = K // 2
        d = mk.spread(half, w, (b,)) if mode == "bucket" else np.full(half, b)
        if mode == "bucket":
            d[:2] = b
        l = np.repeat(mk.digits(w, d), 2, axis=0)
        flips = np.arange(K) % 2 == 1
        l[flips] = q_minus(l[flips], mk.q)
        pidx = np.repeat(_pts_random(mk, half), 2)
        pidx[pidx == INF] = P
        cases.append(Case("E %s mode: s on P and q - s on P" % mode, c, [(l, pidx)], w=w, intended=np.where(flips, -1, 1) * np.repeat(d, 2),
                          mode=mode, G=1, inf=True))
    # s on P and s on -P, every term: O again
    K = 2 * (T // 2 + 4)
    d = np.full(K // 2, b)
    l = np.repeat(mk.digits(w, d), 2, axis=0)
    pj = np.arange(K // 2) % NPTS
    pidx = np.stack([pj, pj + NPTS], axis=1).reshape(-1)
    cases.append(Case("E list mode: s on P and s on -P", c, [(l, pidx)], w=w, intended=np.repeat(d, 2), mode="list", G=1, inf=True))
    return cases


def family_F(curve, c_hi, c_lo, c_mid, chunk):
    """-> the calls of one table, in order: (case, fresh-table comparison); the first call comes back at the end"""
    ch = chunk
    hi = Maker(curve, c_hi, chunk, 6)
    w0, wm = 0, hi.nwin // 2
    K = 2 * ch + 9
    T = hi.g.T
    b0, bm = _target(hi, w0), _target(hi, wm)
    first = Case("F 3 MSMs of 2 chunk + 9 terms, list items, c = %d" % c_hi, c_hi, [
        (hi.digits(w0, _place(hi, K, _positions(hi, ch, 2 * ch, T + 1), b0, w0, (abs(b0),))), _pts_random(hi, K)),
        (hi.random(K), _pts_random(hi, K)),
        (hi.digits(wm, np.full(K, bm)), _pts_random(hi, K))], w=wm, at=2, mode="list", G=3,
        modes={(0, w0): "list", (2, wm): "list"})
    small_hi = Case("F K = 9, c = %d" % c_hi, c_hi, [(hi.random(9), _pts_random(hi, 9))], G=1)
    lo = Maker(curve, c_lo, chunk, 7)
    small_lo = Case("F K = 9, c = %d" % c_lo, c_lo, [(lo.random(9), _pts_random(lo, 9))], G=1)
    mid = Maker(curve, c_mid, chunk, 8)
    wq = mid.nwin // 2
    two = Case("F K = chunk + 1 in bucket mode, c = %d" % c_mid, c_mid, [(mid.digits(wq, mid.spread(ch + 1, wq)), _pts_random(mid, ch + 1))], w=wq,
               mode="bucket", G=2)
    return [first, small_hi, small_lo, two, first]


def family_G(curve, c, chunk):
    mk = Maker(curve, c, chunk, 9)
    T = mk.g.T
    w = mk.nwin // 2
    b = _target(mk, w)
    K = 2 * T + 9
    cases = []
    for count in (1, 3, 9):
        crowded = count // 2
        msms = []
        for j in range(count):
            n = T + 1 if j == crowded else T - (j % 3)
            msms.append((mk.digits(w, _place(mk, K, _positions(mk, 0, K, n), b, w, (b,))), _pts_random(mk, K)))
        # (nine MSMs of windows up to 12 bits: the launch's workgroups are no multiple of 8 and bk_unit_of_wave's remap has a ragged
        # tail -- on secp256k1 only with four waves per workgroup, which 64 KB of LDS do not give, so nothing is claimed there; at 13 and
        # 14 bits an item's units fill whole multiples of 8 workgroups whatever the count)
        cases.append(Case("G %d MSMs, number %d crowded" % (count, crowded), c, msms, w=w, at=crowded, mode="list", largest=T + 1, G=1,
                          modes={(j, w): ("list" if j == crowded else "bucket") for j in range(count)}, ragged=count == 9 and c <= 12 and curve != "secp256k1"))
    return cases


def f_widths(curve):
    """(c_hi, c_lo, c_mid) of family F on a curve: 14 / 10 / 13 bits on STARK as far as the curve's widths go"""
    ws = WIDTHS[curve]
    return ws[-1], ws[0], ws[-2] if len(ws) > 1 else ws[0]


def cases_of(curve, fam, c, chunk, single_chunk=False):
    """the calls of one family at one width.  single_chunk: what runs against the emulator's production chunk -- A up to one full
    chunk (K = 1 .. 65, chunk - 1 and chunk: the 16-bit local indices of a full sorted run), D and E with one run per bucket"""
    if fam == "A":
        return family_A(curve, c, chunk, below_chunk_only=single_chunk)
    if fam == "D":
        return family_D(curve, c, chunk, one_chunk_only=single_chunk)
    if fam == "F":
        return family_F(curve, *f_widths(curve), chunk)
    return {"B": family_B, "C": family_C, "E": family_E, "G": family_G}[fam](curve, c, chunk)


def family_widths(curve, fam):
    return (WIDTHS[curve][-1],) if fam == "F" else WIDTHS[curve]


# ---- the construction check: no engine ----------------------------------------------------------------------------------------------
def histograms(case, j, chunk):
    """-> (digits [K][nwin] of MSM j by digit_cases.model_bucket, {(window, chunk): counts per |digit|}).  The model is plain Python, one
    call per scalar: it, not the constructions, is what the check's time goes to (about 10 us per term, 30 s for STARK at 24 576)"""
    q = dc.order(case.curve)
    ks = to_ints(case.msms[j][0])
    assert all(0 <= k < q for k in ks), "a scalar is not canonical"
    D = np.array([dc.model_bucket(k, q, case.c)[1] for k in ks], dtype=np.int64)
    NBK = 1 << (case.c - 1)
    h = {}
    for g0 in range(-(-case.K // chunk)):
        part = np.abs(D[g0 * chunk:(g0 + 1) * chunk])
        for w in range(D.shape[1]):
            h[(w, g0)] = np.bincount(part[:, w], minlength=NBK + 1)
    return D, h


def share_span(counts):
    """list mode cuts a run of Tu sorted terms into 64 shares [Tu l / 64, Tu (l + 1) / 64): the largest difference between the buckets of
    a share's last and first term -- the bucket boundaries (empty buckets included) its walk crosses"""
    cum = np.cumsum(counts[1:])
    Tu = int(cum[-1])
    best = 0
    for lane in range(64):
        s0, s1 = (Tu * lane) >> 6, (Tu * (lane + 1)) >> 6
        if s1 > s0:
            best = max(best, int(np.searchsorted(cum, s1 - 1, side="right")) - int(np.searchsorted(cum, s0, side="right")))
    return best


def _mode(h, w, G, T):
    return "list" if max(int(h[(w, g0)][1:].max()) if (w, g0) in h else 0 for g0 in range(G)) > T else "bucket"


def check_case(case, chunk):
    """-> (failure messages, the line that says which edge the case reaches)"""
    geo = Geo(case.c, chunk)
    e, fails = case.edge, []
    G = geo.chunks(case.K)
    K_chunks = -(-case.K // chunk)                          # chunks that hold terms (the padding of the last row may open one more)
    say = lambda msg: fails.append("%s c = %d [%s, chunk %d]: %s" % (case.curve, case.c, case.name, chunk, msg))
    if G > CHUNKS_MAX:
        say("%d chunks: more than the engine takes" % G)
    if "G" in e and e["G"] != G:
        say("G = %d, built for %d" % (G, e["G"]))
    if e.get("more_chunks_than_units") and not G > geo.units:
        say("G = %d does not exceed the %d units" % (G, geo.units))
    for l, pidx in case.msms:
        if pidx.min() < 0 or pidx.max() > INF:
            say("a point index outside the pool")
    # workgroups of the k_bucket_acc launch under the emulator and under either LDS size a device may report
    n_units = len(case.msms) * dc.windows(dc.order(case.curve), dc.KIND_BUCKET, case.c) * geo.units
    wgs = [-(-n_units // geo.waves_per_workgroup(case.curve, G, cap)) for cap in (None,) + LDS_CAPS]
    if e.get("ragged") and not all(v % 8 for v in wgs):
        say("%s workgroups of units (emulator, 64 KB, 160 KB of LDS): a multiple of 8, built for a ragged tail" % wgs)
    line = "%-9s c=%2d%s %-62s K=%6d x%d G=%d%s" % (case.curve, case.c, " (packed counters)" if geo.packed else "", case.name, case.K, len(case.msms), G,
                                                  " (%d / %d / %d workgroups under the emulator / 64 KB / 160 KB of LDS: ragged tail)" % tuple(wgs) if e.get("ragged") else "")
    if case.w is None:
        return fails, line
    w = case.w
    hist = {}
    for j in sorted({case.at} | {j for j, _ in e.get("modes", {})}):
        hist[j] = histograms(case, j, chunk)
    D, h = hist[case.at]
    if case.intended is not None and not np.array_equal(D[:, w], case.intended):
        say("window %d: %d digits are not the intended ones" % (w, int(np.sum(D[:, w] != case.intended))))
    per_chunk = [h[(w, g0)] for g0 in range(K_chunks)]
    largest = max(int(x[1:].max()) for x in per_chunk)
    tu = [int(x[1:].sum()) for x in per_chunk] + [0] * (G - K_chunks)
    mode = "list" if largest > geo.T else "bucket"
    line += " window %d: %s mode, largest bucket %d (T = %d), Tu = %s" % (w, mode, largest, geo.T, tu)
    if e.get("mode") and e["mode"] != mode:
        say("%s mode, built for %s mode (largest bucket %d, T = %d)" % (mode, e["mode"], largest, geo.T))
    if e.get("largest") is not None and e["largest"] != largest:
        say("largest bucket %d, built for %d" % (largest, e["largest"]))
    for g0, v in e.get("tu", {}).items():
        if tu[g0] != v:
            say("Tu of chunk %d is %d, built for %d" % (g0, tu[g0], v))
    total = sum(per_chunk)
    if e.get("nonempty") is not None:
        got = set(int(k) for k in np.nonzero(total[1:])[0] + 1)
        if got != set(e["nonempty"]):
            say("non-empty buckets %s..., built for %s..." % (sorted(got)[:6], sorted(e["nonempty"])[:6]))
    if e.get("inside"):
        got = np.nonzero(total[1:])[0] + 1
        if got.min() < e["inside"][0] or got.max() > e["inside"][1]:
            say("buckets %d .. %d, built for %d .. %d" % (got.min(), got.max(), e["inside"][0], e["inside"][1]))
    if e.get("span") is not None:
        span = max(share_span(x) for x in per_chunk)
        line += ", a share spans %d bucket boundaries" % span
        if span < e["span"]:
            say("the widest share spans %d bucket boundaries, built for %d" % (span, e["span"]))
    for bkt, per in (e.get("runs") or {}).items():
        got = [int(x[bkt]) for x in per_chunk]
        if got != list(per):
            say("bucket %d holds %s terms per chunk, built for %s" % (bkt, got, list(per)))
    for (j, wj), want in e.get("modes", {}).items():
        got = _mode(hist[j][1], wj, K_chunks, geo.T)
        if got != want:
            say("MSM %d window %d in %s mode, built for %s" % (j, wj, got, want))
    return fails, line


def all_cases(curve, chunk, fams=FAMILIES, single_chunk=False):
    for fam in fams:
        for c in family_widths(curve, fam):
            seen = set()
            for case in cases_of(curve, fam, c, chunk, single_chunk):
                if id(case) in seen:
                    continue
                seen.add(id(case))
                case.curve = curve
                yield fam, case


def self_check(chunk, curves=tuple(WIDTHS), fams=FAMILIES):
    """every construction against the digit model -> (failure messages, checks, the lines of the listing)"""
    fails, n, lines = list(geometry_is_the_engines()), 0, []
    for curve in curves:
        for fam, case in all_cases(curve, chunk, fams):
            f, line = check_case(case, chunk)
            fails += f
            lines.append(line)
            n += 1
    return fails, n, lines


# ---- references and the run against an engine ---------------------------------------------------------------------------------------
class Bench:
    """one engine, one table, the 12 points"""

    def __init__(self, eng, coracle, curve, chunk):
        self.eng, self.co, self.curve, self.cv, self.chunk = eng, coracle, curve, mo.CURVES[curve], chunk
        self.q, self.pb = self.cv.q, eng.point_bytes
        fb = self.pb // 2
        gi = coracle.gen_inputs(curve, 2, 3, 5)
        self.params, self.pk = gi["params"], gi["pk"]
        raw = eng.setup(2, 9, bytes([9] * 32))
        self.base = [raw[self.pb * i:self.pb * (i + 1)] for i in range(NPTS)]
        assert len(set(self.base)) == NPTS and bytes(self.pb) not in self.base

        def neg(pt):
            y = int.from_bytes(pt[fb:], "little")
            return pt[:fb] + ((self.cv.p - y) % self.cv.p).to_bytes(fb, "little")
        tab = self.base + [neg(pt) for pt in self.base] + [bytes(self.pb)]
        self.tab = np.frombuffer(b"".join(tab), dtype=np.uint8).reshape(2 * NPTS + 1, self.pb)
        self.inf = bytes(self.pb)
        self.t = None

    def table(self):
        t = self.eng.table(2, 3, self.params, self.pk)
        t.set_bucket_min(1)
        return t

    def folded(self, l, pidx):
        """the 12 scalars of the equivalent MSM over the pool: per point, the sum of its terms' scalars minus those of its negative"""
        lo = (l & np.uint64(0xFFFFFFFF)).astype(np.uint64)
        hi = l >> np.uint64(32)
        out = []
        for j in range(NPTS):
            s = 0
            for rows, sign in ((pidx == j, 1), (pidx == j + NPTS, -1)):
                if rows.any():
                    a, b = lo[rows].sum(axis=0), hi[rows].sum(axis=0)       # (each below 2^32 x 2^20 terms)
                    s += sign * sum((int(a[i]) << (64 * i)) + (int(b[i]) << (64 * i + 32)) for i in range(4))
            out.append(s % self.q)
        return out

    def want(self, l, pidx, python_too):
        sc = self.folded(l, pidx)
        want = self.co.msm(self.curve, b"".join(s.to_bytes(32, "little") for s in sc), b"".join(self.base))
        fails = []
        if python_too:
            with mo.curve_ctx(self.cv):
                pts = [mo.pt_from_wire(pt) for pt in self.base]
                py = mo.pt_wire(mo.msm(self.cv, sc, pts))
            if py != want:
                fails.append("the Python oracle's big-integer MSM differs from the C++ oracle's")
        return want, fails

    def call(self, t, case):
        """-> (result bytes, failure message or None of the profile)"""
        sc = b"".join(np.ascontiguousarray(l, dtype="<u8").tobytes() for l, _ in case.msms)
        pts = b"".join(self.tab[pidx].tobytes() for _, pidx in case.msms)
        t.set_bucket_split(min(case.c, 12))
        t.set_bucket_bits(case.c)
        self.eng.profile_enable(True)
        got = t.msm(len(case.msms), case.K, sc, pts)
        rep = self.eng.profile_report()
        self.eng.profile_enable(False)
        bad = [k for k in ("k_bucket_sort", "k_bucket_acc", "k_bucket_list", "k_bucket_reduce", "k_bucket_final") if k not in rep]
        if bad or "k_bucket_msm" in rep or "k_var_msm" in rep or "k_var_msm_q" in rep:
            return got, "not on the split pipeline: kernels %s" % sorted(rep)      # (rep: {kernel name: (launches, ms)})
        # the engine really sorts in chunks of self.chunk terms: k_bucket_sort ran one workgroup per (MSM, window, chunk)
        blocks = self.eng.last_profile_items.get("k_bucket_sort")
        want = len(case.msms) * dc.windows(self.q, dc.KIND_BUCKET, case.c) * Geo(case.c, self.chunk).chunks(case.K)
        if blocks != want:
            return got, "k_bucket_sort ran %s workgroups, %d (MSM, window, chunk) triples at a chunk of %d terms" % (blocks, want, self.chunk)
        return got, None


def run_cases(bench, cases, python_first=True):
    """each call against the oracle's bytes, MSM by MSM -> (failure messages, checks)"""
    fails, n = [], 0
    t = bench.table()
    try:
        for i, case in enumerate(cases):
            where = "%s c = %d [%s]" % (bench.curve, case.c, case.name)
            wants = []
            for j, (l, pidx) in enumerate(case.msms):
                want, f = bench.want(l, pidx, python_first and i == 0 and j == 0)
                fails += ["%s: %s" % (where, m) for m in f]
                wants.append(want)
            if case.edge.get("inf") and wants[0] != bench.inf:
                fails.append("%s: the reference is not the point at infinity" % where)
            got, prof = bench.call(t, case)
            if prof:
                fails.append("%s: %s" % (where, prof))
            for j, want in enumerate(wants):
                if got[bench.pb * j:bench.pb * (j + 1)] != want:
                    fails.append("%s: MSM %d of %d (K = %d): got %s, want %s" % (where, j, len(wants), case.K, got[bench.pb * j:bench.pb * (j + 1)].hex(), want.hex()))
                n += 1
    finally:
        t.close()
    return fails, n


def run_reuse(bench, cases):
    """family F: the calls in order on ONE table, each against the oracle and against the bytes of a fresh table"""
    fails, n = [], 0
    t = bench.table()
    try:
        for i, case in enumerate(cases):
            where = "%s [call %d: %s]" % (bench.curve, i, case.name)
            want = b""
            for j, (l, pidx) in enumerate(case.msms):
                wj, f = bench.want(l, pidx, i == 0 and j == 0)
                fails += ["%s: %s" % (where, m) for m in f]
                want += wj
            got, prof = bench.call(t, case)
            fresh_t = bench.table()
            try:
                fresh, prof2 = bench.call(fresh_t, case)
            finally:
                fresh_t.close()
            for p in (prof, prof2):
                if p:
                    fails.append("%s: %s" % (where, p))
            if got != want:
                fails.append("%s: differs from the oracle: got %s, want %s" % (where, got.hex(), want.hex()))
            if got != fresh:
                fails.append("%s: differs from a fresh table's bytes" % where)
            n += 2 * len(case.msms)
    finally:
        t.close()
    return fails, n


def run_family(eng, coracle, curve, fam, chunk, widths=None, single_chunk=False):
    """one family on one curve, every width (or `widths`) -> (failure messages, checks)"""
    bench = Bench(eng, coracle, curve, chunk)
    fails, n = [], 0
    for c in widths or family_widths(curve, fam):
        cases = cases_of(curve, fam, c, chunk, single_chunk)
        for case in cases:
            case.curve = curve
        f, k = (run_reuse if fam == "F" else run_cases)(bench, cases)
        fails += f
        n += k
    return fails, n
