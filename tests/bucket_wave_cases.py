"""Cases, a model of the kernel's decisions, references and checks for the one-wave bucket kernel (kernels_bucket.hpp: k_bucket_msm,
body_bucket_msm; engine_core.hpp run_bucket) at its structural edges, through the public mp_msm with mp_set_bucket_min / _bits and
mp_set_bucket_split kept above the width under test.  Shared by tests/test_bucket_wave_emu.py (the kernel body under the development
emulator, CPU) and tests/test_gpu_bucket_wave.py (gfx950) -- same constructions, same expectations, the canonical result point compared
byte for byte with the C++ oracle's, and for the first case of every family and width with the Python oracle's big-integer group law.

The rules the cases lean on: one 64-lane wave owns a (MSM, window) item.  Bucket k = 1 .. NBK = 2^(c-1) has home lane (k - 1) // NB
and class (k - 1) % NB, NB = NBK / 64.  Per class the lanes are ranked by the size of their bucket (more terms first, ties to the lower
lane); worker r sums the rank-r bucket of an even class and the rank-(63 - r) bucket of an odd one, n[worker] terms in all (the RANKED
walk, reduced by parked sums, a suffix scan and log2 NB doublings).  An item whose max(n) exceeds T // 64 + T // 128 + 32 (T: terms with a
non-zero digit) is cut into 64 equal shares [T l >> 6, T (l + 1) >> 6) of the list sorted by bucket instead (the BALANCED walk: lo * run
+ acc by double-and-add).  Persistent waves draw items from one counter per partition of the MSMs (8 partitions from 8 MSMs on).
decide() states these rules on the signed digits of digit_cases.model_bucket; RULES_SOURCE ties them to the source text.

Points, scalars built from intended digits and the Case shape are those of tests/bucket_split_cases.py (imported, not copied).
self_check() recomputes from the digit model alone the edge every case is named for -- mode, max(n) and the threshold, the workers
that hold terms, the non-empty buckets, where the share boundaries fall, the lowest bucket every share reaches -- and fails without
an engine if a construction misses it.

Families that name a window run it in window 0, a middle window and the top window; the others sit in the middle window, the top window
taking only the few digits Maker.top_cap() allows (secp256k1 at 8 bits, whose top window is full, runs the bucket layouts there too).

Out of scope, not tested here: windows of 12 to 14 bits forced onto this kernel with mp_set_bucket_split(15); 11 bits on BLS12-377
(the split pipeline by default); a phase with several bucket jobs of different lengths (reachable only through proofs with a lowered
bucket_min: the golden-vector test covers it); the MP_EXP_BK_STAGE = 0 build.

Every run_* function returns (failure messages, number of checks); no case is skipped or excused."""
import os

import numpy as np

import bucket_split_cases as bsc
import digit_cases as dc
from bucket_split_cases import INF, NPTS, Case, from_ints, q_minus, to_ints

ROOT = bsc.ROOT
FAMILIES = ("A", "B", "C", "D", "E", "F", "G")
BALANCED_FAMILIES = ("A", "D", "E", "G")      # what runs against the emulator library whose every window takes the balanced walk
WIDTHS = {"stark": (8, 9, 10, 11), "secp256k1": (8, 11), "bn254": (9,), "bls12_377": (8, 10)}
NL = 64
WAVES_PER_CU = 8                # BK_WAVES_PER_CU
EMU_CUS = 2                     # the emulator's cu_count()
SPLIT_KERNELS = ("k_bucket_sort", "k_bucket_acc", "k_bucket_list", "k_bucket_reduce", "k_bucket_final")

# ---- the kernel's rules, copied by hand in WaveGeo / decide / partition_sizes below -----------------------------------------------------
RULES_SOURCE = {
    "mental-poker_amd/csrc/kernels_bucket.hpp": (
        "static const uint32_t BK_WAVES_PER_CU = 8;",
        "MP_HD uint32_t bk_buckets(uint32_t c) { return 1u << (c - 1); }",
        "const uint32_t NBK = bk_buckets(a.bits), NB = NBK >> LOG_NL, LOGNB = a.bits - 1u - LOG_NL, HW = NBK + 4u;",
        "r += (o > mine || (o == mine && l < lane)) ? 1u : 0u;",
        "cur[j * NL + ((j & 1u) ? NL - 1u - r : r)] = lane;",
        "const bool balanced = wv.max(n) > T / NL + T / (2 * NL) + 32;",
        "const uint32_t s0 = (uint32_t)(((uint64_t)T * lane) >> LOG_NL), s1 = (uint32_t)(((uint64_t)T * (lane + 1)) >> LOG_NL);",
        "if (li >= ((a.count + a.parts - 1u - part) / a.parts) * per_eq) {",
        "const uint32_t w = li % a.nwin, jb = (li / a.nwin) % a.njobs, b = (li / per_eq) * a.parts + part;",
        "#ifdef MP_EXP_BK_BALANCED",
    ),
    "mental-poker_amd/csrc/engine_core.hpp": (
        "if (!ctx->bk_slots) ctx->bk_slots = BK_WAVES_PER_CU * rt::cu_count();",
        "const uint32_t nitems = count * ph.n_b * bw, nslots = std::min(nitems, bucket_slots());",
        "count, bk_xcd_affine && count >= 8u ? 8u : 1u, tile, tile_K, bk_stage ? 1u : 0u,",
        'ctx->prof.begin("k_bucket_msm", s, nitems);',
    ),
    "tools/hostemu/rt.hpp": (
        "inline uint32_t cu_count() { return 2; }",
        "static constexpr uint32_t NL = 64, LOG_NL = 6;",
    ),
    "tools/hostemu/Makefile": (
        "DEFS := -DMP_EXP_BK_BALANCED",
        "LIB := libmpemu_balanced.so",
    ),
}


def rules_are_the_engines():
    """-> the lines of RULES_SOURCE that the source no longer has (none: the model below is the kernel's arithmetic)"""
    missing = []
    for name, lines in RULES_SOURCE.items():
        with open(os.path.join(ROOT, name)) as f:
            text = f.read()
        missing += ["%s: %s" % (name, ln) for ln in lines if ln not in text]
    return missing


class WaveGeo:
    """buckets, home lanes and classes of a c-bit window on one 64-lane wave"""

    def __init__(self, c):
        self.c = c
        self.NBK = 1 << (c - 1)                            # bk_buckets
        self.NB = self.NBK // NL                           # buckets per home lane = classes
        self.LOGNB = c - 1 - 6

    def lane(self, k):
        return (k - 1) // self.NB

    def cls(self, k):
        return (k - 1) % self.NB

    def bucket(self, lane, j):
        return self.NB * lane + 1 + j

    @staticmethod
    def threshold(T):
        return T // NL + T // (2 * NL) + 32


def partition_sizes(count):
    """MSMs per partition of a launch of `count` MSMs: (count + parts - 1 - part) / parts, 8 partitions from 8 MSMs on"""
    parts = 8 if count >= 8 else 1
    return [(count + parts - 1 - p) // parts for p in range(parts)]


def slots_of(cus):
    return WAVES_PER_CU * cus


def decide(absd, c):
    """the decisions of one (MSM, window) item from its |digits| (zeros included): T, counts per bucket, n per worker, the mode, the
    balanced shares and the buckets they start and end in"""
    g = WaveGeo(c)
    cnt = np.bincount(np.asarray(absd, dtype=np.int64), minlength=g.NBK + 1)[1:g.NBK + 1]
    T = int(cnt.sum())
    per = cnt.reshape(NL, g.NB)                            # [home lane][class]
    lanes = np.arange(NL)
    n = np.zeros(NL, dtype=np.int64)
    for j in range(g.NB):
        col = per[:, j]
        # rank of lane x: the lanes with a larger count, or an equal count and a lower index
        r = ((col[None, :] > col[:, None]) | ((col[None, :] == col[:, None]) & (lanes[None, :] < lanes[:, None]))).sum(axis=1)
        worker = r if j % 2 == 0 else NL - 1 - r
        n[worker] += col
    thr = g.threshold(T)
    s = (T * np.arange(NL + 1)) >> 6                       # share l: positions [s[l], s[l + 1]) of the sorted list
    order = np.repeat(np.arange(1, g.NBK + 1), cnt)
    full = [l for l in range(NL) if s[l + 1] > s[l]]
    lo = {l: int(order[s[l]]) for l in full}               # the lowest bucket the share reaches
    hi = {l: int(order[s[l + 1] - 1]) for l in full}
    edges = np.cumsum(cnt)[np.nonzero(cnt)[0]][:-1] if T else np.zeros(0, dtype=np.int64)      # positions where the bucket changes
    on = sum(1 for e in edges if int(e) in set(int(v) for v in s))
    return {"T": T, "cnt": cnt, "n": n, "maxn": int(n.max()), "thr": thr, "mode": "balanced" if int(n.max()) > thr else "ranked",
            "workers": set(int(l) for l in np.nonzero(n)[0]), "nonempty": set(int(k) + 1 for k in np.nonzero(cnt)[0]),
            "shares": set(int(s[l + 1] - s[l]) for l in range(NL)), "lo": lo, "hi": hi,
            "span": max([hi[l] - lo[l] for l in full] or [0]), "cuts_on": on, "cuts_inside": len(edges) - on}


# ---- scalars -------------------------------------------------------------------------------------------------------------------------
class Maker(bsc.Maker):
    """the split cases' scalar maker (random, digits, top_cap) with this kernel's geometry beside it"""

    def __init__(self, curve, c, seed):
        bsc.Maker.__init__(self, curve, c, bsc.CHUNK_GPU, 100 + seed)
        self.wg = WaveGeo(c)

    def background(self, K, w, avoid=()):
        """digits of window w spread over all buckets and both signs (the top window: over the values it takes), none on `avoid`"""
        if w == self.nwin - 1:
            d = self.rs.randint(0, self.top_cap() + 1, size=K).astype(np.int64)
        else:
            d = self.rs.randint(-self.wg.NBK, self.wg.NBK, size=K).astype(np.int64)
        for b in avoid:
            d[np.abs(d) == b] = 0
        return d

    def signed(self, k, w):
        """bucket numbers -> digits: alternating signs below the top window, where the last bucket is the negative digit"""
        k = np.asarray(k, dtype=np.int64)
        if w == self.nwin - 1:
            return k
        d = np.where(np.arange(len(k)) % 2 == 1, -k, k)
        return np.where(k == self.wg.NBK, -self.wg.NBK, d)


def _pts(mk, K):
    return mk.rs.randint(0, 2 * NPTS + 1, size=K)


def _windows(mk):
    return (("window 0", 0), ("middle window", mk.nwin // 2), ("top window", mk.nwin - 1))


def _mid_digit(mk):
    return mk.wg.NBK // 2 + 3          # odd: bucket b has an even class and b + 1 the next class of the same home lane


def _one(mk, name, w, d, pidx=None, flips=None, **edge):
    d = np.asarray(d, dtype=np.int64)
    l = mk.digits(w, d, flips)
    want = d if flips is None else np.where(flips, -d, d)
    return Case(name, mk.c, [(l, _pts(mk, len(d)) if pidx is None else np.asarray(pidx))], w=w, intended=want, **edge)


def _shuffled(mk, d):
    return np.asarray(d, dtype=np.int64)[mk.rs.permutation(len(d))]


# ---- the families --------------------------------------------------------------------------------------------------------------------
def family_A(curve, c):
    """lengths: nq = kpad / 8 below, at and above the 64 lanes; the K - 1 clamps; the padding of the row counted as zero digits"""
    mk = Maker(curve, c, 1)
    front = from_ints([0, 1, mk.q - 1])

    def msm(K):
        l = mk.random(K)
        l[:min(K, 3)] = front[:min(K, 3)]
        return l, _pts(mk, K)
    cases = [Case("A K = 1 x 3: 0, 1, q - 1", c, [(front[j:j + 1].copy(), np.array([j])) for j in range(3)], nq=8)]
    for K in (7, 8, 9, 63, 64, 65, 511, 512, 513, 520):
        nq = -(-K // 64) * 8
        cases.append(Case("A K = %d" % K, c, [msm(K)], nq=nq))
        cases.append(Case("A K = %d x 3" % K, c, [msm(K) for _ in range(3)], nq=nq))
    return cases


def _threshold_crowd(g, base, b):
    """the crowd m on bucket b beside the |digits| `base` that puts max(n) exactly on the threshold, one more term tipping it"""
    for m in range(1, 8 * g.NBK):
        at, over = decide(np.concatenate([base, np.full(m, b)]), g.c), decide(np.concatenate([base, np.full(m + 1, b)]), g.c)
        if at["maxn"] == at["thr"] and over["maxn"] == over["thr"] + 1:
            return m
    raise AssertionError("no crowd reaches the threshold")


def family_B(curve, c):
    mk = Maker(curve, c, 2)
    g = mk.wg
    NB, w = g.NB, mk.nwin // 2
    cases = []
    # one term on every other bucket (the odd ones: the even classes, every lane) and a crowd on ONE bucket of class 1
    odd = np.arange(1, g.NBK, 2)
    b = g.bucket(37, 1)
    m = _threshold_crowd(g, odd, b)
    for extra, mode in ((0, "ranked"), (1, "balanced")):
        k = _shuffled(mk, np.concatenate([odd, np.full(m + extra, b)]))
        cases.append(_one(mk, "B %d terms on one bucket beside one on every other bucket" % (m + extra), w, mk.signed(k, w), mode=mode,
                          T=len(k), over=extra, n_of={63: NB // 2 + m + extra}))
    # the crowd that tipped it, over two buckets of ONE home lane: classes 0 and 1 go to workers 0 and 63
    h1 = (m + 1) // 2
    h2 = m + 1 - h1
    k = _shuffled(mk, np.concatenate([odd, np.full(h1, g.bucket(37, 0)), np.full(h2, b)]))
    cases.append(_one(mk, "B the same crowd over two buckets of one home lane", w, mk.signed(k, w), mode="ranked", T=len(odd) + m + 1,
                      n_of={0: NB // 2 + h1, 63: NB // 2 + h2}))
    # ... over two buckets of ONE class in different lanes: ranks 0 and 1 of class 1, workers 63 and 62
    k = _shuffled(mk, np.concatenate([odd, np.full(h2, g.bucket(11, 1)), np.full(h1, b)]))
    cases.append(_one(mk, "B the same crowd over two buckets of one class", w, mk.signed(k, w), mode="ranked", T=len(odd) + m + 1,
                      n_of={63: NB // 2 + h2, 62: NB // 2 + h1}))
    # the smallest balanced item: 33 terms on one digit, T < 64, threshold 32
    for wname, wj in _windows(mk):
        bj = 1 if wj == mk.nwin - 1 else (77 if wj == 0 else _mid_digit(mk))
        for cnt, mode in ((32, "ranked"), (33, "balanced")):
            d = np.full(cnt, bj) if wj else np.full(cnt, -bj)
            cases.append(_one(mk, "B %s: %d terms all on one digit" % (wname, cnt), wj, d, mode=mode, T=cnt, maxn=cnt, thr=32, nonempty={bj}))
    return cases


def _cut_inside(n_up, lo_from):
    """n_low >= lo_from such that the boundary between n_low and n_up sorted terms falls inside a share"""
    return next(n for n in range(lo_from, lo_from + 200) if all(((n + n_up) * lane) >> 6 != n for lane in range(NL + 1)))


def family_C(curve, c):
    mk = Maker(curve, c, 3)
    g = mk.wg
    NBK, w, b = g.NBK, mk.nwin // 2, _mid_digit(mk)
    sizes = {33: {0, 1}, 63: {0, 1}, 64: {1}, 65: {1, 2}, 129: {2, 3}}
    cases = []
    for dname, dv in (("digit 1", 1), ("the last bucket", -NBK), ("a middle digit", b)):
        for T, sh in sizes.items():
            cases.append(_one(mk, "C %d terms all on %s" % (T, dname), w, np.full(T, dv), mode="balanced", T=T, shares=sh, nonempty={abs(dv)},
                              lo_all={abs(dv)}))
    for wname, wj in (("window 0", 0), ("top window", mk.nwin - 1)):
        cases.append(_one(mk, "C %s: 65 terms all on digit 1" % wname, wj, np.full(65, 1), mode="balanced", T=65, shares={1, 2}, nonempty={1}))
    # two adjacent digits: the bucket boundary on a share boundary (64 + 64: between the shares of lanes 31 and 32) and inside a share
    cases.append(_one(mk, "C two adjacent digits, the boundary on a share boundary", w, _shuffled(mk, [b] * 64 + [b + 1] * 64), mode="balanced", T=128,
                      nonempty={b, b + 1}, cuts_on=1, cuts_inside=0))
    n_low = _cut_inside(96, 97)
    cases.append(_one(mk, "C two adjacent digits, the boundary inside a share", w, _shuffled(mk, [b] * n_low + [b + 1] * 96), mode="balanced",
                      T=n_low + 96, nonempty={b, b + 1}, cuts_on=0, cuts_inside=1, span=1))
    # (one share crosses NBK - 2 empty buckets: the first crossing adds run to an acc at infinity, the second adds run to acc == run)
    cases.append(_one(mk, "C digits 1 and the last bucket only", w, _shuffled(mk, [1] * n_low + [-NBK] * 96), mode="balanced", T=n_low + 96,
                      nonempty={1, NBK}, cuts_on=0, cuts_inside=1, span=NBK - 1))
    n_sp = NBK
    sp = 1 + (np.arange(n_sp) * (NBK - 1)) // (n_sp - 1)
    crowd = np.full(4 * n_sp, b)
    cases.append(_one(mk, "C a crowd beside T / 4 terms spread over all buckets", w, _shuffled(mk, np.concatenate([mk.signed(sp, w), crowd])),
                      mode="balanced", T=5 * n_sp, nonempty=set(range(1, NBK + 1)), span=2))
    two = _shuffled(mk, [b] * 128 + [b + 1] * 128)
    cases.append(_one(mk, "C every term the same point", w, two, pidx=np.full(256, 5), mode="balanced", T=256, nonempty={b, b + 1}))
    # (shares of four terms, P - P + P - P: the running sum is at infinity inside every share and where a share crosses into bucket b)
    srt = np.sort(two)[::-1]
    cases.append(_one(mk, "C points alternating P, -P", w, srt, pidx=np.where(np.arange(256) % 2 == 0, 3, NPTS + 3), mode="balanced", T=256,
                      nonempty={b, b + 1}, shares={4}))
    n_low = _cut_inside(96, 97)
    cases.append(_one(mk, "C all scalars above q / 2", w, _shuffled(mk, [b] * n_low + [b + 1] * 96), flips=np.ones(n_low + 96, dtype=bool),
                      mode="balanced", T=n_low + 96, nonempty={b, b + 1}, flipped=True))
    return cases


def _lane_load(g):
    """terms per bucket with which ONE home lane's NB buckets keep workers 0 and 63 at or below the threshold"""
    return max(t for t in range(1, 17) if max(1, g.NB // 2) * t <= g.threshold(g.NB * t))


def family_D(curve, c):
    mk = Maker(curve, c, 4)
    g = mk.wg
    NBK, NB, w = g.NBK, g.NB, mk.nwin // 2
    every = np.arange(1, NBK + 1)
    allw = set(range(NL))
    cases = [_one(mk, "D every bucket once, ONE point", w, mk.signed(every, w), pidx=np.full(NBK, 5), mode="ranked", T=NBK, maxn=NB,
                  workers=allw, nonempty=set(every.tolist())),
             _one(mk, "D every bucket once, 12 points in rotation", w, mk.signed(every, w), pidx=np.arange(NBK) % NPTS, mode="ranked", T=NBK,
                  maxn=NB, workers=allw, nonempty=set(every.tolist())),
             _one(mk, "D only bucket 1", w, np.where(np.arange(32) % 3 == 1, -1, 1), mode="ranked", T=32, maxn=32, workers={0}, nonempty={1}),
             _one(mk, "D only the last bucket", w, np.full(29, -NBK), mode="ranked", T=29, maxn=29, workers={NL - 1},
                  nonempty={NBK})]
    for name, j in (("the last class", NB - 1), ("class 0", 0)) + ((("class 1", 1),) if NB > 2 else ()):      # (two classes: the last one is the odd one)
        ks = np.array([g.bucket(l, j) for l in range(NL)])
        cases.append(_one(mk, "D only the buckets of %s" % name, w, mk.signed(ks, w), mode="ranked", T=NL, maxn=1, workers=allw,
                          nonempty=set(ks.tolist())))
    t = _lane_load(g)
    for name, lane in (("home lane 37", 37), ("lane 0 (no doubling)", 0), ("lane 63 (the largest multiplier)", 63)):
        ks = np.repeat(np.array([g.bucket(lane, j) for j in range(NB)]), t)
        cases.append(_one(mk, "D the buckets of %s hold everything" % name, w, mk.signed(_shuffled(mk, ks), w), mode="ranked", T=NB * t,
                          maxn=(NB // 2) * t, workers={0, NL - 1}, nonempty=set(ks.tolist())))
    # class 0: 64, 63, .. 1 terms by lane (rank = lane); class 1: 1, 2, .. 64 (rank = 63 - lane, worker = lane): 65 terms per worker
    ks = np.concatenate([np.repeat(g.bucket(l, 0), NL - l) for l in range(NL)] + [np.repeat(g.bucket(l, 1), l + 1) for l in range(NL)])
    cases.append(_one(mk, "D counts descending by lane in class 0, ascending in class 1", w, mk.signed(_shuffled(mk, ks), w), mode="ranked",
                      T=NL * (NL + 1), maxn=NL + 1, workers=allw, n_of={l: NL + 1 for l in range(NL)}))
    hole = g.bucket(21, NB - 1)
    ks = every[every != hole]
    cases.append(_one(mk, "D exactly one empty bucket", w, mk.signed(ks, w), mode="ranked", T=NBK - 1, maxn=NB, nonempty=set(ks.tolist())))
    ks = np.arange(1, NBK // 2 + 1)
    cases.append(_one(mk, "D lanes 32 .. 63 all empty", w, mk.signed(ks, w), mode="ranked", T=NBK // 2, nonempty=set(ks.tolist())))
    if curve == "secp256k1" and c == 8:
        # the 256-bit order fills the top window: its buckets 1 .. 127 by digits, and the last one, 128, by (q - 1) / 2 and (q + 1) / 2 alone
        top = mk.nwin - 1
        ks = np.arange(1, mk.top_cap() + 1)
        cases.append(_one(mk, "D top window: every bucket it takes by digits, once", top, ks, pidx=np.arange(len(ks)) % NPTS, mode="ranked",
                          T=len(ks), nonempty=set(ks.tolist())))
        l = mk.random(40)
        l[::2] = from_ints([(mk.q - 1) // 2, (mk.q + 1) // 2] * 10)
        cases.append(Case("D top window: the last bucket, (q - 1) / 2 and (q + 1) / 2", c, [(l, _pts(mk, 40))], w=top, mode="ranked", has=NBK))
    return cases


def family_E(curve, c):
    mk = Maker(curve, c, 5)
    w, b = mk.nwin // 2, _mid_digit(mk)
    P, N, O = 7, NPTS + 7, INF
    seqs = (("P, P", [P, P], None), ("P, P, P", [P, P, P], None), ("P, -P, P", [P, N, P], None), ("O, P, O", [O, P, O], None),
            ("-P under a negative digit", [P, N], [1, -1]))
    cases = []
    for what, seq, signs in seqs:
        sg = signs or [1] * len(seq)
        K = 64 + len(seq)
        where = mk.rs.permutation(K)[:len(seq)]
        d = mk.background(K, w, (b,))
        d[where] = [b * s for s in sg]
        pidx = _pts(mk, K)
        pidx[where] = seq
        cases.append(_one(mk, "E ranked: %s alone in its bucket" % what, w, d, pidx=pidx, mode="ranked", count_of={b: len(seq)}))
        K = 72
        rep = np.arange(K) % len(seq)
        cases.append(_one(mk, "E balanced: %s over every share" % what, w, np.array([b * s for s in sg])[rep], pidx=np.array(seq)[rep],
                          mode="balanced", T=K, nonempty={b}))
    return cases


def _cancelling(mk, K):
    """K terms that sum to infinity: s and q - s on one point, pair by pair (an odd K: one zero scalar more)"""
    half = mk.random(K // 2)
    l = np.zeros((K, 4), dtype=np.uint64)
    l[0:2 * (K // 2):2] = half
    l[1:2 * (K // 2):2] = q_minus(half, mk.q)
    pidx = np.repeat(mk.rs.randint(0, 2 * NPTS, size=K // 2 + 1), 2)[:K]
    return l, pidx


def family_F(curve, c, slots):
    """items, partitions and reuse: the calls of ONE table, in order"""
    mk = Maker(curve, c, 6)
    g, nwin = mk.wg, mk.nwin
    w, b = nwin // 2, _mid_digit(mk)
    cases = []
    for count in (1, 7, 8, 9, 15, 16, 17):
        K = 64 + count % 9
        msms = [(mk.random(K), _pts(mk, K)) for _ in range(count)]
        infs = ()
        if count > 1:      # (neither is the last MSM: that one is the odd one out of partition 0 at 9 and 17, and its result shall not be zero bytes)
            msms[1] = (np.zeros((K, 4), dtype=np.uint64), _pts(mk, K))
            msms[count // 2] = _cancelling(mk, K)
            infs = (1, count // 2)
        for lanes in (1, 4):
            cases.append(Case("F %d MSMs of %d terms, %d lane(s) per group operation" % (count, K, lanes), c, msms, lanes=lanes, infs=infs,
                              parts=partition_sizes(count)))
    count = slots // nwin + 1
    cases.append(Case("F %d MSMs of 64 terms: more items than the %d persistent waves" % (count, slots), c,
                      [(mk.random(64), _pts(mk, 64)) for _ in range(count)], over_slots=slots))
    msms = [(mk.digits(w, np.full(72, b) if j % 2 == 0 else mk.background(72, w, (b,))), _pts(mk, 72)) for j in range(4)]
    cases.append(Case("F MSMs alternating between a balanced and a ranked window", c, msms, w=w, at=0, mode="balanced",
                      modes={(j, w): ("balanced" if j % 2 == 0 else "ranked") for j in range(4)}))
    cases.append(Case("F K = 2500", c, [(mk.random(2500), _pts(mk, 2500))]))
    cases.append(Case("F K = 9 straight after K = 2500", c, [(mk.random(9), _pts(mk, 9))]))
    return cases


def family_G(curve, c):
    mk = Maker(curve, c, 7)
    g = mk.wg
    cases = []
    for wname, w in _windows(mk):
        top = w == mk.nwin - 1
        d = 1 + mk.rs.randint(0, mk.top_cap() if top else g.NBK - 1, size=70)
        l = from_ints([int(v) << (c * w) for v in d])
        cases.append(Case("G non-zero digits in %s only%s" % (wname, ": every window zero but the top" if top else ""), c, [(l, _pts(mk, 70))],
                          w=w, intended=d.astype(np.int64), only_windows={w}))
    # window 1 holds P (2^c on P), window 0 holds -2^c P (2^(c-1) - 1 twice and 2 once on -P): neither is infinity, their fold is
    sc, pidx = [], []
    for j in (2, 5, 9):
        sc += [1 << c, g.NBK - 1, g.NBK - 1, 2]
        pidx += [j, NPTS + j, NPTS + j, NPTS + j]
    cases.append(Case("G a result at infinity from windows that are not", c, [(from_ints(sc), np.array(pidx))], w=0, only_windows={0, 1}, infs=(0,)))
    return cases


def cases_of(curve, fam, c, slots=slots_of(EMU_CUS)):
    if fam == "F":
        return family_F(curve, c, slots)
    return {"A": family_A, "B": family_B, "C": family_C, "D": family_D, "E": family_E, "G": family_G}[fam](curve, c)


# ---- the construction check: no engine -----------------------------------------------------------------------------------------------
def digits_of(case, j):
    """digits [K][nwin] of MSM j by digit_cases.model_bucket"""
    q = dc.order(case.curve)
    ks = to_ints(case.msms[j][0])
    assert all(0 <= k < q for k in ks), "a scalar is not canonical"
    return np.array([dc.model_bucket(k, q, case.c)[1] for k in ks], dtype=np.int64), ks


def check_case(case):
    """-> (failure messages, the line that says which edge the case reaches)"""
    e, fails = case.edge, []
    q = dc.order(case.curve)
    nwin = dc.windows(q, dc.KIND_BUCKET, case.c)
    say = lambda msg: fails.append("%s c = %d [%s]: %s" % (case.curve, case.c, case.name, msg))
    for l, pidx in case.msms:
        if pidx.min() < 0 or pidx.max() > INF:
            say("a point index outside the pool")
    kpad = -(-case.K // 64) * 64
    line = "%-9s c=%2d %-72s K=%5d x%-3d nq=%d" % (case.curve, case.c, case.name, case.K, len(case.msms), kpad // 8)
    if "nq" in e and e["nq"] != kpad // 8:
        say("nq = %d, built for %d" % (kpad // 8, e["nq"]))
    if "parts" in e:
        line += " MSMs per partition %s" % e["parts"]
        if sum(e["parts"]) != len(case.msms) or e["parts"] != [sum(1 for b in range(len(case.msms)) if b % len(e["parts"]) == p) for p in range(len(e["parts"]))]:
            say("partition sizes %s do not deal %d MSMs by e mod parts" % (e["parts"], len(case.msms)))
    if "over_slots" in e:
        line += " %d items for %d persistent waves" % (len(case.msms) * nwin, e["over_slots"])
        if not len(case.msms) * nwin > e["over_slots"] or (len(case.msms) - 1) * nwin > e["over_slots"]:
            say("%d items, built to be just more than %d slots" % (len(case.msms) * nwin, e["over_slots"]))
    if case.w is None:
        return fails, line
    w = case.w
    D, ks = digits_of(case, case.at)
    if case.intended is not None and not np.array_equal(D[:, w], case.intended):
        say("window %d: %d digits are not the intended ones" % (w, int(np.sum(D[:, w] != case.intended))))
    r = decide(np.abs(D[:, w]), case.c)
    held = sorted(r["workers"])
    line += " window %d: %s, max(n) = %d (threshold %d), T = %d, %d workers%s, %d buckets" % (
        w, r["mode"], r["maxn"], r["thr"], r["T"], len(held), " %s" % held if len(held) <= 2 else "", len(r["nonempty"]))
    if r["mode"] == "balanced" or "cuts_on" in e:
        los = sorted(set(r["lo"].values()))
        line += ", shares of %s terms, %d bucket boundaries on a share boundary and %d inside, lowest buckets %s, widest span %d" % (
            sorted(r["shares"]), r["cuts_on"], r["cuts_inside"], los if len(los) <= 3 else "%d .. %d" % (los[0], los[-1]), r["span"])
    for key in ("mode", "T", "maxn", "thr", "workers", "nonempty", "shares", "cuts_on", "cuts_inside"):
        if key in e and e[key] != r[key]:
            say("%s is %s, built for %s" % (key, str(r[key])[:60], str(e[key])[:60]))
    if "over" in e and r["maxn"] - r["thr"] != e["over"]:
        say("max(n) = %d at a threshold of %d, built for %d above it" % (r["maxn"], r["thr"], e["over"]))
    for wk, v in e.get("n_of", {}).items():
        if int(r["n"][wk]) != v:
            say("worker %d has %d terms, built for %d" % (wk, int(r["n"][wk]), v))
    for bkt, v in e.get("count_of", {}).items():
        if int(r["cnt"][bkt - 1]) != v:
            say("bucket %d holds %d terms, built for %d" % (bkt, int(r["cnt"][bkt - 1]), v))
    if "lo_all" in e and set(r["lo"].values()) != e["lo_all"]:
        say("the shares reach down to buckets %s, built for %s" % (sorted(set(r["lo"].values()))[:6], sorted(e["lo_all"])))
    if "span" in e and r["span"] < e["span"]:
        say("the widest share spans %d buckets, built for %d" % (r["span"], e["span"]))
    if "has" in e:
        line += ", bucket %d holds %d terms" % (e["has"], int(r["cnt"][e["has"] - 1]))
        if not r["cnt"][e["has"] - 1]:
            say("bucket %d is empty" % e["has"])
    if e.get("flipped") and not all(k > q // 2 for k in ks):
        say("a scalar is not above q / 2")
    if "only_windows" in e:
        used = set(int(x) for x in np.nonzero(np.abs(D).sum(axis=0))[0])
        line += ", non-zero digits in windows %s of %d" % (sorted(used), nwin)
        if used != e["only_windows"]:
            say("non-zero digits in windows %s, built for %s" % (sorted(used), sorted(e["only_windows"])))
    for (j, wj), want in e.get("modes", {}).items():
        got = decide(np.abs(digits_of(case, j)[0][:, wj]), case.c)["mode"]
        if got != want:
            say("MSM %d window %d is %s, built for %s" % (j, wj, got, want))
    if "modes" in e:
        line += ", modes by MSM %s" % [e["modes"][k][0] for k in sorted(e["modes"])]
    return fails, line


def all_cases(curve, fams=FAMILIES):
    for fam in fams:
        for c in WIDTHS[curve]:
            for case in cases_of(curve, fam, c):
                case.curve = curve
                yield fam, case


def self_check(curves=tuple(WIDTHS), fams=FAMILIES):
    """every construction against the digit model -> (failure messages, checks, the lines of the listing)"""
    fails, n, lines = list(rules_are_the_engines()), 0, []
    for curve in curves:
        for fam, case in all_cases(curve, fams):
            f, line = check_case(case)
            fails += f
            lines.append(line)
            n += 1
    return fails, n, lines


# ---- references and the run against an engine ----------------------------------------------------------------------------------------
class Bench(bsc.Bench):
    """the split cases' bench -- one engine, the 12 points, the folded reference -- with calls that must run on k_bucket_msm"""

    def __init__(self, eng, coracle, curve, slots):
        bsc.Bench.__init__(self, eng, coracle, curve, 0)
        self.slots = slots

    def call(self, t, case):
        """-> (result bytes, failure message or None of the profile)"""
        sc = b"".join(np.ascontiguousarray(l, dtype="<u8").tobytes() for l, _ in case.msms)
        pts = b"".join(self.tab[pidx].tobytes() for _, pidx in case.msms)
        lanes = case.edge.get("lanes", 0)
        t.set_bucket_split(15)
        t.set_bucket_bits(case.c)
        t.set_group_lanes(lanes)
        self.eng.profile_enable(True)
        try:
            got = t.msm(len(case.msms), case.K, sc, pts)
            rep = self.eng.profile_report()
        finally:
            self.eng.profile_enable(False)
            t.set_group_lanes(0)
        if "k_bucket_msm" not in rep or [k for k in SPLIT_KERNELS + ("k_var_msm", "k_var_msm_q") if k in rep]:
            return got, "not on the one-wave bucket kernel: kernels %s" % sorted(rep)
        items = self.eng.last_profile_items.get("k_bucket_msm")
        want = len(case.msms) * dc.windows(self.q, dc.KIND_BUCKET, case.c)
        if rep["k_bucket_msm"][0] != 1 or items != want:
            return got, "k_bucket_msm: %d launches of %s items, %d (MSM, window) pairs" % (rep["k_bucket_msm"][0], items, want)
        if "over_slots" in case.edge and (self.slots != case.edge["over_slots"] or not items > self.slots):
            return got, "%d items for %d persistent waves (the case was built for %d)" % (items, self.slots, case.edge["over_slots"])
        if lanes and ("k_bucket_fold_q" in rep) != (lanes == 4) or lanes and ("k_bucket_fold" in rep) != (lanes == 1):
            return got, "%d lane(s) per group operation, but the fold kernels were %s" % (lanes, sorted(k for k in rep if "fold" in k))
        return got, None


def run_cases(bench, cases):
    """each call on ONE table, in order, against the oracle's bytes, MSM by MSM -> (failure messages, checks)"""
    fails, n = [], 0
    t = bench.table()
    try:
        for i, case in enumerate(cases):
            where = "%s c = %d [%s]" % (bench.curve, case.c, case.name)
            wants = []
            for j, (l, pidx) in enumerate(case.msms):
                want, f = bench.want(l, pidx, i == 0 and j == 0)
                fails += ["%s: %s" % (where, m) for m in f]
                wants.append(want)
            for j in case.edge.get("infs", ()):
                if wants[j] != bench.inf:
                    fails.append("%s: the reference of MSM %d is not the point at infinity" % (where, j))
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


def run_family(eng, coracle, curve, fam, slots, widths=None):
    """one family on one curve, every width (or `widths`) -> (failure messages, checks)"""
    bench = Bench(eng, coracle, curve, slots)
    fails, n = [], 0
    for c in widths or WIDTHS[curve]:
        cases = cases_of(curve, fam, c, slots)
        for case in cases:
            case.curve = curve
        f, k = run_cases(bench, cases)
        fails += f
        n += k
    return fails, n


# ---- eight and more equations through the tile and link paths ------------------------------------------------------------------------
def run_group_screen(eng, coracle, bits, cv="stark"):
    """18 proofs of a 2 x 3 deck screened in groups of 2: 9 equations dealt to 8 partitions, partition 0 with two of them.  (The
    engine only takes group sizes that divide the batch -- nearest_divisor in engine_core.hpp --, so a batch of 17 keeps the per-proof
    screen and no equation can be half full: 18 is the smallest batch with 9 equations.)  Proof b is member b / 9 of equation b mod 9.
    Honest, and one response bit flipped in proof 17 (equation 8: partition 0's second equation), in proof 16 (equation 7: partition
    7) and in proof 14: the status words of the per-proof screen"""
    m, n, B = 2, 3, 18
    per = 4 * m * n + 11 * m + 8
    fails, checks = [], 0
    ins = [coracle.gen_inputs(cv, m, n, 8100 + b) for b in range(B)]
    g0 = ins[0]
    t = eng.table(m, n, g0["params"], g0["pk"])
    try:
        t.set_work_split(0)
        t.set_group_verify(0, 0)
        decks = b"".join(g["deck"] for g in ins)
        out_d, out_p, st0 = t.shuffle_and_remask_batch(decks, b"".join(g["rho"] for g in ins), [v for g in ins for v in g["perm"]],
                                                       b"".join(g["prover_seed"] for g in ins))
        if st0 != [0] * B:
            fails.append("the prover's status words: %s" % st0)
        psz = t.proof_bytes
        cases = {"honest": out_p}
        for b in (17, 16, 14):
            bad = bytearray(out_p)
            bad[(b + 1) * psz - 31] ^= 2
            cases["proof %d bad" % b] = bytes(bad)
        want = {k: t.verify_shuffle_batch(decks, out_d, p) for k, p in cases.items()}
        for b in (17, 16, 14):
            k = "proof %d bad" % b
            if [v != 0 for v in want[k]] != [i == b for i in range(B)]:
                fails.append("per-proof screen, %s: status %s" % (k, want[k]))
        if want["honest"] != [0] * B:
            fails.append("per-proof screen, honest: status %s" % want["honest"])
        checks += 4
        t.set_bucket_split(15)
        t.set_bucket_bits(bits)
        # first in groups of 3: longer digit rows in the same (grow-only) buffer, whose digits stay behind in the padding of the rows of
        # the groups of 2 -- the padding counts as zero digits whatever it holds
        t.set_group_verify(3 * per, 0)
        if t.group_size(B) != 3:
            fails.append("groups of %d proofs, not of 3" % t.group_size(B))
        looked = t.reverified_count()
        got = t.verify_shuffle_batch(decks, out_d, out_p)
        if got != want["honest"] or t.reverified_count() != looked:
            fails.append("%d bits, honest, groups of 3: the group screen says %s, %d proofs were verified again" % (bits, got, t.reverified_count() - looked))
        checks += 1
        t.set_group_verify(2 * per, 0)
        if t.group_size(B) != 2:
            fails.append("groups of %d proofs, not of 2" % t.group_size(B))
        nwin = dc.windows(dc.order(cv), dc.KIND_BUCKET, bits)
        for k, p in cases.items():
            looked = t.reverified_count()
            eng.profile_enable(True)
            try:
                got = t.verify_shuffle_batch(decks, out_d, p)
                rep = eng.profile_report()
            finally:
                eng.profile_enable(False)
            if got != want[k]:
                fails.append("%d bits, %s: the group screen says %s, the per-proof screen %s" % (bits, k, got, want[k]))
            # (a wrong equation value only sends its proofs through the finer pass, which gives the right words: the count tells) the two
            # members of a failing equation are looked at again, nobody else, and nobody at all in an honest batch
            looked = t.reverified_count() - looked
            if looked != (0 if k == "honest" else 2):
                fails.append("%d bits, %s: %d proofs were verified again, not %d" % (bits, k, looked, 0 if k == "honest" else 2))
            checks += 2
            if "k_bucket_msm" not in rep or [s for s in SPLIT_KERNELS if s in rep]:
                fails.append("%d bits, %s: not on the one-wave bucket kernel: %s" % (bits, k, sorted(rep)))
            elif k == "honest" and (rep["k_bucket_msm"][0] != 1 or eng.last_profile_items.get("k_bucket_msm") != 9 * nwin):
                fails.append("%d bits, honest: %d launches of k_bucket_msm, the last of %s items; 9 equations of %d windows are %d" % (
                    bits, rep["k_bucket_msm"][0], eng.last_profile_items.get("k_bucket_msm"), nwin, 9 * nwin))
            checks += 1
    finally:
        t.close()
    return fails, checks


def run_chain_nine(eng, coracle, cv="stark"):
    """9 ungrouped tables of 2 links (the construction of chain_cases.run_chain_cases): 9 chain equations in one launch.  Honest, and one
    bad link in table 8: the status words of the per-link verifier"""
    m, n, L, T = 2, 3, 2, 9
    fails, checks = [], 0
    g0 = coracle.gen_inputs(cv, m, n, 50)
    params, pk = g0["params"], g0["pk"]
    table = eng.table(m, n, params, pk)
    try:
        if table.chain_group_size(T, L, False) != 1:
            fails.append("the tables are grouped by %d" % table.chain_group_size(T, L, False))
        chain = [[coracle.gen_inputs(cv, m, n, 70 + t)["deck"] for t in range(T)]]
        proofs = []
        for j in range(L):
            nxt, prf = [], []
            for t in range(T):
                gi = coracle.gen_inputs(cv, m, n, 100 + 10 * j + t)
                d, p = coracle.shuffle_and_remask(cv, m, n, params, pk, chain[j][t], gi["rho"], gi["perm"], gi["prover_seed"])
                nxt.append(d)
                prf.append(p)
            chain.append(nxt)
            proofs.append(prf)
        decks = b"".join(b"".join(row) for row in chain)
        bad = [row[:] for row in proofs]
        bad[1][8] = proofs[1][0]                           # link 1 of table 8: another table's proof
        for name, prf in (("honest", proofs), ("a bad link in table 8", bad)):
            exp = []
            for j in range(L):
                exp += table.verify_shuffle_batch(b"".join(chain[j]), b"".join(chain[j + 1]), b"".join(prf[j]))
            looked = table.reverified_count()
            eng.profile_enable(True)
            try:
                st = table.verify_shuffle_chain(T, L, decks, b"".join(b"".join(row) for row in prf), None)
                rep = eng.profile_report()
            finally:
                eng.profile_enable(False)
            if st != exp or [v != 0 for v in st] != [name != "honest" and i == 1 * T + 8 for i in range(L * T)]:
                fails.append("chain, %s: status %s, link by link %s" % (name, st, exp))
            # (a wrong equation value only sends its links through the per-link verifier, which gives the right words: the count tells)
            looked = table.reverified_count() - looked
            if looked != (0 if name == "honest" else L):
                fails.append("chain, %s: %d links were verified again, not %d" % (name, looked, 0 if name == "honest" else L))
            checks += 2
            if name == "honest":
                items = eng.last_profile_items.get("k_bucket_msm")
                if "k_bucket_msm" not in rep or rep["k_bucket_msm"][0] != 1 or not items or items % T:
                    fails.append("chain, honest: k_bucket_msm %s, items %s: not one launch of 9 equations" % (rep.get("k_bucket_msm"), items))
                checks += 1
    finally:
        table.close()
    return fails, checks
