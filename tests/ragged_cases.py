"""Cases, references and checks for the ragged calls: cards with different numbers of tokens, tables with different numbers of players and
shuffle chains of different lengths in one call -- mp_reveal_ragged_batch, mp_unmask_ragged_batch[_dev], mp_aggregate_keys_ragged_batch
and mp_verify_shuffle_chain_ragged.  Shared by tests/test_ragged_emu.py (the kernel bodies under the development emulator, CPU) and
tests/test_gpu_ragged.py (the gfx950 build) -- same cases, same expectations.

Item c of a call owns the lanes first[c] .. first[c+1] - 1 of an offsets array with first[0] = 0.  Two expectations, independent of each
other: (1) the C++ oracle, the way open_cases.py and deal_cases.py use it (coracle.msm, coracle.sigma_prove, coracle.sigma_verify; the
fold of lane words into card and table words is done here); (2) the uniform calls on the items regrouped by their count: item by item
they must give what the ragged call gives, and with equal counts the ragged call returns the bytes and words of the uniform one.

Every case names the edge its offsets are there for and asserts it on the CPU (edge_failures) before the library is asked.  Every run_*
function takes an engine (_native.Engine), the coracle module and a curve name, and returns (failure messages, number of checks made)."""
import ctypes
import hashlib
import os
import random
import re

import mp_oracle as po
from trait_cases import BAD_ENCODING, CURVES, Ctx, M_, N_  # noqa: F401  (CURVES: for the test files)

BAD_ARGUMENT = -3
CHAUM_PEDERSEN, SCHNORR = 6, 5
NO_INDEX = 0xFFFFFFFF
REVEAL = po.REVEAL_RNG_SEED
MAX_LANES = 1048576
WAVE = 64
WORKGROUP = 256                 # lanes per workgroup of MP_RUN / MP_KERNEL: asserted against csrc/rt.hpp by workgroup_size()
SCREEN_GROUPS = (64, 0xFFFFFFFF)      # the group sizes of tests/sigma_screen_cases.py: GROUP and AUTO
AUTO_REPEAT = 18                      # AUTO screens a call from 64 x 16 = 1 024 lanes on: 18 x the 67 lanes of the mixed case
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def workgroup_size():
    """the block size MP_KERNEL launches with, read from the runtime header"""
    text = open(os.path.join(ROOT, "mental-poker_amd", "csrc", "rt.hpp")).read()
    m = re.search(r"#define MP_KERNEL\(NAME, ARGS, BODY\).*?__launch_bounds__\((\d+)\).*?blockIdx\.x \* (\d+)u \+ threadIdx\.x", text, re.S)
    assert m and m.group(1) == m.group(2), "MP_KERNEL not found in rt.hpp"
    return int(m.group(1))


def offsets(counts):
    first = [0]
    for n in counts:
        first.append(first[-1] + n)
    return first


def _straddles(first, edge):
    """some item has lanes on both sides of the boundary in front of lane `edge`: its first lane is edge - 1 or lower, its last lane edge
    or higher (first[c] < edge < first[c+1])"""
    return any(a < edge < b for a, b in zip(first, first[1:]))


# (name, counts, what its offsets must hit).  Lanes are numbered from 0: "ends at lane 63" = the next item starts at lane 64.
CASES = [
    ("one item, one lane", (1,), lambda f: f == [0, 1]),
    ("65 items of one lane", (1,) * 65, lambda f: f == list(range(66))),
    ("one item with all 257 lanes", (257,), lambda f: f == [0, 257] and _straddles(f, WAVE) and _straddles(f, WORKGROUP)),
    ("an item ends at lane 63, the next starts at lane 64", (60, 4, 5), lambda f: WAVE in f and f[f.index(WAVE) - 1] < WAVE - 1),
    ("an item straddles lanes 63 | 64", (61, 6, 2), lambda f: WAVE not in f and _straddles(f, WAVE) and f[1] == 61 and f[2] == 67),
    ("an item straddles the workgroup edge", (9,) * 28 + (10, 1),
     lambda f: WORKGROUP not in f and _straddles(f, WORKGROUP) and f[28] == WORKGROUP - 4 and f[29] == WORKGROUP + 6),
    ("one-lane items on both sides of a ten-lane item", (1, 10, 1), lambda f: f == [0, 1, 11, 12]),
    ("counts 2..10 mixed, the last item of one lane", (7, 2, 10, 3, 9, 4, 8, 5, 6, 2, 10, 1),
     lambda f: sorted(set(b - a for a, b in zip(f, f[1:]))) == [1] + list(range(2, 11)) and f[-1] - f[-2] == 1),
]
EQUAL = [(7, 9), (13, 5)]       # (items, lanes per item): held to the uniform call byte for byte
MIXED = CASES[-1]


def edge_failures(cases=None):
    """the offsets of every case hit the edge the case names"""
    fails = []
    if workgroup_size() != WORKGROUP:
        fails.append("rt.hpp launches blocks of %d lanes, the cases assume %d" % (workgroup_size(), WORKGROUP))
    for name, counts, hits in (cases if cases is not None else CASES):
        f = offsets(counts)
        if f[0] != 0 or any(b <= a for a, b in zip(f, f[1:])) or not hits(f):
            fails.append("case '%s': the offsets %s miss the edge" % (name, f[:12]))
    return fails


def _by_count(counts):
    """{count: [items with that count]}: the calls a caller makes today"""
    groups = {}
    for i, n in enumerate(counts):
        groups.setdefault(n, []).append(i)
    return groups


# ---------------------------------------------------------------------------------------------------------------- opening
_OPEN_CACHE = {}


class Ragged:
    """open_cases.Batch with a count per card: keys, cards, signers, prover seeds; tokens, proofs and plaintexts as the oracle computes
    them.  The edge kinds are those of open_cases.Batch.  The oracle's part is computed once per (curve, counts, salt, edges)."""

    def __init__(self, c, counts, salt=0, edges=True):
        self.c, self.counts, self.C = c, list(counts), len(counts)
        self.first = offsets(counts)
        self.B = self.first[-1]
        key = (c.curve, tuple(counts), salt, edges)
        if key not in _OPEN_CACHE:
            _OPEN_CACHE[key] = self._build(salt, edges)
        d = _OPEN_CACHE[key]
        self.sk, self.pk, self.K = d["sk"], d["pk"], len(d["sk"])
        self.cards, self.signer, self.kinds = list(d["cards"]), list(d["signer"]), list(d["kinds"])
        self.seeds, self.tokens, self.proofs, self.plain = d["seeds"], list(d["tokens"]), list(d["proofs"]), list(d["plain"])

    def _build(self, salt, edges):
        c, C, q = self.c, self.C, self.c.q
        rng = random.Random(7000 * C + 10 * self.B + salt + c.cv.cid)
        # players 0..4: the edge keys (token = O, +-c0, ...); 5 and 6: sk and q - sk (their tokens cancel); the rest random
        sk = [0, 1, q - 1, (q - 1) // 2, (q + 1) // 2]
        s = rng.randrange(3, q - 1)
        sk += [s, q - s] + [rng.randrange(3, q - 1) for _ in range(min(max(max(self.counts), 3), 12))]
        K = len(sk)
        pk = [c.mul(k, c.G) for k in sk]
        cards, signer, kinds = [], [], []
        for i, T in enumerate(self.counts):
            c0, c1 = c.pool[1 + (i + C) % 15], c.pool[1 + (3 * i + T) % 15]
            sg = [(i + 3 * j + T) % K for j in range(T)]          # walks through the edge keys as well
            kind = "generic"
            k = (i + C + T) % 8 if edges else 0
            if k == 1:
                kind, c0 = "c0 = O", c.inf
            elif k == 2:
                kind, c1 = "c1 = O", c.inf
            elif k == 3 and T >= 2:
                kind, c1 = "c1 = O, one signer twice", c.inf           # c1 - t - t: the second subtraction is a doubling
                sg[0] = sg[1] = 7
            elif k == 4 and T >= 2:
                kind = "sum of the tokens = O"                          # sk, q - sk, and the key 0 for the rest
                sg = [5, 6] + [0] * (T - 2)
            elif k == 5:
                kind = "sum of the tokens = c1"
                sg = [7 + j % (K - 7) for j in range(T)]
                c1 = c.co.msm(c.curve, c.sc(1) * T, b"".join(c.mul(sk[g], c0) for g in sg))
            elif k == 6 and T >= 3:
                kind = "two tokens cancel"
                sg[1], sg[2] = 5, 6
            kinds.append(kind)
            cards.append(c0 + c1)
            signer += sg
        seeds = [hashlib.blake2s(b"ragged reveal seed %d %d %d %d" % (C, self.B, salt, b)).digest() for b in range(self.B)]
        tokens, proofs = [], []
        for i in range(C):
            c0 = cards[i][:c.pb]
            for b in range(self.first[i], self.first[i + 1]):
                g = signer[b]
                tok = c.mul(sk[g], c0)
                tokens.append(tok)
                proofs.append(c.co.sigma_prove(c.curve, 2, c0 + c.G, tok + pk[g], c.sc(sk[g]), REVEAL, seeds[b]))
        self.cards = cards
        plain = [self.plain_of(i, tokens[self.first[i]:self.first[i + 1]]) for i in range(C)]
        return dict(sk=sk, pk=pk, cards=cards, signer=signer, kinds=kinds, seeds=seeds, tokens=tokens, proofs=proofs, plain=plain)

    def plain_of(self, i, toks):
        c = self.c
        return c.co.msm(c.curve, c.sc(1) + c.sc(c.q - 1) * len(toks), self.cards[i][c.pb:] + b"".join(toks))

    def lanes(self, i):
        return range(self.first[i], self.first[i + 1])

    def card_list(self):
        """the true card of the first, the middle and the last item, other points and the identity in between; the first one a second
        time further down (the smaller index counts)"""
        c, C = self.c, self.C
        rng = random.Random(79 + C + self.B)
        fill = lambda: c.mul(rng.randrange(3, c.q - 1), c.G)      # noqa: E731
        return [self.plain[0], fill(), c.inf, self.plain[C // 2], fill(), self.plain[0], self.plain[C - 1]]

    def inputs(self):
        return dict(keys=list(self.pk), cards=list(self.cards), signer=list(self.signer), tokens=list(self.tokens), proofs=list(self.proofs))

    def secret_bytes(self):
        return b"".join(self.c.sc(k) for k in self.sk)

    def reveal(self, t):
        return t.reveal_ragged_batch(b"".join(self.pk), self.secret_bytes(), b"".join(self.cards), self.counts, self.signer, b"".join(self.seeds))

    def unmask(self, t, lst, d=None):
        d = d if d is not None else self.inputs()
        return t.unmask_ragged_batch(b"".join(d["keys"]), b"".join(d["cards"]), self.counts, d["signer"], b"".join(d["tokens"]),
                                     b"".join(d["proofs"]), b"".join(lst))


def _check_open(fails, tag, b, got, lst, want_ts):
    """got = (plaintexts, indices, token_status, card_status) of one ragged unmask call against the oracle's expectations: the card word
    is the first token word that is not 0 in lane order; a card of status 0 opens to the oracle's plaintext and its index in lst, the
    others to zero bytes and no index"""
    c = b.c
    plain, idx, ts, cs = got
    if ts != want_ts:
        fails.append("%s: token status %s, expected %s" % (tag, [(i, v) for i, v in enumerate(ts) if v != want_ts[i]][:8],
                                                           [(i, want_ts[i]) for i, v in enumerate(ts) if v != want_ts[i]][:8]))
    for i in range(b.C):
        word = next((want_ts[l] for l in b.lanes(i) if want_ts[l] != 0), 0)
        if cs[i] != word:
            fails.append("%s card %d (%s, lanes %d..%d): card status %d, expected %d" % (tag, i, b.kinds[i], b.first[i], b.first[i + 1] - 1, cs[i], word))
        wp = b.plain[i] if word == 0 else c.inf
        wi = (lst.index(wp) if wp in lst else NO_INDEX) if word == 0 else NO_INDEX
        if plain[i * c.pb:(i + 1) * c.pb] != wp:
            fails.append("%s card %d (%s): plaintext differs from the oracle's" % (tag, i, b.kinds[i]))
        if idx[i] != wi:
            fails.append("%s card %d (%s): index %#x, expected %#x" % (tag, i, b.kinds[i], idx[i], wi))
    return 3 * b.C + b.B


def _open_against_uniform(fails, tag, t, b, d, lst, got, revealed=None):
    """the second expectation: one uniform call per distinct count on the cards of that count gives, item by item, what the ragged call
    gave -- tokens, proofs and words of reveal (honest inputs only), plaintexts, indices and words of unmask"""
    c = b.c
    pb, psz = c.pb, 2 * c.pb + 32
    plain, idx, ts, cs = got
    n = 0
    for T, items in sorted(_by_count(b.counts).items()):
        lanes = [l for i in items for l in b.lanes(i)]
        cards = b"".join(d["cards"][i] for i in items)
        up, ui, uts, ucs = t.unmask_batch(b"".join(d["keys"]), cards, T, [d["signer"][l] for l in lanes], b"".join(d["tokens"][l] for l in lanes),
                                          b"".join(d["proofs"][l] for l in lanes), b"".join(lst))
        if uts != [ts[l] for l in lanes] or ucs != [cs[i] for i in items] or ui != [idx[i] for i in items] or \
                up != b"".join(plain[i * pb:(i + 1) * pb] for i in items):
            fails.append("%s: the cards of %d tokens differ between mp_unmask_ragged_batch and mp_unmask_batch" % (tag, T))
        n += 4
        if revealed is not None:
            tok, prf, st = revealed
            ut, upf, ust = t.reveal_batch(b"".join(b.pk), b.secret_bytes(), cards, T, [b.signer[l] for l in lanes], b"".join(b.seeds[l] for l in lanes))
            if ust != [st[l] for l in lanes] or ut != b"".join(tok[l * pb:(l + 1) * pb] for l in lanes) or \
                    upf != b"".join(prf[l * psz:(l + 1) * psz] for l in lanes):
                fails.append("%s: the cards of %d tokens differ between mp_reveal_ragged_batch and mp_reveal_batch" % (tag, T))
            n += 3
    return n


def run_open_case(eng, coracle, curve, case):
    """one honest case: reveal gives the oracle's tokens and proofs lane by lane, unmask all words 0 with the oracle's plaintexts and
    their indices (and plaintexts alone without a card list); both agree with the uniform calls on the cards regrouped by count"""
    name, counts, _ = case
    fails = edge_failures([case])
    if fails:
        return fails, 1
    c = Ctx(eng, coracle, curve)
    checks = 1
    b = Ragged(c, counts)
    tag = "%s '%s'" % (curve, name)
    for i in range(b.C):      # the edge cards are what they say, in the oracle
        if (b.kinds[i] == "sum of the tokens = c1" and b.plain[i] != c.inf) or (b.kinds[i] == "sum of the tokens = O" and b.plain[i] != b.cards[i][c.pb:]):
            fails.append("%s card %d: the case '%s' is not what it says in the oracle" % (tag, i, b.kinds[i]))
    tok, prf, st = b.reveal(c.t)
    if st != [0] * b.B:
        fails.append("%s: reveal status %s" % (tag, [(i, v) for i, v in enumerate(st) if v][:8]))
    psz = 2 * c.pb + 32
    for i in range(b.C):
        for l in b.lanes(i):
            if tok[l * c.pb:(l + 1) * c.pb] != b.tokens[l]:
                fails.append("%s lane %d (card %d, %s, signer %d): token differs from the oracle's" % (tag, l, i, b.kinds[i], b.signer[l]))
            if prf[l * psz:(l + 1) * psz] != b.proofs[l]:
                fails.append("%s lane %d (card %d, %s, signer %d): proof differs from the oracle's" % (tag, l, i, b.kinds[i], b.signer[l]))
    checks += 3 * b.B
    lst = b.card_list()
    d = b.inputs()
    d["tokens"] = [tok[l * c.pb:(l + 1) * c.pb] for l in range(b.B)]
    d["proofs"] = [prf[l * psz:(l + 1) * psz] for l in range(b.B)]
    got = b.unmask(c.t, lst, d)
    checks += _check_open(fails, tag, b, got, lst, [0] * b.B)
    checks += _open_against_uniform(fails, tag, c.t, b, d, lst, got, (tok, prf, st))
    checks += _check_open(fails, tag + ", no list", b, b.unmask(c.t, []), [], [0] * b.B)
    c.close()
    return fails, checks


def run_open_equal(eng, coracle, curve, shape):
    """equal counts: the ragged calls return the bytes and words of the uniform calls, with edge cards and one bad token in the batch"""
    C, T = shape
    c = Ctx(eng, coracle, curve)
    fails = []
    b = Ragged(c, (T,) * C, salt=2)
    if b.first != [i * T for i in range(C + 1)]:
        fails.append("%s (%d, %d): the offsets are not c * T" % (curve, C, T))
    keys, cards, seeds = b"".join(b.pk), b"".join(b.cards), b"".join(b.seeds)
    if b.reveal(c.t) != c.t.reveal_batch(keys, b.secret_bytes(), cards, T, b.signer, seeds):
        fails.append("%s (%d, %d): mp_reveal_ragged_batch differs from mp_reveal_batch" % (curve, C, T))
    lst = b.card_list()
    d = b.inputs()
    d["tokens"][(C // 2) * T + T - 1] = c.pool[0]
    got = b.unmask(c.t, lst, d)
    want = c.t.unmask_batch(keys, cards, T, b.signer, b"".join(d["tokens"]), b"".join(b.proofs), b"".join(lst))
    if got != want:
        fails.append("%s (%d, %d): mp_unmask_ragged_batch differs from mp_unmask_batch" % (curve, C, T))
    if [i for i, v in enumerate(want[3]) if v] != [C // 2] or want[3][C // 2] != CHAUM_PEDERSEN:
        fails.append("%s (%d, %d): card status %s" % (curve, C, T, want[3]))
    c.close()
    return fails, 4


DEFECT_COUNTS = (3, 5, 1, 4, 2, 6, 1, 3, 4)
_DEFECT_CACHE = {}


def open_defects(c):
    """-> (batch, inputs, expected token words).  In one call: a tampered proof at the first lane of card 1, at the last lane of card 3
    and in the one-lane card 2; a signer >= K in card 4; a token whose coordinate is not reduced in card 5; a c1 off the curve in card 7,
    which spoils its three tokens -- one of them has a signer >= K as well and keeps MP_ERR_BAD_ARGUMENT -- and leaves the first token of
    card 8, the lane after its last, alone.  Cards 0, 6 (one lane) and 8 are honest.  Random keys only: every defect is a defect."""
    b = Ragged(c, DEFECT_COUNTS, salt=11, edges=False)
    co, curve, pb, q = c.co, c.curve, c.pb, c.q
    b.signer = [7 + (3 * l + 2) % (b.K - 7) for l in range(b.B)]
    if curve not in _DEFECT_CACHE:
        for i in range(b.C):
            c0 = b.cards[i][:pb]
            for l in b.lanes(i):
                g = b.signer[l]
                b.tokens[l] = c.mul(b.sk[g], c0)
                b.proofs[l] = co.sigma_prove(curve, 2, c0 + c.G, b.tokens[l] + b.pk[g], c.sc(b.sk[g]), REVEAL, b.seeds[l])
        _DEFECT_CACHE[curve] = (b.tokens, b.proofs, [b.plain_of(i, b.tokens[b.first[i]:b.first[i + 1]]) for i in range(b.C)])
    b.tokens, b.proofs, b.plain = (list(v) for v in _DEFECT_CACHE[curve])
    d = b.inputs()
    want = [0] * b.B
    f = b.first
    z1 = lambda p: p[:2 * pb] + c.sc((int.from_bytes(p[2 * pb:], "little") + 1) % q)      # noqa: E731
    for l, name in ((f[1], "first lane of card 1"), (f[4] - 1, "last lane of card 3"), (f[2], "the one-lane card 2")):
        d["proofs"][l] = z1(d["proofs"][l])
        want[l] = co.sigma_verify(curve, 2, d["cards"][[i for i in range(b.C) if l in b.lanes(i)][0]][:pb] + c.G,
                                  d["tokens"][l] + d["keys"][d["signer"][l]], d["proofs"][l], REVEAL)
        assert want[l] == CHAUM_PEDERSEN, "the oracle accepts the tampered proof at the %s" % name
    d["signer"][f[4] + 1] = b.K
    want[f[4] + 1] = BAD_ARGUMENT
    tk = d["tokens"][f[5] + 2]
    d["tokens"][f[5] + 2] = c.p.to_bytes(c.fb, "little") + tk[c.fb:]
    want[f[5] + 2] = BAD_ENCODING
    d["cards"][7] = d["cards"][7][:pb] + c.off_curve(d["cards"][7][pb:])
    d["signer"][f[7] + 1] = b.K + 5
    want[f[7]:f[8]] = [BAD_ENCODING, BAD_ARGUMENT, BAD_ENCODING]
    b.kinds = ["honest", "bad first lane", "bad one-lane card", "bad last lane", "signer >= K", "token not reduced", "honest one-lane card",
               "c1 off the curve", "honest"]
    assert f[8] == f[7] + 3 and want[f[8]] == 0 and [next((want[l] for l in b.lanes(i) if want[l]), 0) for i in range(b.C)] == \
        [0, CHAUM_PEDERSEN, CHAUM_PEDERSEN, CHAUM_PEDERSEN, BAD_ARGUMENT, BAD_ENCODING, 0, BAD_ENCODING, 0]
    return b, d, want


def run_open_defects(eng, coracle, curve):
    """the defects of open_defects: exactly their lanes and cards have a word, every other lane and card is 0 and opens to the oracle's
    plaintext; the uniform calls on the regrouped cards say the same"""
    c = Ctx(eng, coracle, curve)
    fails = []
    b, d, want = open_defects(c)
    lst = [b.plain[0], b.plain[8], b.plain[6]]
    got = b.unmask(c.t, lst, d)
    checks = _check_open(fails, "%s defects" % curve, b, got, lst, want)
    checks += _open_against_uniform(fails, "%s defects" % curve, c.t, b, d, lst, got)
    # the prover's side: a signer past the keys and a card off the curve between honest lanes
    sg = list(b.signer)
    sg[b.first[3] + 1] = b.K
    cards = list(b.cards)
    cards[5] = c.off_curve(cards[5][:c.pb]) + cards[5][c.pb:]
    tok, prf, st = c.t.reveal_ragged_batch(b"".join(b.pk), b.secret_bytes(), b"".join(cards), b.counts, sg, b"".join(b.seeds))
    wst = [0] * b.B
    wst[b.first[3] + 1] = BAD_ARGUMENT
    wst[b.first[5]:b.first[6]] = [BAD_ENCODING] * 6
    psz = 2 * c.pb + 32
    if st != wst:
        fails.append("%s reveal with refused lanes: status %s, expected %s" % (curve, st, wst))
    for l in range(b.B):
        if wst[l] == 0 and (tok[l * c.pb:(l + 1) * c.pb] != b.tokens[l] or prf[l * psz:(l + 1) * psz] != b.proofs[l]):
            fails.append("%s reveal lane %d (honest, next to refused ones): differs from the oracle's" % (curve, l))
    c.close()
    return fails, checks + 2 * b.B


def run_open_python_oracle(eng, coracle, curve):
    """the third restatement on one tiny batch of cards with 2, 3 and 1 tokens: po.compute_reveal_token and po.unmask"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    b = Ragged(c, (2, 3, 1), salt=5, edges=False)
    tok, prf, st = b.reveal(c.t)
    plain, idx, ts, cs = b.unmask(c.t, [b.plain[1]])
    psz = 2 * c.pb + 32
    with po.curve_ctx(c.cv):
        pts = [po.pt_from_wire(c.params[i * c.pb:(i + 1) * c.pb]) for i in range(N_ + 3)]
        pp = po.Params(c.cv, M_, N_, pts[0], pts[1:1 + N_], pts[1 + N_], pts[2 + N_])
        for i in range(b.C):
            masked = (po.pt_from_wire(b.cards[i][:c.pb]), po.pt_from_wire(b.cards[i][c.pb:]))
            tpk = []
            for l in b.lanes(i):
                g = b.signer[l]
                pk = po.pt_from_wire(b.pk[g])
                token, proof = po.compute_reveal_token(pp, b.sk[g], pk, masked, b.seeds[l])
                if po.pt_wire(token) != tok[l * c.pb:(l + 1) * c.pb] or po.sigma_proof_bytes(proof) != prf[l * psz:(l + 1) * psz]:
                    fails.append("%s lane %d: token or proof differs from the Python oracle's" % (curve, l))
                tpk.append((token, proof, pk))
            if po.pt_wire(po.unmask(pp, tpk, masked)) != plain[i * c.pb:(i + 1) * c.pb]:
                fails.append("%s card %d: plaintext differs from the Python oracle's" % (curve, i))
            checks += len(tpk) + 1
    if st != [0] * 6 or ts != [0] * 6 or cs != [0] * 3 or idx != [NO_INDEX, 0, NO_INDEX]:
        fails.append("%s: status %s %s %s, indices %s" % (curve, st, ts, cs, idx))
    c.close()
    return fails, checks + 1


def run_open_dev(eng, coracle, curve, torch, device):
    """mp_unmask_ragged_batch_dev: the inputs of the defect batch in buffers of `device` ("cpu" under the emulator, whose device
    pointers are host pointers), the offsets a host array, give the outputs of mp_unmask_ragged_batch"""
    c = Ctx(eng, coracle, curve)
    fails = []
    b, d, _ = open_defects(c)
    lst = [b.plain[0], b.plain[8], b.plain[6]]
    want = b.unmask(c.t, lst, d)
    dev = lambda raw, dt=torch.uint8: torch.frombuffer(bytearray(raw), dtype=dt).to(device)      # noqa: E731
    keys, cards, tk, pf, pl = dev(b"".join(d["keys"])), dev(b"".join(d["cards"])), dev(b"".join(d["tokens"])), dev(b"".join(d["proofs"])), dev(b"".join(lst))
    sg = torch.tensor(d["signer"], dtype=torch.int32).to(device)      # (indices below 2^31: the same bits as uint32)
    out = torch.full((b.C * c.pb,), 0xAA, dtype=torch.uint8, device=device)
    idx = torch.full((b.C,), 7, dtype=torch.int32, device=device)
    ts = torch.full((b.B,), 7, dtype=torch.int32, device=device)
    cs = torch.full((b.C,), 7, dtype=torch.int32, device=device)
    if device != "cpu":
        torch.cuda.synchronize()
    c.t.unmask_ragged_batch_dev(len(d["keys"]), keys.data_ptr(), b.counts, cards.data_ptr(), sg.data_ptr(), tk.data_ptr(), pf.data_ptr(), len(lst),
                                pl.data_ptr(), out.data_ptr(), idx.data_ptr(), ts.data_ptr(), cs.data_ptr())
    eng.sync()
    got = (bytes(out.cpu().numpy().tobytes()), [v & NO_INDEX for v in idx.cpu().tolist()], ts.cpu().tolist(), cs.cpu().tolist())
    if got != want:
        fails.append("%s: mp_unmask_ragged_batch_dev differs from mp_unmask_ragged_batch (token status %s / %s, card status %s / %s)" %
                     (curve, got[2], want[2], got[3], want[3]))
    # a malformed offsets array: MP_ERR_BAD_ARGUMENT, nothing enqueued, the output buffers keep their bytes
    out.fill_(0xAA), idx.fill_(7), ts.fill_(7), cs.fill_(7)
    if device != "cpu":
        torch.cuda.synchronize()
    n = 0
    for name, first in bad_offsets(b.counts):
        arr = (ctypes.c_uint32 * len(first))(*first) if first is not None else None
        rc = c.t.lib.mp_unmask_ragged_batch_dev(c.t.h, len(d["keys"]), keys.data_ptr(), b.C, cards.data_ptr(), arr, sg.data_ptr(), tk.data_ptr(),
                                                pf.data_ptr(), len(lst), pl.data_ptr(), out.data_ptr(), idx.data_ptr(), ts.data_ptr(), cs.data_ptr())
        eng.sync()
        if rc != BAD_ARGUMENT:
            fails.append("%s mp_unmask_ragged_batch_dev, %s: %d, expected %d" % (curve, name, rc, BAD_ARGUMENT))
        n += 1
    if set(out.cpu().tolist()) != {0xAA} or set(idx.cpu().tolist() + ts.cpu().tolist() + cs.cpu().tolist()) != {7}:
        fails.append("%s mp_unmask_ragged_batch_dev: a refused call wrote to its output buffers" % curve)
    c.close()
    return fails, 3 + n


def bad_offsets(counts):
    """(name, offsets array | None) -- each is MP_ERR_BAD_ARGUMENT for a call of len(counts) items"""
    f = offsets(counts)
    C = len(counts)
    assert C >= 3
    zero = list(f)
    zero[2] = zero[1]
    dec = list(f)
    dec[2] = dec[1] - 1
    big = list(f)
    big[C] = MAX_LANES + 1
    return [("first = NULL", None), ("first[0] != 0", [1] + f[1:]), ("a zero count", zero), ("a decreasing entry", dec),
            ("first[C] > 1 048 576", big), ("first[C] > 1 048 576 in one item", f[:C - 1] + [f[C - 1], f[C - 1] + MAX_LANES])]


def run_argument_errors(eng, coracle, curve):
    """null pointers and malformed offsets, on the three host-buffer calls: MP_ERR_BAD_ARGUMENT, and the output buffers keep their bytes"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    lib, h = c.t.lib, c.t.h
    counts = (2, 3, 1)
    C, B = 3, 6
    good = (ctypes.c_uint32 * 4)(*offsets(counts))
    buf = (ctypes.c_uint8 * 8192)()
    outs = [(ctypes.c_uint8 * 8192)() for _ in range(4)]

    def fill():
        for o in outs:
            ctypes.memset(o, 0xAA, 8192)

    def untouched():
        return all(bytes(o) == b"\xAA" * 8192 for o in outs)
    u32 = lambda o: ctypes.cast(o, ctypes.POINTER(ctypes.c_uint32))      # noqa: E731
    i32 = lambda o: ctypes.cast(o, ctypes.POINTER(ctypes.c_int32))       # noqa: E731
    sg = u32(buf)
    on = lambda a, v: v if a is not None else None                       # noqa: E731  (a[k] is None: argument k of the call is NULL)
    calls = {
        "mp_reveal_ragged_batch": lambda f, a: lib.mp_reveal_ragged_batch(h, 1, a[0], a[1], C, a[2], f, on(a[3], sg), a[4], on(a[5], outs[0]),
                                                                           on(a[6], outs[1]), on(a[7], i32(outs[2]))),
        "mp_unmask_ragged_batch": lambda f, a: lib.mp_unmask_ragged_batch(h, 1, a[0], C, a[1], f, on(a[2], sg), a[3], a[4], 0, None, on(a[5], outs[0]),
                                                                           on(a[6], u32(outs[1])), on(a[7], i32(outs[2])), on(a[8], i32(outs[3]))),
        "mp_aggregate_keys_ragged_batch": lambda f, a: lib.mp_aggregate_keys_ragged_batch(h, C, f, a[0], a[1], a[2], on(a[3], outs[0]),
                                                                                           on(a[4], i32(outs[1])), on(a[5], i32(outs[2]))),
    }
    nargs = {"mp_reveal_ragged_batch": 8, "mp_unmask_ragged_batch": 9, "mp_aggregate_keys_ragged_batch": 6}
    fill()
    for fn, call in calls.items():
        for name, first in bad_offsets(counts):
            arr = (ctypes.c_uint32 * len(first))(*first) if first is not None else None
            rc = call(arr, [buf] * nargs[fn])
            if rc != BAD_ARGUMENT:
                fails.append("%s %s, %s: %d, expected %d" % (curve, fn, name, rc, BAD_ARGUMENT))
            checks += 1
        for pos in range(nargs[fn]):
            a = [buf] * nargs[fn]
            a[pos] = None
            if call(good, a) != BAD_ARGUMENT:
                fails.append("%s %s: a null pointer as argument %d is accepted" % (curve, fn, pos))
            checks += 1
        if lib.mp_reveal_ragged_batch(None, 1, buf, buf, C, buf, good, sg, buf, outs[0], outs[1], i32(outs[2])) != BAD_ARGUMENT:
            fails.append("%s: a null table is accepted" % curve)
    # K and the card list past their limits, C = 0
    for name, rc in (("K = 0", lib.mp_unmask_ragged_batch(h, 0, buf, C, buf, good, sg, buf, buf, 0, None, outs[0], u32(outs[1]), i32(outs[2]), i32(outs[3]))),
                     ("K over the limit", lib.mp_reveal_ragged_batch(h, MAX_LANES + 1, buf, buf, C, buf, good, sg, buf, outs[0], outs[1], i32(outs[2]))),
                     ("card list over the limit", lib.mp_unmask_ragged_batch(h, 1, buf, C, buf, good, sg, buf, buf, 4097, buf, outs[0], u32(outs[1]),
                                                                             i32(outs[2]), i32(outs[3]))),
                     ("C = 0", lib.mp_unmask_ragged_batch(h, 1, buf, 0, buf, good, sg, buf, buf, 0, None, outs[0], u32(outs[1]), i32(outs[2]), i32(outs[3]))),
                     ("tables = 0", lib.mp_aggregate_keys_ragged_batch(h, 0, good, buf, buf, buf, outs[0], i32(outs[1]), i32(outs[2])))):
        if rc != BAD_ARGUMENT:
            fails.append("%s %s: %d, expected %d" % (curve, name, rc, BAD_ARGUMENT))
        checks += 1
    if not untouched():
        fails.append("%s: a refused call wrote to its output buffers" % curve)
    c.close()
    return fails, checks + 1


# ---------------------------------------------------------------------------------------------------------------- seating
_SEAT_CACHE = {}


class RaggedSeating:
    """deal_cases.Seating with a count per table: keys, Schnorr proofs and public information of the players; the aggregate keys as
    the oracle sums them.  The edge kinds are those of deal_cases.Seating."""

    def __init__(self, c, counts, salt=0, edges=True):
        self.c, self.counts, self.tables = c, list(counts), len(counts)
        self.first = offsets(counts)
        self.B = self.first[-1]
        key = (c.curve, tuple(counts), salt, edges)
        if key not in _SEAT_CACHE:
            _SEAT_CACHE[key] = self._build(salt, edges)
        d = _SEAT_CACHE[key]
        self.sk, self.kinds, self.pk, self.infos, self.proofs, self.agg = d["sk"], d["kinds"], d["pk"], d["infos"], d["proofs"], d["agg"]

    def _build(self, salt, edges):
        c, q, tables = self.c, self.c.q, self.tables
        rng = random.Random(9100 * tables + 10 * self.B + salt + c.cv.cid)
        sk, kinds = [], []
        for k, P in enumerate(self.counts):
            sks = [rng.randrange(3, q - 1) for _ in range(P)]
            kind = "generic"
            e = (k + tables + P) % 7 if edges else 6
            if e == 0:
                kind, sks[k % P] = "secret key 0", 0
            elif e == 1:
                kind, sks[k % P] = "secret key 1", 1
            elif e == 2:
                kind, sks[k % P] = "secret key q - 1", q - 1
            elif e == 3 and P >= 2:
                kind = "one key twice"
                sks[P - 1] = sks[0]
                if P >= 3:
                    sks[1:P - 1] = [0] * (P - 3) + [sks[0]]
            elif e == 4 and P >= 2:
                kind = "sk and q - sk: the aggregate is O"
                sks = [sks[0], q - sks[0]] + [0] * (P - 2)
            sk += sks
            kinds.append(kind)
        pk = [c.mul(x, c.G) for x in sk]
        infos = [b"player %d" % l + b"!" * (l % 5) for l in range(self.B)]
        seeds = [hashlib.blake2s(b"ragged seat seed %d %d %d %d" % (tables, self.B, salt, l)).digest() for l in range(self.B)]
        proofs = [c.co.sigma_prove(c.curve, 1, c.G, pk[l], c.sc(sk[l]), po.KEY_OWN_RNG_SEED + infos[l], seeds[l]) for l in range(self.B)]
        agg = [c.co.msm(c.curve, c.sc(1) * P, b"".join(pk[self.first[k]:self.first[k + 1]])) for k, P in enumerate(self.counts)]
        return dict(sk=sk, kinds=kinds, pk=pk, infos=infos, proofs=proofs, agg=agg)

    def lanes(self, k):
        return range(self.first[k], self.first[k + 1])

    def fs_raw(self, l, infos=None):
        return po.KEY_OWN_RNG_SEED + (self.infos if infos is None else infos)[l]

    def run(self, t, keys=None, proofs=None, infos=None):
        return t.aggregate_keys_ragged_batch(self.counts, b"".join(self.pk if keys is None else keys), b"".join(self.proofs if proofs is None else proofs),
                                             b"".join(self.c.fs_digest(self.fs_raw(l, infos)) for l in range(self.B)))


def _check_seating(fails, tag, s, got, want_ps):
    c = s.c
    keys, ps, ts = got
    if ps != want_ps:
        fails.append("%s: player status %s, expected %s" % (tag, [(i, v) for i, v in enumerate(ps) if v != want_ps[i]][:8],
                                                            [(i, want_ps[i]) for i, v in enumerate(ps) if v != want_ps[i]][:8]))
    for k in range(s.tables):
        word = next((want_ps[l] for l in s.lanes(k) if want_ps[l] != 0), 0)
        if ts[k] != word:
            fails.append("%s table %d (%s, lanes %d..%d): status %d, expected %d" % (tag, k, s.kinds[k], s.first[k], s.first[k + 1] - 1, ts[k], word))
        if keys[k * c.pb:(k + 1) * c.pb] != (s.agg[k] if word == 0 else c.inf):
            fails.append("%s table %d (%s): aggregate key differs from %s" % (tag, k, s.kinds[k], "the oracle's" if word == 0 else "zero bytes"))
    return s.B + 2 * s.tables


def _seating_against_uniform(fails, tag, t, s, keys, proofs, infos, got):
    """one mp_aggregate_keys_batch call per distinct count on the tables of that count: table by table what the ragged call gave"""
    pb = s.c.pb
    gk, ps, ts = got
    n = 0
    for P, items in sorted(_by_count(s.counts).items()):
        lanes = [l for k in items for l in s.lanes(k)]
        uk, ups, uts = t.aggregate_keys_batch(len(items), P, b"".join(keys[l] for l in lanes), b"".join(proofs[l] for l in lanes),
                                              b"".join(s.c.fs_digest(s.fs_raw(l, infos)) for l in lanes))
        if ups != [ps[l] for l in lanes] or uts != [ts[k] for k in items] or uk != b"".join(gk[k * pb:(k + 1) * pb] for k in items):
            fails.append("%s: the tables of %d players differ between mp_aggregate_keys_ragged_batch and mp_aggregate_keys_batch" % (tag, P))
        n += 3
    return n


def run_seating_case(eng, coracle, curve, case):
    """one honest case: every proof verifies in the oracle and in the engine, the aggregate keys are the oracle's sums and those of the
    uniform call on the tables regrouped by size"""
    name, counts, _ = case
    fails = edge_failures([case])
    if fails:
        return fails, 1
    c = Ctx(eng, coracle, curve)
    s = RaggedSeating(c, counts)
    tag = "%s seating '%s'" % (curve, name)
    for l in range(s.B):
        if coracle.sigma_verify(curve, 1, c.G, s.pk[l], s.proofs[l], s.fs_raw(l)) != 0:
            fails.append("%s lane %d: the oracle refuses its own proof" % (tag, l))
    for k in range(s.tables):
        if s.kinds[k].startswith("sk and q - sk") and s.agg[k] != c.inf:
            fails.append("%s table %d: the case '%s' is not what it says in the oracle" % (tag, k, s.kinds[k]))
    got = s.run(c.t)
    checks = 1 + _check_seating(fails, tag, s, got, [0] * s.B)
    checks += _seating_against_uniform(fails, tag, c.t, s, s.pk, s.proofs, s.infos, got)
    c.close()
    return fails, checks


def run_seating_equal(eng, coracle, curve, shape):
    tables, P = shape
    c = Ctx(eng, coracle, curve)
    s = RaggedSeating(c, (P,) * tables, salt=2)
    proofs = list(s.proofs)
    l = (tables // 2) * P + P - 1
    proofs[l] = proofs[l][:c.pb] + c.sc((int.from_bytes(proofs[l][c.pb:], "little") + 1) % c.q)
    fails = []
    for tag, prf in (("honest", s.proofs), ("one bad seat", proofs)):
        want = c.t.aggregate_keys_batch(tables, P, b"".join(s.pk), b"".join(prf), b"".join(c.fs_digest(s.fs_raw(i)) for i in range(s.B)))
        if s.run(c.t, proofs=prf) != want:
            fails.append("%s (%d, %d) %s: mp_aggregate_keys_ragged_batch differs from mp_aggregate_keys_batch" % (curve, tables, P, tag))
        if [k for k, v in enumerate(want[2]) if v] != ([] if prf is s.proofs else [tables // 2]):
            fails.append("%s (%d, %d) %s: table status %s" % (curve, tables, P, tag, want[2]))
    c.close()
    return fails, 4


def seating_defects(c):
    """-> (seating, keys, proofs, infos, expected player words): a tampered proof at the first seat of table 1 and at the last seat of
    table 3, which has an earlier seat with another word (the first counts); a proof for another fs_init at the one-seat table 2; a key
    off the curve at table 5"""
    s = RaggedSeating(c, DEFECT_COUNTS, salt=13, edges=False)
    keys, proofs, infos = list(s.pk), list(s.proofs), list(s.infos)
    f, pb = s.first, c.pb
    z1 = lambda p: p[:pb] + c.sc((int.from_bytes(p[pb:], "little") + 1) % c.q)      # noqa: E731
    proofs[f[1]] = z1(proofs[f[1]])
    proofs[f[4] - 1] = z1(proofs[f[4] - 1])
    proofs[f[3] + 1] = proofs[f[3] + 1][:pb] + c.sc(c.q)          # table 3: an earlier seat with another word: the first counts
    infos[f[2]] = b"somebody else"                                # the one-seat table: a proof for another fs_init
    keys[f[5] + 3] = c.off_curve(keys[f[5] + 3])
    want = []
    for l in range(s.B):
        if l in (f[3] + 1, f[5] + 3):
            want.append(BAD_ENCODING)
        else:
            want.append(c.co.sigma_verify(c.curve, 1, c.G, keys[l], proofs[l], s.fs_raw(l, infos)))
    assert [l for l in range(s.B) if want[l] == SCHNORR] == [f[1], f[2], f[4] - 1] and sum(1 for v in want if v == 0) == s.B - 5, want
    return s, keys, proofs, infos, want


def run_seating_defects(eng, coracle, curve):
    c = Ctx(eng, coracle, curve)
    fails = []
    s, keys, proofs, infos, want = seating_defects(c)
    got = s.run(c.t, keys=keys, proofs=proofs, infos=infos)
    checks = _check_seating(fails, "%s seating defects" % curve, s, got, want)
    checks += _seating_against_uniform(fails, "%s seating defects" % curve, c.t, s, keys, proofs, infos, got)
    if got[2] != [0, SCHNORR, SCHNORR, BAD_ENCODING, 0, BAD_ENCODING, 0, 0, 0]:
        fails.append("%s seating defects: table status %s" % (curve, got[2]))
    c.close()
    return fails, checks + 1


# ---------------------------------------------------------------------------------------------------------------- the screen
def run_screen(eng, coracle, curve):
    """the ragged verifiers on a table with set_sigma_screen(g, 1), g the group sizes of tests/sigma_screen_cases.py: the words and bytes
    of the unscreened table, for the mixed honest case and for the defects; and the calls did go through the screen -- under AUTO, which
    leaves such small calls on the per-proof path, a call of 1 206 lanes as well, where it must have run"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    hb = Ragged(c, MIXED[1])
    hs = RaggedSeating(c, MIXED[1])
    b, d, _ = open_defects(c)
    s, keys, proofs, infos, _ = seating_defects(c)
    lst = hb.card_list()
    calls = [("unmask, honest", hb.B, lambda t: hb.unmask(t, lst)), ("unmask, defects", b.B, lambda t: b.unmask(t, lst, d)),
             ("seating, honest", hs.B, lambda t: hs.run(t)), ("seating, defects", s.B, lambda t: s.run(t, keys=keys, proofs=proofs, infos=infos))]
    want = [f(c.t) for _, _, f in calls]
    for g in SCREEN_GROUPS:
        on = eng.table(c.t.m, c.t.n, c.params, c.pk)
        on.set_sigma_screen(g, 1)
        for (name, lanes, f), w in zip(calls, want):
            before = on.sigma_screen_stats()
            got = f(on)
            grew = [x - y for x, y in zip(on.sigma_screen_stats(), before)]
            if got != w:
                fails.append("%s %s, groups of %#x: the screened call differs from the unscreened one (stats +%s)" % (curve, name, g, grew))
            # (groups of 64: every call is screened; AUTO keeps calls too small for groups of 16 lanes on the per-proof path)
            screened = grew[0] == lanes or (g == SCREEN_GROUPS[1] and grew == [0, 0, 0, 0])
            if not screened or (name.endswith("honest") and grew[2:] != [0, 0]) or (name.endswith("defects") and grew[0] and grew[2] == 0):
                fails.append("%s %s, groups of %#x: sigma_screen_stats grew by %s for %d lanes" % (curve, name, g, grew, lanes))
            checks += 2
        on.close()
    # AUTO on a call large enough for it (64 equations of at least 16 lanes): the mixed counts eighteen times over, 1 206 lanes, tokens
    # and proofs from mp_reveal_ragged_batch (held to the oracle elsewhere).  The screen must have run over every lane; with one token
    # replaced some group fails, and the words and bytes stay those of the unscreened table
    counts = list(MIXED[1]) * AUTO_REPEAT
    first = offsets(counts)
    B = first[-1]
    cards = [c.pool[1 + i % 15] + c.pool[1 + (3 * i + 1) % 15] for i in range(len(counts))]
    signer = [7 + (i + 3 * j) % (hb.K - 7) for i, n in enumerate(counts) for j in range(n)]
    seeds = b"".join(hashlib.blake2s(b"ragged screen seed %d" % l).digest() for l in range(B))
    keys = b"".join(hb.pk)
    tok, prf, st = c.t.reveal_ragged_batch(keys, hb.secret_bytes(), b"".join(cards), counts, signer, seeds)
    if any(st) or B < 64 * 16:
        fails.append("%s AUTO: reveal status %s for %d lanes" % (curve, [(i, v) for i, v in enumerate(st) if v][:8], B))
    bad = tok[:first[100] * c.pb] + c.pool[0] + tok[(first[100] + 1) * c.pb:]
    on = eng.table(c.t.m, c.t.n, c.params, c.pk)
    on.set_sigma_screen(SCREEN_GROUPS[1], 1)
    for name, tokens in (("honest", tok), ("one bad token", bad)):
        w = c.t.unmask_ragged_batch(keys, b"".join(cards), counts, signer, tokens, prf)
        before = on.sigma_screen_stats()
        got = on.unmask_ragged_batch(keys, b"".join(cards), counts, signer, tokens, prf)
        grew = [x - y for x, y in zip(on.sigma_screen_stats(), before)]
        if got != w or [i for i, v in enumerate(w[3]) if v] != ([] if tokens is tok else [100]):
            fails.append("%s AUTO, %s: the screened call differs from the unscreened one (card status %s, stats +%s)" %
                         (curve, name, [(i, v) for i, v in enumerate(w[3]) if v], grew))
        # (BLS12-377: the one-wave bucket kernel is off for the 14-limb field -- engine_core.hpp group_points = 0 --, so AUTO screens only
        # calls of 40 000 points = 8 000 opening lanes and more, too many for a quick test: this call must stay on the per-proof path there,
        # and the leg with groups of 64 above is what shows the screen on that curve)
        if curve == "bls12_377":
            wrong = grew != [0, 0, 0, 0]
        else:
            wrong = grew[0] != B or grew[1] < 1 or (tokens is tok and grew[2:] != [0, 0]) or (tokens is bad and grew[2] < 1)
        if wrong:
            fails.append("%s AUTO, %s: sigma_screen_stats grew by %s for %d lanes" % (curve, name, grew, B))
        checks += 2
    on.close()
    c.close()
    return fails, checks


# ---------------------------------------------------------------------------------------------------------------- chains
CHAIN_LINKS = [3, 1, 2, 3, 1]        # groups of two, two and one tables
CHAIN_MN = (2, 3)                    # the small deck of the chain tests (tests/test_cabi_and_host.py, tests/test_gpu_round4.py)
_CHAIN_CACHE = {}


def _chains(coracle, cvn, m, n, links, keyed):
    """per table (key, [decks], [proofs]) as the oracle shuffles them"""
    key = (cvn, m, n, tuple(links), keyed)
    if key not in _CHAIN_CACHE:
        g0 = coracle.gen_inputs(cvn, m, n, 50)
        out = []
        for t, L in enumerate(links):
            pk = coracle.gen_inputs(cvn, m, n, 60 + t)["pk"] if keyed else g0["pk"]
            decks, proofs = [coracle.gen_inputs(cvn, m, n, 70 + t)["deck"]], []
            for j in range(L):
                gi = coracle.gen_inputs(cvn, m, n, 100 + 10 * j + t)
                d, p = coracle.shuffle_and_remask(cvn, m, n, g0["params"], pk, decks[j], gi["rho"], gi["perm"], gi["prover_seed"])
                decks.append(d)
                proofs.append(p)
            out.append((pk, decks, proofs))
        _CHAIN_CACHE[key] = (g0, out)
    return _CHAIN_CACHE[key]


def _flat(chains, keyed, proofs=None):
    """table-major: the decks of table 0, then those of table 1, ...; proofs and keys likewise"""
    return (b"".join(b"".join(dk) for _, dk, _ in chains), b"".join(b"".join(proofs[t] if proofs else pf) for t, (_, _, pf) in enumerate(chains)),
            b"".join(pk * len(pf) for pk, _, pf in chains) if keyed else None)


def run_chains(eng, coracle, keyed, cvn="stark"):
    """mp_verify_shuffle_chain_ragged on links = [3, 1, 2, 3, 1]: honest chains give 0 everywhere; with a proof swapped at link 1 of
    table 0 and at the only link of table 1 exactly those two words are not 0 and the vector equals mp_verify_shuffle_batch[_keys] link
    by link; equal links give the words of mp_verify_shuffle_chain after transposing the layout; argument errors"""
    m, n = CHAIN_MN
    links = CHAIN_LINKS
    g0, chains = _chains(coracle, cvn, m, n, links, keyed)
    off = offsets(links)
    fails = []
    if sorted(len(v) for v in _by_count(links).values()) != [1, 2, 2] or off != [0, 3, 4, 6, 9, 10]:
        fails.append("links %s do not give groups of two, two and one tables" % links)
    table = eng.table(m, n, g0["params"], None if keyed else g0["pk"])
    decks, pf, keys = _flat(chains, keyed)
    st = table.verify_shuffle_chain_ragged(links, decks, pf, keys)
    if st != [0] * off[-1]:
        fails.append("honest chains: status %s" % st)
    # table 0, link 1 gets the proof of table 3, link 1 (the other table of its group); table 1's only link that of table 4
    bad = [list(p) for _, _, p in chains]
    bad[0][1] = chains[3][2][1]
    bad[1][0] = chains[4][2][0]
    decks, bpf, keys = _flat(chains, keyed, bad)
    st = table.verify_shuffle_chain_ragged(links, decks, bpf, keys)
    exp = []
    for t, (pk, dk, _) in enumerate(chains):
        for j in range(links[t]):
            exp += (table.verify_shuffle_batch_keys(pk, dk[j], dk[j + 1], bad[t][j]) if keyed else table.verify_shuffle_batch(dk[j], dk[j + 1], bad[t][j]))
    if st != exp or [i for i, v in enumerate(st) if v] != [off[0] + 1, off[1]] or any(v < 0 for v in st):
        fails.append("tampered chains: status %s, link by link %s" % (st, exp))
    # the chain settings apply to every group: sub-chains of two links and passes of one table, same words
    table.set_chain_max_links(2)
    table.set_chain_slice(1)
    try:
        if table.verify_shuffle_chain_ragged(links, decks, bpf, keys) != exp:
            fails.append("tampered chains, sub-chains of 2 links and passes of 1 table: the words differ")
    finally:
        table.set_chain_max_links(0)
        table.set_chain_slice(0)
    # equal links: tables 0 and 3 (3 links each), once ragged and table-major, once uniform and link-major
    pair = [(chains[0][0], chains[0][1], bad[0]), chains[3]]
    d2, p2, k2 = _flat(pair, keyed)
    rag = table.verify_shuffle_chain_ragged([3, 3], d2, p2, k2)
    uni = table.verify_shuffle_chain(2, 3, b"".join(pair[t][1][j] for j in range(4) for t in range(2)),
                                     b"".join(pair[t][2][j] for j in range(3) for t in range(2)),
                                     b"".join(pair[t][0] for j in range(3) for t in range(2)) if keyed else None)
    if rag != [uni[j * 2 + t] for t in range(2) for j in range(3)] or [i for i, v in enumerate(rag) if v] != [1]:
        fails.append("equal links: ragged %s, uniform (link-major) %s" % (rag, uni))
    # argument errors
    lib, h = table.lib, table.h
    buf = (ctypes.c_uint8 * 64)()
    stw = (ctypes.c_int32 * 16)(*([7] * 16))
    kb = buf if keyed else None
    for name, tables, lk in (("links[t] == 0", 3, [2, 0, 1]), ("tables == 0", 0, [1]), ("links[t] over the limit", 2, [1, 4096]), ("links = NULL", 2, None)):
        arr = (ctypes.c_uint32 * len(lk))(*lk) if lk is not None else None
        rc = lib.mp_verify_shuffle_chain_ragged(h, tables, arr, kb, buf, buf, stw)
        if rc != BAD_ARGUMENT:
            fails.append("mp_verify_shuffle_chain_ragged, %s: %d, expected %d" % (name, rc, BAD_ARGUMENT))
    if list(stw) != [7] * 16:
        fails.append("mp_verify_shuffle_chain_ragged: a refused call wrote status words")
    table.close()
    return fails, 12
