"""Cases, references and checks for the opening phase: mp_reveal_batch (a player's reveal tokens with their Chaum-Pedersen proofs),
mp_unmask_batch (whoever opens: verification, c1 - sum of the tokens, card lookup) and mp_unmask_batch_dev, on every curve.  Shared by
tests/test_open_emu.py (the kernel bodies under the development emulator, CPU) and tests/test_gpu_open.py (the gfx950 build) -- same
cases, same expectations: exact equality with the C++ oracle (coracle.sigma_prove, coracle.sigma_verify, coracle.msm) and, for one tiny
batch, with the Python oracle's compute_reveal_token / unmask as well.

A batch is C cards with T tokens each; lane c * T + j is token j of card c.  Every run_* function takes an engine (_native.Engine), the
coracle module and a curve name, and returns (failure messages, number of checks made); the tests assert that the list is empty."""
import ctypes
import hashlib
import random

import mp_oracle as po
from trait_cases import BAD_ENCODING, CURVES, Ctx, M_, N_, off_subgroup_points  # noqa: F401  (CURVES: for the test files)

SHAPES = [(1, 1), (7, 9), (8, 8), (13, 5), (257, 1)]      # 1, 63, 64, 65 lanes and 257 lanes / cards: around a wave and a block
STARK_EXTRA = [(52, 4)]                                    # a deck at a table of four
PO_SHAPE = (2, 3)                                          # the batch that is also compared with the Python oracle
BAD_ARGUMENT = -3                                          # MP_ERR_BAD_ARGUMENT (include/mpshuffle.h)
CHAUM_PEDERSEN = 6
NO_INDEX = 0xFFFFFFFF
REVEAL = po.REVEAL_RNG_SEED


def shapes(curve):
    return SHAPES + (STARK_EXTRA if curve == "stark" else [])


class Batch:
    """keys, cards, signers, prover seeds; tokens, proofs and plaintexts as the oracle computes them"""

    def __init__(self, c, C, T, salt=0, edges=True):
        self.c, self.C, self.T = c, C, T
        q = c.q
        rng = random.Random(4000 * C + 10 * T + salt + c.cv.cid)
        # players 0..4: the edge keys (token = O, +-c0, ...); 5 and 6: sk and q - sk (their tokens cancel); the rest random
        self.sk = [0, 1, q - 1, (q - 1) // 2, (q + 1) // 2]
        s = rng.randrange(3, q - 1)
        self.sk += [s, q - s] + [rng.randrange(3, q - 1) for _ in range(max(T, 3))]
        self.K = len(self.sk)
        self.pk = [c.mul(k, c.G) for k in self.sk]
        self.cards, self.signer, self.kinds = [], [], []
        for i in range(C):
            c0, c1 = c.pool[1 + (i + C) % 15], c.pool[1 + (3 * i + T) % 15]
            sg = [(i + 3 * j + T) % self.K for j in range(T)]          # walks through the edge keys as well
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
                kind = "sum of the tokens = c1"                         # c1 is set below, once the tokens are known
                sg = [7 + j % (self.K - 7) for j in range(T)]
            elif k == 6 and T >= 3:
                kind = "two tokens cancel"
                sg[1], sg[2] = 5, 6
            self.kinds.append(kind)
            if kind == "sum of the tokens = c1":
                toks = [c.mul(self.sk[g], c0) for g in sg]
                c1 = c.co.msm(c.curve, c.sc(1) * T, b"".join(toks))
            self.cards.append(c0 + c1)
            self.signer += sg
        self.seeds = [hashlib.blake2s(b"reveal seed %d %d %d %d" % (C, T, salt, b)).digest() for b in range(C * T)]
        self.tokens, self.proofs = [], []
        for b in range(C * T):
            c0, g = self.cards[b // T][:c.pb], self.signer[b]
            tok = c.mul(self.sk[g], c0)
            self.tokens.append(tok)
            self.proofs.append(c.co.sigma_prove(c.curve, 2, c0 + c.G, tok + self.pk[g], c.sc(self.sk[g]), REVEAL, self.seeds[b]))
        self.plain = [self.plain_of(i, self.tokens[i * T:(i + 1) * T]) for i in range(C)]

    def plain_of(self, i, toks):
        c = self.c
        return c.co.msm(c.curve, c.sc(1) + c.sc(c.q - 1) * len(toks), self.cards[i][c.pb:] + b"".join(toks))

    def card_list(self, with_identity):
        """the true card of the first, the middle and the last card of the batch first, in the middle and last in the list; the first
        one a second time further down (the smaller index counts); other points in between; every other card is absent -- unless it
        opens to the same point as one of the three.  The identity (several edge cards open to it) is in the list or not."""
        c, C = self.c, self.C
        rng = random.Random(77 + C + self.T)
        fill = lambda: c.mul(rng.randrange(3, c.q - 1), c.G)
        lst = [self.plain[0], fill(), fill()]
        if with_identity:
            lst.append(c.inf)
        lst += [self.plain[C // 2], fill(), self.plain[0], fill(), self.plain[C - 1]]
        if not with_identity:
            lst = [p for p in lst if p != c.inf] or [fill()]
        return lst

    def keys_bytes(self):
        return b"".join(self.pk)

    def reveal(self, t):
        return t.reveal_batch(self.keys_bytes(), b"".join(self.c.sc(k) for k in self.sk), b"".join(self.cards), self.T, self.signer,
                              b"".join(self.seeds))

    def unmask(self, t, lst, keys=None, cards=None, signer=None, tokens=None, proofs=None):
        return t.unmask_batch(keys if keys is not None else self.keys_bytes(), b"".join(cards if cards is not None else self.cards), self.T,
                              signer if signer is not None else self.signer, b"".join(tokens if tokens is not None else self.tokens),
                              b"".join(proofs if proofs is not None else self.proofs), b"".join(lst))


def _check_open(fails, tag, b, got, lst, want_ts):
    """got = (plaintexts, indices, token_status, card_status) of one unmask call against the expectations of batch b: cards whose
    tokens all have status 0 open to the oracle's plaintext and its index in lst, the others to zero bytes and no index"""
    c, C, T = b.c, b.C, b.T
    plain, idx, ts, cs = got
    n = 0
    if ts != want_ts:
        fails.append("%s: token status %s, expected %s" % (tag, [(i, v) for i, v in enumerate(ts) if v != want_ts[i]][:8],
                                                           [(i, want_ts[i]) for i, v in enumerate(ts) if v != want_ts[i]][:8]))
    for i in range(C):
        first = next((v for v in want_ts[i * T:(i + 1) * T] if v != 0), 0)
        if cs[i] != first:
            fails.append("%s card %d (%s): card status %d, expected %d" % (tag, i, b.kinds[i], cs[i], first))
        wp = b.plain[i] if first == 0 else c.inf
        wi = (lst.index(wp) if wp in lst else NO_INDEX) if first == 0 else NO_INDEX
        if plain[i * c.pb:(i + 1) * c.pb] != wp:
            fails.append("%s card %d (%s): plaintext differs from the oracle's" % (tag, i, b.kinds[i]))
        if idx[i] != wi:
            fails.append("%s card %d (%s): index %#x, expected %#x" % (tag, i, b.kinds[i], idx[i], wi))
        n += 3
    return n + C * T


def run_honest(eng, coracle, curve, shape_list=None, edges=True):
    """reveal: tokens and proofs equal the oracle's lane by lane; unmask: all statuses 0, plaintexts and indices right, with the identity
    in the card list and without it"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    for C, T in (shape_list if shape_list is not None else shapes(curve)):
        b = Batch(c, C, T, edges=edges)
        tag = "%s (%d, %d)" % (curve, C, T)
        for i in range(C):      # the edge cards are what they say, in the oracle
            if (b.kinds[i] == "sum of the tokens = c1" and b.plain[i] != c.inf) or \
                    (b.kinds[i] == "sum of the tokens = O" and b.plain[i] != b.cards[i][c.pb:]):
                fails.append("%s card %d: the case '%s' is not what it says in the oracle" % (tag, i, b.kinds[i]))
        tok, prf, st = b.reveal(c.t)
        if st != [0] * (C * T):
            fails.append("%s: reveal status %s" % (tag, [(i, v) for i, v in enumerate(st) if v][:8]))
        psz = 2 * c.pb + 32
        for l in range(C * T):
            if tok[l * c.pb:(l + 1) * c.pb] != b.tokens[l]:
                fails.append("%s lane %d (%s, signer %d): token differs from the oracle's" % (tag, l, b.kinds[l // T], b.signer[l]))
            if prf[l * psz:(l + 1) * psz] != b.proofs[l]:
                fails.append("%s lane %d (%s, signer %d): proof differs from the oracle's" % (tag, l, b.kinds[l // T], b.signer[l]))
        checks += 3 * C * T
        for with_identity in (True, False):
            lst = b.card_list(with_identity)
            got = b.unmask(c.t, lst, tokens=[tok[l * c.pb:(l + 1) * c.pb] for l in range(C * T)],
                           proofs=[prf[l * psz:(l + 1) * psz] for l in range(C * T)])
            checks += _check_open(fails, "%s, identity %s the list" % (tag, "in" if with_identity else "not in"), b, got, lst, [0] * (C * T))
        # no card list at all: plaintexts only
        got = b.unmask(c.t, [])
        checks += _check_open(fails, tag + ", no list", b, got, [], [0] * (C * T))
    c.close()
    return fails, checks


def run_python_oracle(eng, coracle, curve):
    """the third restatement on one tiny batch: po.compute_reveal_token and po.unmask"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    C, T = PO_SHAPE
    b = Batch(c, C, T, salt=5, edges=False)
    tok, prf, st = b.reveal(c.t)
    plain, idx, ts, cs = b.unmask(c.t, [b.plain[1]])
    psz = 2 * c.pb + 32
    with po.curve_ctx(c.cv):
        pts = [po.pt_from_wire(c.params[i * c.pb:(i + 1) * c.pb]) for i in range(N_ + 3)]
        pp = po.Params(c.cv, M_, N_, pts[0], pts[1:1 + N_], pts[1 + N_], pts[2 + N_])
        for i in range(C):
            masked = (po.pt_from_wire(b.cards[i][:c.pb]), po.pt_from_wire(b.cards[i][c.pb:]))
            tpk = []
            for j in range(T):
                l, g = i * T + j, b.signer[i * T + j]
                pk = po.pt_from_wire(b.pk[g])
                token, proof = po.compute_reveal_token(pp, b.sk[g], pk, masked, b.seeds[l])
                if po.pt_wire(token) != tok[l * c.pb:(l + 1) * c.pb] or po.sigma_proof_bytes(proof) != prf[l * psz:(l + 1) * psz]:
                    fails.append("%s lane %d: token or proof differs from the Python oracle's" % (curve, l))
                tpk.append((token, proof, pk))
            if po.pt_wire(po.unmask(pp, tpk, masked)) != plain[i * c.pb:(i + 1) * c.pb]:
                fails.append("%s card %d: plaintext differs from the Python oracle's" % (curve, i))
            checks += T + 1
    if st != [0] * (C * T) or ts != [0] * (C * T) or cs != [0] * C or idx != [NO_INDEX, 0]:
        fails.append("%s: status %s %s %s, indices %s" % (curve, st, ts, cs, idx))
    c.close()
    return fails, checks + 1


def _noncanonical(c, P):
    """x replaced by p: a coordinate that is not reduced"""
    return c.p.to_bytes(c.fb, "little") + P[c.fb:]


def defect_list(c, b):
    """(name, expected token status, edit) -- edit(d) changes the dictionary of the batch's inputs for the lane `d["lane"]`; the last
    two entries touch a card point: every token of the card then has the status"""
    pb, q = c.pb, c.q
    spare = c.pool[0]

    def proof_part(name, f, want):
        def edit(d):
            l = d["lane"]
            d["proofs"][l] = f(d["proofs"][l])
        return (name, want, edit)

    def token(name, f, want):
        def edit(d):
            d["tokens"][d["lane"]] = f(d["tokens"][d["lane"]])
        return (name, want, edit)

    def signer(name, f, want):
        def edit(d):
            d["signer"][d["lane"]] = f(d["signer"][d["lane"]])
        return (name, want, edit)

    def bad_key(name, f):
        def edit(d):
            l = d["lane"]
            d["keys"].append(f(d["keys"][d["signer"][l]]))      # a key of its own, named by this lane alone
            d["signer"][l] = len(d["keys"]) - 1
        return (name, BAD_ENCODING, edit)

    def card(name, half, f):
        def edit(d):
            i = d["lane"] // b.T
            cd = d["cards"][i]
            d["cards"][i] = f(cd[:pb]) + cd[pb:] if half == 0 else cd[:pb] + f(cd[pb:])
        return (name, BAD_ENCODING, edit)

    z_of = lambda p: int.from_bytes(p[2 * pb:], "little")
    out = [
        token("token replaced by another point", lambda t: spare, CHAUM_PEDERSEN),
        proof_part("A_0 replaced", lambda p: spare + p[pb:], CHAUM_PEDERSEN),
        proof_part("A_1 replaced", lambda p: p[:pb] + spare + p[2 * pb:], CHAUM_PEDERSEN),
        proof_part("z + 1", lambda p: p[:2 * pb] + c.sc((z_of(p) + 1) % q), CHAUM_PEDERSEN),
        signer("signer names another key", lambda g: (g + 1) % b.K if (g + 1) % b.K not in (5, 6) else 8, CHAUM_PEDERSEN),
        signer("signer = K", lambda g: -1, BAD_ARGUMENT),      # (run_defects puts K there once the key list is complete)
        token("token off the curve", c.off_curve, BAD_ENCODING),
        token("token with a coordinate that is not reduced", lambda t: _noncanonical(c, t), BAD_ENCODING),
        proof_part("z = q", lambda p: p[:2 * pb] + c.sc(q), BAD_ENCODING),
        proof_part("A_1 off the curve", lambda p: p[:pb] + c.off_curve(p[pb:2 * pb]) + p[2 * pb:], BAD_ENCODING),
        bad_key("key off the curve", c.off_curve),
        card("c0 off the curve", 0, c.off_curve),
        card("c1 off the curve", 1, c.off_curve),
    ]
    return out


def _inputs(b):
    return dict(keys=list(b.pk), cards=list(b.cards), signer=list(b.signer), tokens=list(b.tokens), proofs=list(b.proofs))


def _statement(c, d, l, T):
    """host-assembled statement of lane l, as mp_sigma_verify_batch takes it"""
    return d["cards"][l // T][:c.pb] + c.G, d["tokens"][l] + d["keys"][d["signer"][l]], d["proofs"][l]


def run_defects(eng, coracle, curve):
    """one defect per card in a batch of generic cards (random keys only: every defect is a defect); every other card and token stays 0
    and opens correctly.  Then the call-level refusals."""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    probe = Batch(c, 1, 1, edges=False)
    ndef = len(defect_list(c, probe))
    C, T = ndef + 2, 5
    b = Batch(c, C, T, salt=11, edges=False)
    b.signer = [7 + (3 * l + l // T) % (b.K - 7) for l in range(C * T)]      # random keys only
    b.tokens = [c.mul(b.sk[b.signer[l]], b.cards[l // T][:c.pb]) for l in range(C * T)]
    b.proofs = [coracle.sigma_prove(curve, 2, b.cards[l // T][:c.pb] + c.G, b.tokens[l] + b.pk[b.signer[l]], c.sc(b.sk[b.signer[l]]), REVEAL,
                                    b.seeds[l]) for l in range(C * T)]
    b.plain = [b.plain_of(i, b.tokens[i * T:(i + 1) * T]) for i in range(C)]
    defects = defect_list(c, b)
    d = _inputs(b)
    want = [0] * (C * T)
    for k, (name, code, edit) in enumerate(defects):
        i = k + 1                                   # cards 0 and C - 1 stay honest
        j = k % T                                   # the place of the bad token moves through the card
        d["lane"] = i * T + j
        edit(d)
        b.kinds[i] = name
        if name.startswith("c0 ") or name.startswith("c1 "):
            for jj in range(T):
                want[i * T + jj] = code
        else:
            want[i * T + j] = code
        if code == CHAUM_PEDERSEN:
            g, a, pf = _statement(c, d, i * T + j, T)
            if coracle.sigma_verify(curve, 2, g, a, pf, REVEAL) == 0:
                fails.append("%s: the oracle accepts the case '%s'" % (curve, name))
    d["signer"] = [len(d["keys"]) if g == -1 else g for g in d["signer"]]
    lst = [b.plain[0], b.plain[C - 1]] + b.plain[1:3]
    got = b.unmask(c.t, lst, keys=b"".join(d["keys"]), cards=d["cards"], signer=d["signer"], tokens=d["tokens"], proofs=d["proofs"])
    checks += _check_open(fails, "%s defects" % curve, b, got, lst, want)
    # ---- call level
    honest = Batch(c, 2, 2, salt=3, edges=False)
    for name, bad in (("off the curve", c.off_curve(c.pool[3])), ("not reduced", _noncanonical(c, c.pool[3]))):
        try:
            honest.unmask(c.t, [honest.plain[0], bad])
            fails.append("%s: a card list with an entry %s is accepted" % (curve, name))
        except Exception as e:
            if getattr(e, "code", None) != BAD_ENCODING:
                fails.append("%s: a card list with an entry %s gives %r" % (curve, name, e))
        checks += 1
    lib, h = c.t.lib, c.t.h
    buf = (ctypes.c_uint8 * 4096)()
    big = 1048576
    for name, (K, Cn, Tn, npl) in (("T = 0", (1, 1, 0, 0)), ("C = 0", (1, 0, 1, 0)), ("K = 0", (0, 1, 1, 0)), ("C T over the limit", (1, big // 4 + 1, 4, 0)),
                                   ("C T over the limit, T large", (1, 3, big // 2, 0)), ("K over the limit", (big + 1, 1, 1, 0)),
                                   ("card list over the limit", (1, 1, 1, 4097))):
        rc = lib.mp_unmask_batch(h, K, buf, Cn, buf, Tn, buf, buf, buf, npl, buf, buf, buf, buf, buf)
        if rc != BAD_ARGUMENT:
            fails.append("%s unmask, %s: %d, expected %d" % (curve, name, rc, BAD_ARGUMENT))
        if npl == 0:
            rc = lib.mp_reveal_batch(h, K, buf, buf, Cn, buf, Tn, buf, buf, buf, buf, buf)
            if rc != BAD_ARGUMENT:
                fails.append("%s reveal, %s: %d, expected %d" % (curve, name, rc, BAD_ARGUMENT))
        checks += 2
    # the prover's side: a secret key >= q, a card off the curve and a signer past the keys, between honest lanes
    hb = Batch(c, 4, 2, salt=9, edges=False)
    sg = [7, 8, 3, 9, 7, 8, 9, hb.K]
    sks = [c.sc(k) for k in hb.sk]
    sks[3] = c.sc(c.q)
    cards = list(hb.cards)
    cards[2] = c.off_curve(cards[2][:c.pb]) + cards[2][c.pb:]
    tok, prf, st = c.t.reveal_batch(hb.keys_bytes(), b"".join(sks), b"".join(cards), 2, sg, b"".join(hb.seeds))
    wst = [0, 0, BAD_ENCODING, 0, BAD_ENCODING, BAD_ENCODING, 0, BAD_ARGUMENT]
    if st != wst:
        fails.append("%s reveal with refused lanes: status %s, expected %s" % (curve, st, wst))
    psz = 2 * c.pb + 32
    for l in (0, 1, 6):
        ref_tok = c.mul(hb.sk[sg[l]], hb.cards[l // 2][:c.pb])
        ref = coracle.sigma_prove(curve, 2, hb.cards[l // 2][:c.pb] + c.G, ref_tok + hb.pk[sg[l]], c.sc(hb.sk[sg[l]]), REVEAL, hb.seeds[l])
        if tok[l * c.pb:(l + 1) * c.pb] != ref_tok or prf[l * psz:(l + 1) * psz] != ref:
            fails.append("%s reveal lane %d (honest, next to refused ones): differs from the oracle's" % (curve, l))
    checks += 8
    c.close()
    return fails, checks


def run_subgroup(eng, coracle, curve="bls12_377"):
    """BLS12-377: each kind of point outside the subgroup as token, as key and as commitment A_0, one per card: refused as a bad encoding,
    and only there; with the table's subgroup test off, what the algebra gives (the oracle's verdict, and the oracle's plaintext for a
    card whose tokens all pass)"""
    assert curve == "bls12_377"
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    kinds = list(zip(("low-order point", "point before cofactor clearing", "subgroup point + low-order point"), off_subgroup_points()))
    places = ("token", "key", "A_0")
    C, T = len(kinds) * len(places) + 2, 3
    b = Batch(c, C, T, salt=21, edges=False)
    d = _inputs(b)
    want = [0] * (C * T)
    k = 0
    for kname, pt in kinds:
        for place in places:
            i = k + 1
            l = i * T + k % T
            if place == "token":
                d["tokens"][l] = pt
            elif place == "key":
                d["keys"].append(pt)
                d["signer"][l] = len(d["keys"]) - 1
            else:
                d["proofs"][l] = pt + d["proofs"][l][c.pb:]
            b.kinds[i] = "%s as %s" % (kname, place)
            want[l] = BAD_ENCODING
            k += 1
    lst = [b.plain[0], b.plain[C - 1]]
    args = dict(keys=b"".join(d["keys"]), cards=d["cards"], signer=d["signer"], tokens=d["tokens"], proofs=d["proofs"])
    checks += _check_open(fails, "bls12_377 subgroup", b, b.unmask(c.t, lst, **args), lst, want)
    c.t.set_subgroup_check(False)
    try:
        got = b.unmask(c.t, lst, **args)
    finally:
        c.t.set_subgroup_check(True)
    want2 = [coracle.sigma_verify(curve, 2, *_statement(c, d, l, T), REVEAL) for l in range(C * T)]
    for i in range(C):
        if not any(want2[i * T:(i + 1) * T]):
            b.plain[i] = b.plain_of(i, d["tokens"][i * T:(i + 1) * T])
    checks += _check_open(fails, "bls12_377 subgroup test off", b, got, lst, want2)
    if not all(want2[l] in (0, CHAUM_PEDERSEN) for l in range(C * T)):
        fails.append("bls12_377 subgroup test off: the oracle's verdicts are %s" % want2)
    c.close()
    return fails, checks


def run_agreement(eng, coracle, curve):
    """one (13, 5) batch with two defects: token_status equals what mp_sigma_verify_batch says for the host-assembled statements, and the
    proofs of mp_reveal_batch are those of mp_sigma_prove_batch"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    C, T = 13, 5
    b = Batch(c, C, T, salt=31)
    d = _inputs(b)
    d["tokens"][3 * T + 2] = c.pool[0]
    p = d["proofs"][7 * T + 4]
    d["proofs"][7 * T + 4] = p[:2 * c.pb] + c.sc(c.q)
    _, _, ts, _ = b.unmask(c.t, [], tokens=d["tokens"], proofs=d["proofs"])
    rows = [_statement(c, d, l, T) for l in range(C * T)]
    fs = eng.blake2s(REVEAL) * (C * T)
    sv = c.t.sigma_verify_batch(2, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[2] for r in rows), fs)
    if ts != sv or sv[3 * T + 2] != CHAUM_PEDERSEN or sv[7 * T + 4] != BAD_ENCODING or sum(1 for v in sv if v) != 2:
        fails.append("%s: token status %s, mp_sigma_verify_batch %s" % (curve, [(i, v) for i, v in enumerate(ts) if v], [(i, v) for i, v in enumerate(sv) if v]))
    tok, prf, st = b.reveal(c.t)
    rows = [_statement(c, _inputs(b), l, T) for l in range(C * T)]
    sp, sst = c.t.sigma_prove_batch(2, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(c.sc(b.sk[g]) for g in b.signer), fs,
                                    b"".join(b.seeds))
    if prf != sp or st != sst or tok != b"".join(b.tokens):
        fails.append("%s: mp_reveal_batch and mp_msm + mp_sigma_prove_batch differ" % curve)
    checks += 2 * C * T
    c.close()
    return fails, checks


def run_dev(eng, coracle, curve, torch, device):
    """mp_unmask_batch_dev: the inputs of a batch with edge cards and one bad token, copied to buffers of `device` by the test, give the
    outputs of mp_unmask_batch ("cpu" under the emulator, whose device pointers are host pointers)"""
    c = Ctx(eng, coracle, curve)
    fails = []
    C, T = 13, 5
    b = Batch(c, C, T, salt=41)
    toks = list(b.tokens)
    toks[4 * T + 1] = c.pool[0]
    lst = b.card_list(True)
    want = b.unmask(c.t, lst, tokens=toks)
    dev = lambda raw, dt=torch.uint8: torch.frombuffer(bytearray(raw), dtype=dt).to(device)
    keys, cards, tk, pf, pl = dev(b.keys_bytes()), dev(b"".join(b.cards)), dev(b"".join(toks)), dev(b"".join(b.proofs)), dev(b"".join(lst))
    sg = torch.tensor(b.signer, dtype=torch.int32).to(device)      # (indices below 2^31: the same bits as uint32)
    out = torch.full((C * c.pb,), 0xAA, dtype=torch.uint8, device=device)
    idx = torch.full((C,), 7, dtype=torch.int32, device=device)
    ts = torch.full((C * T,), 7, dtype=torch.int32, device=device)
    cs = torch.full((C,), 7, dtype=torch.int32, device=device)
    if device != "cpu":
        torch.cuda.synchronize()
    c.t.unmask_batch_dev(b.K, keys.data_ptr(), C, cards.data_ptr(), T, sg.data_ptr(), tk.data_ptr(), pf.data_ptr(), len(lst), pl.data_ptr(),
                         out.data_ptr(), idx.data_ptr(), ts.data_ptr(), cs.data_ptr())
    eng.sync()
    got = (bytes(out.cpu().numpy().tobytes()), [v & NO_INDEX for v in idx.cpu().tolist()], ts.cpu().tolist(), cs.cpu().tolist())
    if got != want:
        fails.append("%s: mp_unmask_batch_dev differs from mp_unmask_batch (token status %s / %s, card status %s / %s)" %
                     (curve, got[2], want[2], got[3], want[3]))
    if want[3][4] != CHAUM_PEDERSEN or sum(1 for v in want[3] if v) != 1:
        fails.append("%s: card status %s" % (curve, want[3]))
    c.close()
    return fails, 2
