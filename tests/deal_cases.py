"""Cases, references and checks for the two phases before the shuffle: dealing -- mp_mask_batch (masking / remasking with their
Chaum-Pedersen proofs), mp_verify_mask_batch and mp_verify_mask_batch_dev -- and seating -- mp_aggregate_keys_batch (Schnorr proofs of
the players' keys, the tables' aggregate keys) -- on every curve.  Shared by tests/test_deal_emu.py (the kernel bodies under the
development emulator, CPU) and tests/test_gpu_deal.py (the gfx950 build) -- same cases, same expectations: exact equality with the C++
oracle (coracle.sigma_prove, coracle.sigma_verify, coracle.msm) and, for one tiny batch, with the Python oracle's mask / verify_mask /
remask_with_proof / verify_remask / compute_aggregate_key as well.  Nothing here takes an expectation from the engine.

A dealing batch is C cards and K keys; card i is masked under keys[key_index[i]].  A seating batch is `tables` tables of P players; lane
table * P + seat.  Every run_* function takes an engine (_native.Engine), the coracle module and a curve name, and returns (failure
messages, number of checks made); the tests assert that the list is empty."""
import ctypes
import hashlib
import random

import mp_oracle as po
from trait_cases import BAD_ENCODING, CURVES, Ctx, M_, N_, off_subgroup_points  # noqa: F401  (CURVES: for the test files)

MASK, REMASK = 0, 1                                         # MP_DEAL_MASK, MP_DEAL_REMASK (include/mpshuffle.h)
KINDS = (MASK, REMASK)
KIND_NAME = {MASK: "mask", REMASK: "remask"}
FS = {MASK: po.MASKING_RNG_SEED, REMASK: po.REMASKING_RNG_SEED}
SHAPES = [(1, 1), (63, 3), (64, 3), (65, 7), (257, 16)]     # (cards, keys): around a wave and a block
STARK_EXTRA = [(52, 1)]                                     # a deck under one key
SEATS = [(1, 1), (7, 9), (8, 8), (13, 5), (257, 1)]         # (tables, players): 1, 63, 64, 65 and 257 lanes
BAD_ARGUMENT = -3                                           # MP_ERR_BAD_ARGUMENT
SCHNORR, CHAUM_PEDERSEN = 5, 6
BIG = 1048576


def shapes(curve):
    return SHAPES + (STARK_EXTRA if curve == "stark" else [])


# the edge lanes of a dealing batch, by name; "generic" entries in between so that edge lanes have ordinary neighbours
EDGES = ["generic", "factor 0: masked == in", "factor 1", "generic", "factor q - 1", "card O / c0 = O", "c1 = O", "generic",
         "masked.c0 = -in.c0", "masked.c1 = -in.c1", "masked.c0 = O", "masked.c1 = O", "generic"]


class Deal:
    """keys, key indices, input cards, factors and prover seeds; masked cards and proofs as the oracle computes them.  Keys and cards
    are multiples of G with known logarithms (Ctx.pool), so that a factor exists for every edge."""

    def __init__(self, c, kind, C, K, salt=0, edges=True, keys=None):
        self.c, self.kind, self.C, self.K = c, kind, C, K
        q = c.q
        rng = random.Random(7000 * C + 100 * K + 10 * kind + salt + c.cv.cid)
        self.ksk = [rng.randrange(3, q - 1) for _ in range(K)]
        self.keys = [c.mul(k, c.G) for k in self.ksk] if keys is None else list(keys)
        self.key_index = [(5 * i + C) % K for i in range(C)]
        self.inputs, self.factors, self.kinds = [], [], []
        for i in range(C):
            name = EDGES[(i + C) % len(EDGES)] if edges else "generic"
            pk = self.keys[self.key_index[i]]
            k0, k1 = c.pool_k[1 + (i + C) % 15], c.pool_k[1 + (3 * i + K) % 15]
            in0 = c.pool[1 + (i + C) % 15] if kind == REMASK else c.inf          # k0 G
            in1 = c.mul(k1, pk)                                                  # k1 pk
            r = rng.randrange(3, q - 1)
            if name.startswith("factor 0"):
                r = 0
            elif name == "factor 1":
                r = 1
            elif name == "factor q - 1":
                r = q - 1
            elif name == "card O / c0 = O":
                if kind == MASK:
                    in1 = c.inf
                else:
                    in0 = c.inf
            elif name == "c1 = O":
                in1 = c.inf
            elif name == "masked.c0 = -in.c0" and kind == REMASK:
                r = -2 * k0 % q                                                  # the verifier's difference is a doubling
            elif name == "masked.c1 = -in.c1":
                r = -2 * k1 % q
            elif name == "masked.c0 = O" and kind == REMASK:
                r = -k0 % q
            elif name == "masked.c1 = O":
                r = -k1 % q
            elif kind == MASK and name in ("masked.c0 = -in.c0", "masked.c0 = O"):
                name = "generic"                                                 # (in.c0 = O when masking: nothing to cancel)
            self.kinds.append(name)
            self.inputs.append((in0, in1))
            self.factors.append(r)
        self.seeds = [hashlib.blake2s(b"deal seed %d %d %d %d %d" % (kind, C, K, salt, i)).digest() for i in range(C)]
        self.masked, self.proofs = [], []
        for i in range(C):
            pk = self.keys[self.key_index[i]]
            a0, a1 = c.mul(self.factors[i], c.G), c.mul(self.factors[i], pk)
            self.masked.append((c.add(self.inputs[i][0], a0), c.add(self.inputs[i][1], a1)))
            self.proofs.append(c.co.sigma_prove(c.curve, 2, c.G + pk, a0 + a1, c.sc(self.factors[i]), FS[kind], self.seeds[i]))

    def input_bytes(self, inputs=None):
        inputs = self.inputs if inputs is None else inputs
        return b"".join(p[1] if self.kind == MASK else p[0] + p[1] for p in inputs)

    def masked_bytes(self, masked=None):
        return b"".join(m[0] + m[1] for m in (self.masked if masked is None else masked))

    def prove(self, t):
        return t.mask_batch(self.kind, b"".join(self.keys), self.key_index, self.input_bytes(), b"".join(self.c.sc(r) for r in self.factors),
                            b"".join(self.seeds))

    def verify(self, t, keys=None, key_index=None, inputs=None, masked=None, proofs=None):
        return t.verify_mask_batch(self.kind, b"".join(self.keys if keys is None else keys), self.key_index if key_index is None else key_index,
                                   self.input_bytes(inputs), self.masked_bytes(masked), b"".join(self.proofs if proofs is None else proofs))

    def edge_holds(self, i):
        """is lane i the edge its name says, in the oracle's points?"""
        c, name = self.c, self.kinds[i]
        (i0, i1), (m0, m1) = self.inputs[i], self.masked[i]
        return {"factor 0: masked == in": (m0, m1) == (i0, i1), "card O / c0 = O": (i1 if self.kind == MASK else i0) == c.inf,
                "c1 = O": i1 == c.inf, "masked.c0 = -in.c0": m0 == c.neg(i0) and m0 != c.inf, "masked.c1 = -in.c1": m1 == c.neg(i1) and m1 != c.inf,
                "masked.c0 = O": m0 == c.inf and i0 != c.inf, "masked.c1 = O": m1 == c.inf and i1 != c.inf}.get(name, True)


def statement(c, key, inp, masked, proof):
    """the host-assembled statement of one card as mp_sigma_verify_batch and coracle.sigma_verify take it: the publics are the oracle's
    differences masked - in (a coordinate negation and an addition: right for every point of the curve)"""
    return c.G + key, c.add(masked[0], c.neg(inp[0])) + c.add(masked[1], c.neg(inp[1])), proof


def _diff(fails, tag, got, want, kinds=None):
    if got != want:
        bad = [i for i in range(len(want)) if i >= len(got) or got[i] != want[i]]
        fails.append("%s: status %s, expected %s%s" % (tag, [(i, got[i]) for i in bad[:8]], [(i, want[i]) for i in bad[:8]],
                                                       " (%s)" % [kinds[i] for i in bad[:8]] if kinds else ""))


def run_honest(eng, coracle, curve, shape_list=None, kinds=KINDS, edges=True):
    """mp_mask_batch: masked cards and proofs equal the oracle's lane by lane; mp_verify_mask_batch: the oracle accepts every statement,
    and so does the engine"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    cb, psz = 2 * c.pb, 2 * c.pb + 32
    for C, K in (shape_list if shape_list is not None else shapes(curve)):
        for kind in kinds:
            b = Deal(c, kind, C, K, edges=edges)
            tag = "%s %s (%d, %d)" % (curve, KIND_NAME[kind], C, K)
            for i in range(C):
                if not b.edge_holds(i):
                    fails.append("%s card %d: the case '%s' is not what it says in the oracle" % (tag, i, b.kinds[i]))
                g, a, pf = statement(c, b.keys[b.key_index[i]], b.inputs[i], b.masked[i], b.proofs[i])
                if coracle.sigma_verify(curve, 2, g, a, pf, FS[kind]) != 0:
                    fails.append("%s card %d (%s): the oracle refuses its own proof" % (tag, i, b.kinds[i]))
            out, prf, st = b.prove(c.t)
            _diff(fails, tag + " prove", st, [0] * C, b.kinds)
            for i in range(C):
                if out[i * cb:(i + 1) * cb] != b.masked[i][0] + b.masked[i][1]:
                    fails.append("%s card %d (%s): masked card differs from the oracle's" % (tag, i, b.kinds[i]))
                if prf[i * psz:(i + 1) * psz] != b.proofs[i]:
                    fails.append("%s card %d (%s): proof differs from the oracle's" % (tag, i, b.kinds[i]))
            _diff(fails, tag + " verify", b.verify(c.t), [0] * C, b.kinds)
            checks += 4 * C
    c.close()
    return fails, checks


def _pp(c):
    pts = [po.pt_from_wire(c.params[i * c.pb:(i + 1) * c.pb]) for i in range(N_ + 3)]
    return po.Params(c.cv, M_, N_, pts[0], pts[1:1 + N_], pts[1 + N_], pts[2 + N_])


def run_python_oracle(eng, coracle, curve):
    """the third restatement on one tiny batch: po.mask / verify_mask / remask_with_proof / verify_remask, po.compute_aggregate_key"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    cb, psz = 2 * c.pb, 2 * c.pb + 32
    with po.curve_ctx(c.cv):
        pp = _pp(c)
        W = po.pt_from_wire
        for kind in KINDS:
            b = Deal(c, kind, 3, 2, salt=5, edges=False)
            out, prf, st = b.prove(c.t)
            vs = b.verify(c.t)
            for i in range(3):
                pk, r = W(b.keys[b.key_index[i]]), b.factors[i]
                if kind == MASK:
                    masked, proof = po.mask(pp, pk, W(b.inputs[i][1]), r, b.seeds[i])
                    ok = po.verify_mask(pp, pk, W(b.inputs[i][1]), masked, proof)
                else:
                    orig = (W(b.inputs[i][0]), W(b.inputs[i][1]))
                    masked, proof = po.remask_with_proof(pp, pk, orig, r, b.seeds[i])
                    ok = po.verify_remask(pp, pk, orig, masked, proof)
                if po.pt_wire(masked[0]) + po.pt_wire(masked[1]) != out[i * cb:(i + 1) * cb] or po.sigma_proof_bytes(proof) != prf[i * psz:(i + 1) * psz]:
                    fails.append("%s %s card %d: masked card or proof differs from the Python oracle's" % (curve, KIND_NAME[kind], i))
                if not ok:
                    fails.append("%s %s card %d: the Python oracle refuses its own proof" % (curve, KIND_NAME[kind], i))
            if st != [0] * 3 or vs != [0] * 3:
                fails.append("%s %s: status %s %s" % (curve, KIND_NAME[kind], st, vs))
            checks += 7
        s = Seating(c, 2, 3, salt=5, edges=False)
        keys, ps, ts = s.run(c.t)
        for k in range(2):
            rows = [(W(s.pk[l]), po.sigma_proof_from_bytes(s.proofs[l], 1), s.infos[l]) for l in range(3 * k, 3 * k + 3)]
            if po.pt_wire(po.compute_aggregate_key(pp, rows)) != keys[k * c.pb:(k + 1) * c.pb]:
                fails.append("%s table %d: aggregate key differs from the Python oracle's" % (curve, k))
        if ps != [0] * 6 or ts != [0] * 2:
            fails.append("%s seating: status %s %s" % (curve, ps, ts))
        checks += 3
    c.close()
    return fails, checks


def _noncanonical(c, P):
    """x replaced by p: a coordinate that is not reduced"""
    return c.p.to_bytes(c.fb, "little") + P[c.fb:]


def defect_list(c, b):
    """(name, expected status or None = what the oracle says (it must refuse), edit, lanes it takes) -- edit(d, l) changes the
    dictionary of the batch's inputs at lane l"""
    pb, q, K = c.pb, c.q, b.K
    spare = c.pool[0]
    z_of = lambda p: int.from_bytes(p[2 * pb:], "little")      # noqa: E731

    def proof_part(name, f, want):
        def edit(d, l):
            d["proofs"][l] = f(d["proofs"][l])
        return (name, want, edit, 1)

    def point(name, what, half, f, want=BAD_ENCODING):
        def edit(d, l):
            v = list(d[what][l])
            v[half] = f(v[half])
            d[what][l] = tuple(v)
        return (name, want, edit, 1)

    def index(name, f, want):
        def edit(d, l):
            d["key_index"][l] = f(d["key_index"][l])
        return (name, want, edit, 1)

    def bad_key(name, f):
        def edit(d, l):
            d["keys"].append(f(d["keys"][d["key_index"][l]]))      # a key of its own, named by this lane alone
            d["key_index"][l] = len(d["keys"]) - 1
        return (name, BAD_ENCODING, edit, 1)

    def swap(d, l):
        d["inputs"][l], d["inputs"][l + 1] = d["inputs"][l + 1], d["inputs"][l]

    def past_and_bad(d, l):
        d["key_index"][l] = -1
        d["proofs"][l] = d["proofs"][l][:2 * pb] + c.sc(q)

    return [
        proof_part("z + 1", lambda p: p[:2 * pb] + c.sc((z_of(p) + 1) % q), None),
        proof_part("A_0 replaced", lambda p: spare + p[pb:], None),
        proof_part("A_1 replaced", lambda p: p[:pb] + spare + p[2 * pb:], None),
        point("masked c1 moved by G", "masked", 1, lambda P: c.add(P, c.G), None),
        ("input card swapped with its neighbour's", None, swap, 2),
        index("the right proof under the wrong key index", lambda k: (k + 1) % K, None),
        index("key_index = K", lambda k: -1, BAD_ARGUMENT),      # (run_defects puts K there once the key list is complete)
        index("key_index = 0xFFFFFFFF", lambda k: 0xFFFFFFFF, BAD_ARGUMENT),
        ("key_index = K and a response >= q", BAD_ARGUMENT, past_and_bad, 1),
        point("input c1 with a coordinate >= p", "inputs", 1, lambda P: _noncanonical(c, P)),
        point("masked c0 with a coordinate >= p", "masked", 0, lambda P: _noncanonical(c, P)),
        point("input c1 off the curve", "inputs", 1, c.off_curve),
        point("masked c0 off the curve", "masked", 0, c.off_curve),
        point("masked c1 off the curve", "masked", 1, c.off_curve),
        proof_part("A_1 off the curve", lambda p: p[:pb] + c.off_curve(p[pb:2 * pb]) + p[2 * pb:], BAD_ENCODING),
        proof_part("A_0 with a coordinate >= p", lambda p: _noncanonical(c, p[:pb]) + p[pb:], BAD_ENCODING),
        proof_part("z = q", lambda p: p[:2 * pb] + c.sc(q), BAD_ENCODING),
        bad_key("key off the curve", c.off_curve),
        bad_key("key with a coordinate >= p", lambda P: _noncanonical(c, P)),
    ]


def _inputs(b):
    return dict(keys=list(b.keys), key_index=list(b.key_index), inputs=list(b.inputs), masked=list(b.masked), proofs=list(b.proofs))


def _oracle_words(c, b, d, want):
    """fills the entries of `want` that are None with the oracle's verdict on the host-assembled statement"""
    for l in range(b.C):
        if want[l] is None:
            want[l] = c.co.sigma_verify(c.curve, 2, *statement(c, d["keys"][d["key_index"][l]], d["inputs"][l], d["masked"][l], d["proofs"][l]), FS[b.kind])
    return want


def run_defects(eng, coracle, curve):
    """one defect per lane (the swap: two) in a batch of generic cards, every third lane honest; then the prover's refused lanes and the
    call-level refusals"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    cb, psz = 2 * c.pb, 2 * c.pb + 32
    for kind in KINDS:
        probe = Deal(c, kind, 1, 3, edges=False)
        C = 3 * len(defect_list(c, probe)) + 2
        b = Deal(c, kind, C, 3, salt=11, edges=False)
        d = _inputs(b)
        want, names = [None] * C, ["honest"] * C
        for k, (name, code, edit, lanes) in enumerate(defect_list(c, b)):
            l = 3 * k + 1                                  # lanes 3 k stay honest
            edit(d, l)
            for j in range(lanes):
                want[l + j], names[l + j] = code, name
        d["key_index"] = [len(d["keys"]) if k == -1 else k for k in d["key_index"]]
        _oracle_words(c, b, d, want)
        tag = "%s %s defects" % (curve, KIND_NAME[kind])
        # the oracle alone: every defect it judges is refused, every honest lane accepted
        for l in range(C):
            if (names[l] == "honest") != (want[l] == 0):
                fails.append("%s lane %d (%s): the oracle says %d" % (tag, l, names[l], want[l]))
        if not (any(v == 0 for v in want) and any(v == CHAUM_PEDERSEN for v in want) and any(v == BAD_ENCODING for v in want)):
            fails.append("%s: the oracle's verdicts are %s" % (tag, want))
        got = b.verify(c.t, keys=d["keys"], key_index=d["key_index"], inputs=d["inputs"], masked=d["masked"], proofs=d["proofs"])
        _diff(fails, tag, got, want, names)
        checks += C
        # ---- the prover: a factor >= q, a key and an input point off the curve and a key index past the keys, between honest lanes
        hb = Deal(c, kind, 8, 3, salt=9, edges=False)
        keys, ki, inputs, factors = list(hb.keys) + [c.off_curve(hb.keys[0])], list(hb.key_index), list(hb.inputs), [c.sc(r) for r in hb.factors]
        factors[1] = c.sc(c.q)
        ki[3] = 3
        inputs[5] = (inputs[5][0], c.off_curve(inputs[5][1]))
        ki[6] = 4
        out, prf, st = c.t.mask_batch(kind, b"".join(keys), ki, hb.input_bytes(inputs), b"".join(factors), b"".join(hb.seeds))
        wst = [0, BAD_ENCODING, 0, BAD_ENCODING, 0, BAD_ENCODING, BAD_ARGUMENT, 0]
        _diff(fails, "%s %s prover with refused lanes" % (curve, KIND_NAME[kind]), st, wst)
        for l in range(8):
            wo, wp = (hb.masked_bytes([hb.masked[l]]), hb.proofs[l]) if wst[l] == 0 else (bytes(cb), bytes(psz))
            if out[l * cb:(l + 1) * cb] != wo or prf[l * psz:(l + 1) * psz] != wp:
                fails.append("%s %s prover lane %d (status %d): output differs from %s" % (curve, KIND_NAME[kind], l, wst[l],
                                                                                          "the oracle's" if wst[l] == 0 else "zero bytes"))
        checks += 16
    # ---- call level: refused before any launch
    lib, h = c.t.lib, c.t.h
    buf = (ctypes.c_uint8 * 4096)()
    for name, (kind, K, C) in (("C = 0", (MASK, 1, 0)), ("K = 0", (REMASK, 0, 1)), ("an unknown kind", (2, 1, 1)), ("kind = -1", (-1, 1, 1)),
                               ("C over the limit", (MASK, 1, BIG + 1)), ("K over the limit", (REMASK, BIG + 1, 1))):
        for fn, rc in (("mask", lib.mp_mask_batch(h, kind, K, buf, C, buf, buf, buf, buf, buf, buf, buf)),
                       ("verify_mask", lib.mp_verify_mask_batch(h, kind, K, buf, C, buf, buf, buf, buf, buf)),
                       ("verify_mask_dev", lib.mp_verify_mask_batch_dev(h, kind, K, buf, C, buf, buf, buf, buf, buf))):
            if rc != BAD_ARGUMENT:
                fails.append("%s mp_%s_batch, %s: %d, expected %d" % (curve, fn, name, rc, BAD_ARGUMENT))
            checks += 1
    for name, (tables, P) in (("P = 0", (1, 0)), ("tables = 0", (0, 1)), ("tables * P over the limit", (BIG // 4 + 1, 4)),
                              ("tables over the limit", (BIG + 1, 1)), ("P over the limit", (3, BIG // 2))):
        rc = lib.mp_aggregate_keys_batch(h, tables, P, buf, buf, buf, buf, buf, buf)
        if rc != BAD_ARGUMENT:
            fails.append("%s mp_aggregate_keys_batch, %s: %d, expected %d" % (curve, name, rc, BAD_ARGUMENT))
        checks += 1
    for pos in range(8):      # a null pointer in every place
        a = [buf] * 8
        a[pos] = None
        rcs = [lib.mp_verify_mask_batch(h, MASK, 1, a[0], 1, a[1], a[2], a[3], a[4], a[5]) if pos < 6 else BAD_ARGUMENT,
               lib.mp_verify_mask_batch_dev(h, MASK, 1, a[0], 1, a[1], a[2], a[3], a[4], a[5]) if pos < 6 else BAD_ARGUMENT,
               lib.mp_mask_batch(h, MASK, 1, a[0], 1, a[1], a[2], a[3], a[4], a[5], a[6], a[7]),
               lib.mp_aggregate_keys_batch(h, 1, 1, a[0], a[1], a[2], a[3], a[4], a[5]) if pos < 6 else BAD_ARGUMENT]
        if rcs != [BAD_ARGUMENT] * 4:
            fails.append("%s: a null pointer as argument %d gives %s" % (curve, pos, rcs))
        checks += 4
    c.close()
    return fails, checks


def run_subgroup(eng, coracle, curve="bls12_377"):
    """BLS12-377: each kind of point outside the subgroup as key, as input point, as masked point and as commitment, every other lane:
    refused as a bad encoding, and only there; with the table's subgroup test off, the oracle's verdict"""
    assert curve == "bls12_377"
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    pts = list(zip(("low-order point", "point before cofactor clearing", "subgroup point + low-order point"), off_subgroup_points()))
    places = ("key", "input c1", "masked c0", "masked c1", "A_0")
    for kind in KINDS:
        C = 2 * len(pts) * len(places) + 1
        b = Deal(c, kind, C, 3, salt=21, edges=False)
        d = _inputs(b)
        on, names = [0] * C, ["honest"] * C
        k = 0
        for kname, pt in pts:
            for place in places:
                l = 2 * k + 1
                if place == "key":
                    d["keys"].append(pt)
                    d["key_index"][l] = len(d["keys"]) - 1
                elif place == "input c1":
                    d["inputs"][l] = (d["inputs"][l][0], pt)
                elif place == "masked c0":
                    d["masked"][l] = (pt, d["masked"][l][1])
                elif place == "masked c1":
                    d["masked"][l] = (d["masked"][l][0], pt)
                else:
                    d["proofs"][l] = pt + d["proofs"][l][c.pb:]
                on[l], names[l] = BAD_ENCODING, "%s as %s" % (kname, place)
                k += 1
        args = dict(keys=d["keys"], key_index=d["key_index"], inputs=d["inputs"], masked=d["masked"], proofs=d["proofs"])
        tag = "bls12_377 %s subgroup" % KIND_NAME[kind]
        _diff(fails, tag, b.verify(c.t, **args), on, names)
        off = _oracle_words(c, b, d, [None] * C)
        if not all(v in (0, CHAUM_PEDERSEN) for v in off) or not any(v == 0 for v in off) or not any(v == CHAUM_PEDERSEN for v in off):
            fails.append("%s test off: the oracle's verdicts are %s" % (tag, off))
        c.t.set_subgroup_check(False)
        try:
            got = b.verify(c.t, **args)
        finally:
            c.t.set_subgroup_check(True)
        _diff(fails, tag + " test off", got, off, names)
        checks += 2 * C
    # seating: a key and a commitment outside the subgroup
    s = Seating(c, 4, 3, salt=21, edges=False)
    keys, proofs = list(s.pk), list(s.proofs)
    keys[4] = pts[0][1]
    proofs[10] = pts[2][1] + proofs[10][c.pb:]
    _, ps, ts = s.run(c.t, keys=keys, proofs=proofs)
    want = [0] * 12
    want[4] = want[10] = BAD_ENCODING
    _diff(fails, "bls12_377 seating subgroup", ps, want)
    _diff(fails, "bls12_377 seating subgroup, tables", ts, [0, BAD_ENCODING, 0, BAD_ENCODING])
    c.close()
    return fails, checks + 16


def run_agreement(eng, coracle, curve):
    """one (65, 1) batch of each kind under the table's own key, with two defects: masked cards, proofs and status words equal those of the
    composed calls on the same inputs -- mp_msm / mp_remask_batch for the cards, mp_msm(k = 2) for the statements, mp_sigma_prove_batch and
    mp_sigma_verify_batch -- and seating equals mp_sigma_verify_batch(nbases = 1) + mp_msm"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    C, q = 65, c.q
    one, minus = c.sc(1), c.sc(q - 1)
    for kind in KINDS:
        b = Deal(c, kind, C, 1, salt=31, keys=[c.pk])
        tag = "%s %s" % (curve, KIND_NAME[kind])
        rb = b"".join(c.sc(r) for r in b.factors)
        if kind == MASK:
            c0 = c.t.msm(C, 1, rb, c.G * C)
            c1 = c.t.msm(C, 2, b"".join(one + c.sc(r) for r in b.factors), b"".join(p[1] + c.pk for p in b.inputs))
            cards = b"".join(c0[i * c.pb:(i + 1) * c.pb] + c1[i * c.pb:(i + 1) * c.pb] for i in range(C))
        else:
            cards = c.t.remask_batch(b.input_bytes(), rb)
        halves = lambda raw, i: (raw[2 * c.pb * i:2 * c.pb * i + c.pb], raw[2 * c.pb * i + c.pb:2 * c.pb * (i + 1)])      # noqa: E731

        def publics(masked_of):
            pts = b"".join(masked_of(i)[h] + b.inputs[i][h] for i in range(C) for h in (0, 1))
            return c.t.msm(2 * C, 2, (one + minus) * (2 * C), pts)
        fs = eng.blake2s(FS[kind]) * C
        pf, pst = c.t.sigma_prove_batch(2, (c.G + c.pk) * C, publics(lambda i: halves(cards, i)), rb, fs, b"".join(b.seeds))
        out, prf, st = b.prove(c.t)
        if out != cards or prf != pf or st != pst or st != [0] * C:
            fails.append("%s: mp_mask_batch and its composed form differ" % tag)
        d = _inputs(b)
        d["masked"][7] = (d["masked"][7][0], c.add(d["masked"][7][1], c.G))
        d["proofs"][40] = d["proofs"][40][:2 * c.pb] + c.sc(q)
        sv = c.t.sigma_verify_batch(2, (c.G + c.pk) * C, publics(lambda i: d["masked"][i]), b"".join(d["proofs"]), fs)
        got = b.verify(c.t, masked=d["masked"], proofs=d["proofs"])
        if got != sv or sv[7] != CHAUM_PEDERSEN or sv[40] != BAD_ENCODING or sum(1 for v in sv if v) != 2:
            fails.append("%s: status %s, mp_sigma_verify_batch %s" % (tag, [(i, v) for i, v in enumerate(got) if v], [(i, v) for i, v in enumerate(sv) if v]))
        checks += 2 * C
    s = Seating(c, 13, 5, salt=31)
    proofs = list(s.proofs)
    proofs[22] = proofs[22][:c.pb] + c.sc((int.from_bytes(proofs[22][c.pb:], "little") + 1) % q)
    keys, ps, ts = s.run(c.t, proofs=proofs)
    sv = c.t.sigma_verify_batch(1, c.G * 65, b"".join(s.pk), b"".join(proofs), b"".join(c.fs_digest(s.fs_raw(l)) for l in range(65)))
    sums = c.t.msm(13, 5, one * 65, b"".join(s.pk))
    want_keys = b"".join(c.inf if k == 4 else sums[k * c.pb:(k + 1) * c.pb] for k in range(13))
    if ps != sv or sv[22] != SCHNORR or sum(1 for v in sv if v) != 1 or keys != want_keys or ts != [SCHNORR if k == 4 else 0 for k in range(13)]:
        fails.append("%s: mp_aggregate_keys_batch and mp_sigma_verify_batch + mp_msm differ (%s / %s, tables %s)" % (curve, ps, sv, ts))
    c.close()
    return fails, checks + 65


def run_dev(eng, coracle, curve, torch, device):
    """mp_verify_mask_batch_dev gives the words of mp_verify_mask_batch.  "cpu" (the emulator, whose device pointers are host pointers): the
    inputs of a batch with edge cards and two defects, copied to tensors by the test.  A GPU: the input cards are the d_out_decks of a
    shuffle prover, used where they lie; they are remasked on the host side and verified through the device pointers."""
    c = Ctx(eng, coracle, curve)
    fails = []
    dev = lambda raw, dt=torch.uint8: torch.frombuffer(bytearray(raw), dtype=dt).to(device)      # noqa: E731
    kind = REMASK
    if device == "cpu":
        b = Deal(c, kind, 65, 7, salt=41)
        d_in = dev(b.input_bytes())
    else:
        N = M_ * N_
        od = torch.empty(len(c.gi["deck"]), dtype=torch.uint8, device=device)
        op = torch.empty(c.t.proof_bytes, dtype=torch.uint8, device=device)
        sp = torch.full((1,), 7, dtype=torch.int32, device=device)
        ins = [dev(c.gi["deck"]), dev(c.gi["rho"]), torch.tensor(list(c.gi["perm"]), dtype=torch.int32).to(device), dev(c.gi["prover_seed"])]
        torch.cuda.synchronize()
        c.t.shuffle_and_remask_batch_dev(1, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), od.data_ptr(), op.data_ptr(),
                                         sp.data_ptr())
        eng.sync()
        raw = bytes(od.cpu().numpy().tobytes())
        if sp.cpu().tolist() != [0] or raw != coracle.shuffle_and_remask(curve, M_, N_, **c.gi)[0]:
            fails.append("%s: the shuffle prover's deck is not the oracle's" % curve)
        b = Deal(c, kind, N, 3, salt=41, edges=False)
        b.inputs = [(raw[2 * c.pb * i:2 * c.pb * i + c.pb], raw[2 * c.pb * i + c.pb:2 * c.pb * (i + 1)]) for i in range(N)]
        b.masked, b.proofs = [], []
        for i in range(N):
            pk, r = b.keys[b.key_index[i]], b.factors[i]
            a0, a1 = c.mul(r, c.G), c.mul(r, pk)
            b.masked.append((c.add(b.inputs[i][0], a0), c.add(b.inputs[i][1], a1)))
            b.proofs.append(coracle.sigma_prove(curve, 2, c.G + pk, a0 + a1, c.sc(r), FS[kind], b.seeds[i]))
        d_in = od
    C = b.C
    masked, proofs = list(b.masked), list(b.proofs)
    masked[C // 2] = (masked[C // 2][0], c.add(masked[C // 2][1], c.G))
    ki = list(b.key_index)
    ki[C - 2] = b.K
    want = _oracle_words(c, b, dict(keys=b.keys, key_index=b.key_index, inputs=b.inputs, masked=masked, proofs=proofs), [None] * C)
    want[C - 2] = BAD_ARGUMENT
    if want[C // 2] != CHAUM_PEDERSEN or sum(1 for v in want if v) != 2:
        fails.append("%s: the oracle's verdicts are %s" % (curve, want))
    host = b.verify(c.t, key_index=ki, masked=masked, proofs=proofs)
    keys, d_m, d_p = dev(b"".join(b.keys)), dev(b.masked_bytes(masked)), dev(b"".join(proofs))
    d_ki = torch.tensor(ki, dtype=torch.int32).to(device)      # (indices below 2^31: the same bits as uint32)
    st = torch.full((C,), 7, dtype=torch.int32, device=device)
    if device != "cpu":
        torch.cuda.synchronize()
    c.t.verify_mask_batch_dev(kind, b.K, keys.data_ptr(), C, d_ki.data_ptr(), d_in.data_ptr(), d_m.data_ptr(), d_p.data_ptr(), st.data_ptr())
    eng.sync()
    got = st.cpu().tolist()
    if got != want or host != want:
        fails.append("%s: mp_verify_mask_batch_dev %s, mp_verify_mask_batch %s, the oracle %s" % (curve, got, host, want))
    c.close()
    return fails, 2 * C


# ---------------------------------------------------------------------------------------------------------------- seating
class Seating:
    """keys, Schnorr proofs and public information of tables x P players; the aggregate keys as the oracle sums them"""

    def __init__(self, c, tables, P, salt=0, edges=True):
        self.c, self.tables, self.P = c, tables, P
        q = c.q
        rng = random.Random(9000 * tables + 10 * P + salt + c.cv.cid)
        self.sk, self.kinds = [], []
        for k in range(tables):
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
                kind = "one key twice"                       # next to each other when P = 2: the sum is a doubling
                sks[P - 1] = sks[0]
                if P >= 3:
                    sks[1:P - 1] = [0] * (P - 3) + [sks[0]]  # 0 + sk + sk (+ sk): the doubling, whatever the order of the additions
            elif e == 4 and P >= 2:
                kind = "sk and q - sk: the aggregate is O"
                sks = [sks[0], q - sks[0]] + [0] * (P - 2)
            self.sk += sks
            self.kinds.append(kind)
        B = tables * P
        self.pk = [c.mul(x, c.G) for x in self.sk]
        self.infos = [b"player %d" % l + b"!" * (l % 5) for l in range(B)]
        self.seeds = [hashlib.blake2s(b"seat seed %d %d %d %d" % (tables, P, salt, l)).digest() for l in range(B)]
        self.proofs = [c.co.sigma_prove(c.curve, 1, c.G, self.pk[l], c.sc(self.sk[l]), self.fs_raw(l), self.seeds[l]) for l in range(B)]
        self.agg = [c.co.msm(c.curve, c.sc(1) * P, b"".join(self.pk[k * P:(k + 1) * P])) for k in range(tables)]

    def fs_raw(self, l, infos=None):
        return po.KEY_OWN_RNG_SEED + (self.infos if infos is None else infos)[l]

    def run(self, t, keys=None, proofs=None, infos=None):
        B = self.tables * self.P
        return t.aggregate_keys_batch(self.tables, self.P, b"".join(self.pk if keys is None else keys), b"".join(self.proofs if proofs is None else proofs),
                                      b"".join(self.c.fs_digest(self.fs_raw(l, infos)) for l in range(B)))


def _check_seating(fails, tag, s, got, want_ps):
    c, P = s.c, s.P
    keys, ps, ts = got
    _diff(fails, tag + " players", ps, want_ps)
    for k in range(s.tables):
        first = next((v for v in want_ps[k * P:(k + 1) * P] if v != 0), 0)
        if ts[k] != first:
            fails.append("%s table %d (%s): status %d, expected %d" % (tag, k, s.kinds[k], ts[k], first))
        if keys[k * c.pb:(k + 1) * c.pb] != (s.agg[k] if first == 0 else c.inf):
            fails.append("%s table %d (%s): aggregate key differs from %s" % (tag, k, s.kinds[k], "the oracle's" if first == 0 else "zero bytes"))
    return len(want_ps) + 2 * s.tables


def run_seating(eng, coracle, curve, seat_list=None):
    """every shape with its edge tables: all proofs verify in the oracle and in the engine, the aggregate keys are the oracle's sums.  Then
    defects in a (7, 9) batch: a proof for another fs_init, a wrong response in the middle of a table, a key off the curve, a response
    >= q -- the table has the word of its first bad seat and zero bytes for a key, the other tables are untouched"""
    c = Ctx(eng, coracle, curve)
    fails, checks = [], 0
    for tables, P in (seat_list if seat_list is not None else SEATS):
        s = Seating(c, tables, P)
        tag = "%s seating (%d, %d)" % (curve, tables, P)
        for l in range(tables * P):
            if coracle.sigma_verify(curve, 1, c.G, s.pk[l], s.proofs[l], s.fs_raw(l)) != 0:
                fails.append("%s lane %d: the oracle refuses its own proof" % (tag, l))
        for k in range(tables):
            if s.kinds[k].startswith("sk and q - sk") and s.agg[k] != c.inf:
                fails.append("%s table %d: the case '%s' is not what it says in the oracle" % (tag, k, s.kinds[k]))
        checks += _check_seating(fails, tag, s, s.run(c.t), [0] * (tables * P))
    if seat_list is None or (7, 9) in seat_list:
        s = Seating(c, 7, 9, salt=3, edges=False)
        keys, proofs, infos = list(s.pk), list(s.proofs), list(s.infos)
        z1 = lambda p: p[:c.pb] + c.sc((int.from_bytes(p[c.pb:], "little") + 1) % c.q)      # noqa: E731
        infos[1 * 9 + 0] = b"somebody else"                  # table 1, first seat: a proof for another fs_init
        proofs[3 * 9 + 4] = z1(proofs[3 * 9 + 4])            # table 3: a bad seat in the middle ...
        proofs[3 * 9 + 7] = proofs[3 * 9 + 7][:c.pb] + c.sc(c.q)      # ... and a later one with another word: the first counts
        keys[5 * 9 + 8] = c.off_curve(keys[5 * 9 + 8])       # table 5, last seat
        want = []
        for l in range(63):
            if l == 3 * 9 + 7 or l == 5 * 9 + 8:
                want.append(BAD_ENCODING)
            else:
                want.append(coracle.sigma_verify(curve, 1, c.G, keys[l], proofs[l], s.fs_raw(l, infos)))
        if [l for l in range(63) if want[l] == SCHNORR] != [9, 31] or sum(1 for v in want if v == 0) != 59:
            fails.append("%s seating defects: the oracle's verdicts are %s" % (curve, want))
        got = s.run(c.t, keys=keys, proofs=proofs, infos=infos)
        checks += _check_seating(fails, "%s seating defects" % curve, s, got, want)
        if got[2] != [0, SCHNORR, 0, SCHNORR, 0, BAD_ENCODING, 0]:
            fails.append("%s seating defects: table status %s" % (curve, got[2]))
    c.close()
    return fails, checks


def run_threads(eng, coracle, curve, threading):
    """two host threads on ONE table, each verifying a batch of its own four times: the context's lock runs the calls one after the other,
    and every result equals the single-threaded one"""
    c = Ctx(eng, coracle, curve)
    fails = []
    batches = [Deal(c, MASK, 65, 7, salt=51), Deal(c, REMASK, 64, 3, salt=52)]
    bad = []
    for b in batches:
        m = list(b.masked)
        m[b.C // 2] = (m[b.C // 2][0], c.add(m[b.C // 2][1], c.G))      # one bad card each
        bad.append(m)
    want = [_oracle_words(c, b, dict(keys=b.keys, key_index=b.key_index, inputs=b.inputs, masked=m, proofs=b.proofs), [None] * b.C)
            for b, m in zip(batches, bad)]
    if [sum(1 for v in w if v) for w in want] != [1, 1]:
        fails.append("%s: the oracle's verdicts are %s" % (curve, want))
    single = [b.verify(c.t, masked=m) for b, m in zip(batches, bad)]
    got, errors = [[], []], []

    def work(k):
        try:
            for _ in range(4):
                got[k].append(batches[k].verify(c.t, masked=bad[k]))
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        fails.append("%s: %r" % (curve, errors))
    for k in range(2):
        if single[k] != want[k] or got[k] != [want[k]] * 4:
            fails.append("%s thread %d: %s, single-threaded %s, the oracle %s" % (curve, k, got[k], single[k], want[k]))
    c.close()
    return fails, 10
