"""Cases and checks for DEGENERATE PARAMETER SETS: commitment keys that coincide or cancel (ck_0 = ck_1; ck_1 = -ck_0, where the sum of the
keys -- a fixed base of its own -- is the point at infinity at n = 2 and ck_2 at n = 3), keys equal to H or to G, an aggregate key equal
to ck_0 or to H.  mp_table::init accepts all of them and builds a whole fixed-base table from the point at infinity for the cancelled
sum (k_fb_windows, k_fb_fill, k_fb_widen, k_normalize).  Shared by tests/test_param_edge_emu.py (the kernel bodies under the development
emulator, CPU) and tests/test_gpu_param_edge.py (the gfx950 build) -- same cases, same expectations: exact equality with the C++ oracle,
which run_oracles_agree holds to the Python oracle on every set first.

Every run_* function returns (failure messages, number of checks made); the tests assert that the list is empty."""
import mp_oracle as po
from shuffle_edge_cases import PLAN_PARAMS, _pmap

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
SHAPES = ((2, 2), (2, 3))
SETS = ["ck0_is_ck1", "ck1_is_minus_ck0", "ck0_is_H", "ck1_is_G", "pk_is_ck0", "pk_is_H"]
INF_BASES = ["ck_0", "H", "G", "pk"]          # a base at infinity other than the key sum: MP_ERR_BAD_ENCODING
BAD_ENCODING = -1                             # MP_ERR_BAD_ENCODING (include/mpshuffle.h)
B = 3                                         # proofs per set


def _neg(cv, pb, P):
    y = int.from_bytes(P[pb // 2:], "little")
    return P[:pb // 2] + ((cv.p - y) % cv.p).to_bytes(pb // 2, "little")


def make_set(coracle, curve, m, n, name):
    """-> dict(params, pk, lanes): the oracle's generic parameters with the points of set `name` replaced, and B generic witnesses"""
    cv = po.CURVES[curve]
    pb = coracle.point_size(curve)
    g = [coracle.gen_inputs(curve, m, n, 5200 + 10 * n + b) for b in range(B)]
    pts = [g[0]["params"][pb * i:pb * (i + 1)] for i in range(n + 3)]      # G, ck_0 .. ck_(n-1), H, the generator
    pk = g[0]["pk"]
    G, H = pts[0], pts[1 + n]
    if name == "ck0_is_ck1":
        pts[2] = pts[1]
    elif name == "ck1_is_minus_ck0":
        pts[2] = _neg(cv, pb, pts[1])
    elif name == "ck0_is_H":
        pts[1] = H
    elif name == "ck1_is_G":
        pts[2] = G
    elif name == "pk_is_ck0":
        pk = pts[1]
    elif name == "pk_is_H":
        pk = H
    elif name in INF_BASES:
        if name == "pk":
            pk = bytes(pb)
        else:
            pts[{"ck_0": 1, "H": 1 + n, "G": 0}[name]] = bytes(pb)
    else:
        raise KeyError(name)
    lanes = [dict(deck=x["deck"], rho=x["rho"], perm=list(x["perm"]), seed=x["prover_seed"]) for x in g]
    return dict(curve=curve, m=m, n=n, name=name, params=b"".join(pts), pk=pk, lanes=lanes, pb=pb)


_CACHE = {}


def cases(coracle, curve, m, n, name):
    """the set with the C++ oracle's shuffled decks and proofs, made once and shared by the tests (nothing changes them)"""
    key = (curve, m, n, name)
    if key not in _CACHE:
        s = make_set(coracle, curve, m, n, name)
        outs = _pmap(lambda ln: coracle.shuffle_and_remask(curve, m, n, s["params"], s["pk"], ln["deck"], ln["rho"], ln["perm"], ln["seed"]), s["lanes"])
        for ln, (d, p) in zip(s["lanes"], outs):
            ln["shuffled"], ln["proof"] = d, p
        _CACHE[key] = s
    return _CACHE[key]


def _tamper(s, b, proof):
    """one response scalar + 1: of the zero argument, of the single-value-product argument, of the multi-exponentiation argument in turn"""
    cv = po.CURVES[s["curve"]]
    with po.curve_ctx(cv):
        p = po.proof_from_bytes(proof, s["m"], s["n"])
        d, key = ((p["product"]["had"]["zero"], "tbar"), (p["product"]["svp"], "rt"), (p["mexp"], "taubar"))[b % 3]
        d[key] = (d[key] + 1) % cv.q
        return po.proof_to_bytes(p)


def run_oracles_agree(coracle, curve, m, n, name):
    """the Python oracle and the C++ oracle make the same shuffled deck and proof under the set and give the same verdicts on them, honest
    and with a response scalar changed (CPU only)"""
    s = cases(coracle, curve, m, n, name)
    cv = po.CURVES[curve]
    fails, checks = [], 0
    with po.curve_ctx(cv):
        w = po.point_bytes()
        pts = [po.pt_from_wire(s["params"][i:i + w]) for i in range(0, len(s["params"]), w)]
        pp = po.Params(cv, m, n, pts[0], pts[1:1 + n], pts[1 + n], pts[2 + n])
        pk = po.pt_from_wire(s["pk"])
        if (po.pp_gsum(pp) is None) != (name == "ck1_is_minus_ck0" and n == 2):
            fails.append("%s (%d, %d) %s: the sum of the commitment keys is %s" % (curve, m, n, name, po.pp_gsum(pp)))
        for b, ln in enumerate(s["lanes"]):
            deck = po.deck_from_bytes(ln["deck"])
            rho = [int.from_bytes(ln["rho"][32 * i:32 * i + 32], "little") for i in range(m * n)]
            sh, pf = po.shuffle_and_remask(pp, pk, deck, rho, ln["perm"], ln["seed"])
            if po.deck_to_bytes(sh) != ln["shuffled"] or po.proof_to_bytes(pf) != ln["proof"]:
                fails.append("%s (%d, %d) %s lane %d: the oracles' outputs differ" % (curve, m, n, name, b))
            bad = _tamper(s, b, ln["proof"])
            for what, proof, py_pf in (("honest", ln["proof"], pf), ("tampered", bad, po.proof_from_bytes(bad, m, n))):
                v_py = po.verify_shuffle(pp, pk, deck, sh, py_pf)
                v_c = coracle.verify_shuffle(curve, m, n, s["params"], s["pk"], ln["deck"], ln["shuffled"], proof)
                if v_py != v_c or (v_c == 0) != (what == "honest"):
                    fails.append("%s (%d, %d) %s lane %d, %s: verdict %d from the Python oracle, %d from the C++ oracle" %
                                 (curve, m, n, name, b, what, v_py, v_c))
                checks += 1
            checks += 1
    return fails, checks


def run_engine(eng, coracle, curve, m, n, name):
    """table creation succeeds; the prover's bytes are the oracle's under every plan; the verifier accepts them under the merged and the
    per-equation strategy and rejects one changed response scalar per proof with the oracle's check code"""
    s = cases(coracle, curve, m, n, name)
    tag = "%s (%d, %d) %s" % (curve, m, n, name)
    fails, checks = [], 0
    lanes = s["lanes"]
    dsz, psz = len(lanes[0]["deck"]), coracle.proof_size(m, n, curve)
    t = eng.table(m, n, s["params"], s["pk"])
    args = (b"".join(ln["deck"] for ln in lanes), b"".join(ln["rho"] for ln in lanes), [v for ln in lanes for v in ln["perm"]],
            b"".join(ln["seed"] for ln in lanes))

    def prove(plan):
        d, p, st = t.shuffle_and_remask_batch(*args)
        for b, ln in enumerate(lanes):
            if st[b] != 0 or d[dsz * b:dsz * (b + 1)] != ln["shuffled"] or p[psz * b:psz * (b + 1)] != ln["proof"]:
                fails.append("%s, %s: lane %d: status %d, the shuffled deck %s, the proof %s the oracle's" %
                             (tag, plan, b, st[b], "is" if d[dsz * b:dsz * (b + 1)] == ln["shuffled"] else "is not",
                              "is" if p[psz * b:psz * (b + 1)] == ln["proof"] else "is not"))
        return len(lanes)

    # the plans of shuffle_edge_cases.run_prover that a shape with m = 2 has (no Toom-Cook below m = 3)
    for lb in (8192, 8, 0):
        t.set_latency_batch(lb)
        checks += prove("latency batch %d" % lb)
    t.set_bucket_min(2)
    checks += prove("bucket kernel from 2 terms")
    t.set_bucket_min(2048)
    t.set_latency_batch(8192)
    for split, prm in PLAN_PARAMS:
        t.set_plan_params(split, *prm)
        t.set_work_split(split)
        checks += prove("work split %d" % split)
    t.set_work_split(-1)

    decks = args[0]
    good = (b"".join(ln["shuffled"] for ln in lanes), b"".join(ln["proof"] for ln in lanes), [0] * len(lanes))
    bad_proofs = [_tamper(s, b, ln["proof"]) for b, ln in enumerate(lanes)]
    bad_exp = [coracle.verify_shuffle(curve, m, n, s["params"], s["pk"], ln["deck"], ln["shuffled"], bad_proofs[b]) for b, ln in enumerate(lanes)]
    if not all(bad_exp):
        fails.append("%s: the oracle accepts a changed response scalar: %s" % (tag, bad_exp))
    bad = (good[0], b"".join(bad_proofs), bad_exp)
    for lb in (8192, 0):
        t.set_latency_batch(lb)
        for merged in (True, False):
            t.set_merged_verify(merged)
            for what, (sh, pf, exp) in (("honest", good), ("one response scalar changed", bad)):
                got = t.verify_shuffle_batch(decks, sh, pf)
                if got != exp:
                    fails.append("%s, latency batch %d, merged %s, %s: status words %s, the oracle's %s" % (tag, lb, merged, what, got, exp))
                checks += len(exp)
    t.close()
    return fails, checks


def run_infinite_base(eng, coracle, curve, m, n, which):
    """a base at infinity other than the key sum: the table is refused with MP_ERR_BAD_ENCODING"""
    s = make_set(coracle, curve, m, n, which)
    try:
        t = eng.table(m, n, s["params"], s["pk"])
    except Exception as e:
        code = getattr(e, "code", None)
        return ([] if code == BAD_ENCODING else ["%s (%d, %d): %s at infinity: error %r" % (curve, m, n, which, e)]), 1
    t.close()
    return ["%s (%d, %d): a table with %s at infinity was created" % (curve, m, n, which)], 1
