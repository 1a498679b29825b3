"""Cases, references and checks for the primitive probe (tools/primcheck/prim_check.hip): one field operation or one group operation per
lane, compared with Python integers / the Python oracle's group law.  Shared by tests/test_primitives_emu.py (the probe built against the
development emulator, CPU) and tests/test_gpu_primitives.py (the gfx950 build) -- same cases, same expectations, exact equality.

Every run_* function returns a list of failure messages (operands in hex); the tests assert that it is empty."""
import ctypes
import functools
import os
import random
import subprocess

import numpy as np

import mp_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tools", "primcheck")
GPU_LIB = os.path.join(PROBE_DIR, "libprimcheck.so")
EMU_LIB = os.path.join(PROBE_DIR, "libprimcheck_emu.so")

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
FIELDS = ["%s_%s" % (c, f) for c in CURVES for f in ("fq", "fr")]

# families / operations and their output slots: the numbers are those of prim_check.hip
FIELD_FAMILIES = {
    "mul": (0, ["mul", "sqr", "mulsub", "mul(lazy)", "sqr(lazy)", "mulsub(lazy)"]),
    "linear": (1, ["add", "sub", "neg", "dbl", "add(lazy)", "sub(lazy)", "neg(lazy)", "dbl(lazy)"]),
    "combined": (2, ["sub_sub_dbl", "sub_dbl", "triple_add", "mulsub(sub_lazy)", "mul(neg_lazy)", "mul(sub_wide)", "sqr(sub_wide)",
                     "is_zero(sub_wide)", "mulsub(sub_wide, sub_lazy)"]),
    "zero": (3, ["is_zero / eq flags"]),
    "misc": (4, ["pack", "unpack(pack)", "from_u32", "half", "in_range / canonical round trip"]),
    "inverse": (5, ["inv", "inv_divsteps(lazy)", "inv_fermat", "inv_fermat(lazy)"]),
}
GROUP_OPS = {"xyzz_dbl": 0, "xyzz_madd_signed": 1, "xyzz_add": 2, "jac_dbl": 3, "jac_madd": 4, "jac_add": 5, "xyzz_to_jac": 6,
             "aff_on_curve": 7, "dbl_chain_250": 8, "madd_run_300": 9}
QUAD_OPS = {"xyzz_dbl_quad": 0, "xyzz_madd_quad": 1, "xyzz_add_quad": 2}
DBL_CHAIN_LEN, MADD_RUN_LEN = 250, 300
WAVE_NOUT, BLOCK_NOUT = 18, 2

N_EDGE, N_RANDOM, N_INVERSE = 40000, 5000, 8000      # tuples per field per family (inverse: N_INVERSE in all)
N_GROUP = 3072                                        # cases per curve per group operation (192 waves of 16 quads)
N_CHAIN = 64


def field_info(name):
    curve, which = name.rsplit("_", 1)
    cv = mo.CURVES[curve]
    fr = which == "fr"
    p = cv.q if fr else cv.p
    nw = 8 if fr or curve != "bls12_377" else 12
    # Montgomery radix of the representation: 8x32 words for the scalar fields, 29-bit limbs (9; 14 on BLS12-377) for the base fields
    rbits = 256 if fr else (29 * 14 if curve == "bls12_377" else 29 * 9)
    return dict(name=name, curve=curve, fr=fr, p=p, nw=nw, rbits=rbits)


# ---- edge values ---------------------------------------------------------------------------------------------------------------------
def _limb_patterns(bits, w):
    nl = -(-bits // w)
    ones = (1 << w) - 1
    pats = [[ones] * nl, [ones if i % 2 == 0 else 0 for i in range(nl)], [0 if i % 2 == 0 else ones for i in range(nl)],
            [1 << (w - 1)] * nl, [ones - 1] * nl, [0x55555555 & ones] * nl, [0xAAAAAAAA & ones] * nl]
    for j in range(nl):
        for fill, special in ((ones, 1), (0, ones), (ones, 0), (0, 1 << (w - 1)), (ones, ones - 1)):
            limbs = [fill] * nl
            limbs[j] = special
            pats.append(limbs)
    return [sum(v << (w * i) for i, v in enumerate(limbs)) for limbs in pats]


@functools.lru_cache(maxsize=None)
def edge_values(p):
    """0, 1, 2, 3, p - 1 .. p - 3, (p +- 1) / 2, 2^k, 2^k +- 1, p - 2^k, limb patterns of the 29-bit and 32-bit forms (all ones, zero,
    alternating, top bit, 2^w - 2, ones with one 1, ...) reduced and truncated below p, their negatives, and seeded random values"""
    bits = p.bit_length()
    vals = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2]
    for k in range(bits):
        vals += [1 << k, (1 << k) + 1, (1 << k) - 1, p - (1 << k)]
    for w in (29, 32):
        for v in _limb_patterns(bits, w):
            for x in (v % p, v & ((1 << (bits - 1)) - 1)):
                vals += [x, (p - x) % p]
    rng = random.Random(p % 1000003)
    vals += [rng.randrange(p) for _ in range(64)]
    seen, out = set(), []
    for v in vals:
        v %= p
        if v not in seen:
            seen.add(v)
            out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def field_tuples(p, n_edge=N_EDGE, n_random=N_RANDOM):
    """(a, b, c, d, mode) per case: n_edge tuples drawn from the edge set (every edge value comes first as a, then as b), n_random random
    ones; a share of the tuples has b = a, c = -a or d = a b, so that zero tests and differences meet true zeros.  mode: four 3-bit
    selectors of the chain that pushes an operand away from its canonical representative (prim_check.hip lazy_rep)."""
    rng = random.Random(p % 999983 + 17)
    E = edge_values(p)
    out = []
    for i in range(n_edge + n_random):
        if i < n_edge:
            a, b, c, d = (rng.choice(E) for _ in range(4))
            if i < len(E):
                a = E[i]
            elif i < 2 * len(E):
                b = E[i - len(E)]
        else:
            a, b, c, d = (rng.randrange(p) for _ in range(4))
        k = i % 16
        if k == 3:
            b = a
        elif k == 5:
            c = (p - a) % p
        elif k == 7:
            d = a * b % p
        elif k == 9:
            b, c = a, (p - a) % p
        elif k == 11:
            d = a * a % p
            b = a
        out.append((a, b, c, d, rng.getrandbits(12)))
    return tuple(out)


# ---- the probe -----------------------------------------------------------------------------------------------------------------------
def build_emu_probe():
    """the probe against the development emulator (kernel bodies as CPU loops): the recipe of tests/cpp/field_check.cpp"""
    src = os.path.join(PROBE_DIR, "prim_check.hip")
    csrc = os.path.join(ROOT, "mental-poker_amd", "csrc")
    emu = os.path.join(ROOT, "tools", "hostemu")
    deps = [src, os.path.join(emu, "rt.hpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(EMU_LIB) or os.path.getmtime(EMU_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-x", "c++", "-include", os.path.join(emu, "rt.hpp"),
                               "-I" + emu, "-I" + csrc, src, "-o", EMU_LIB])
    return EMU_LIB


def _words(values, nw):
    nb = 4 * nw
    return np.frombuffer(b"".join(int(v).to_bytes(nb, "little") for v in values), dtype="<u4").copy()


def _ints(arr, nw):
    """uint32 array (..., nw) -> flat list of Python integers"""
    raw = np.ascontiguousarray(arr, dtype="<u4").tobytes()
    nb = 4 * nw
    return [int.from_bytes(raw[i:i + nb], "little") for i in range(0, len(raw), nb)]


class Probe:
    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError("%s is not built (the gfx950 probe is built by __graft_entry__.build())" % path)
        self.lib = ctypes.CDLL(path)
        self.dead = None
        self.rt_name = self._fn("pc_rt_name", ctypes.c_char_p)().decode()

    def _fn(self, name, restype=ctypes.c_int):
        f = getattr(self.lib, name)
        f.restype = restype
        return f

    def _run(self, what, fn, args, error_fn):
        """a runtime error (a failed launch or copy) ends the probe's use of the device: nothing more is launched after it"""
        if self.dead:
            raise RuntimeError("prim_check: not run, an earlier call failed: %s" % self.dead)
        if fn(*args) != 0:
            self.dead = "%s: %s" % (what, self._fn(error_fn, ctypes.c_char_p)().decode())
            raise RuntimeError("prim_check " + self.dead)

    def _call(self, curve, kind, *args):
        self._run("%s %s" % (kind, curve), self._fn("pc_%s_%s" % (kind, curve)), args, "pc_error_%s" % curve)

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def field(self, name, family, tuples):
        """-> uint32 array (cases, slots, nw)"""
        info = field_info(name)
        fam, slots = FIELD_FAMILIES[family]
        nw, n = info["nw"], len(tuples)
        ins = _words([v for t in tuples for v in t[:4]], nw)
        aux = np.array([t[4] for t in tuples], dtype="<u4")
        out = np.zeros(n * len(slots) * nw, dtype="<u4")
        self._call(info["curve"], "field", ctypes.c_int(1 if info["fr"] else 0), ctypes.c_int(fam), ctypes.c_uint32(n), self._p(ins), self._p(aux),
                   self._p(out))
        return out.reshape(n, len(slots), nw)

    def group(self, curve, op, P, Q, aux, quad=False):
        """P, Q: lists of 4-tuples of integers -> uint32 array (cases, 4, nw); quad: (cases, 4 lanes, 4, nw)"""
        nw = field_info(curve + "_fq")["nw"]
        n = len(P)
        pw, qw = _words([v for t in P for v in t], nw), _words([v for t in Q for v in t], nw)
        auxw = np.array(aux, dtype="<u4")
        out = np.zeros(n * (4 if quad else 1) * 4 * nw, dtype="<u4")
        self._call(curve, "quad" if quad else "group", ctypes.c_int(op), ctypes.c_uint32(n), self._p(pw), self._p(qw), self._p(auxw), self._p(out))
        return out.reshape((n, 4, 4, nw) if quad else (n, 4, nw))

    def helpers(self, rows, block=False):
        rows = np.ascontiguousarray(rows, dtype="<u4")
        n, width = rows.shape
        assert width == (256 if block else 64)
        nout = BLOCK_NOUT if block else WAVE_NOUT
        out = np.zeros(n * width * nout, dtype="<u4")
        self._run("helpers", self._fn("pc_block_helpers" if block else "pc_wave_helpers"), (ctypes.c_uint32(n), self._p(rows), self._p(out)),
                  "pc_error_stark")
        return out.reshape(n, width, nout)


# ---- field reference -------------------------------------------------------------------------------------------------------------------
def _field_expected(info, family, tuples):
    """-> list of rows of expected slot values (Python integers)"""
    p = info["p"]
    if family == "mul":
        return [(a * b % p, a * a % p, (a * b - c * d) % p) * 2 for a, b, c, d, _ in tuples]
    if family == "linear":
        return [((a + b) % p, (a - b) % p, -a % p, 2 * a % p) * 2 for a, b, c, d, _ in tuples]
    if family == "combined":
        rows = []
        for a, b, c, d, _ in tuples:
            p1, p2 = a * b % p, c * c % p
            p3 = (p1 - c * d) % p
            x3 = (p2 - p1 - 2 * p3) % p
            w = (p1 - d) % p
            rows.append((x3, (p2 - 2 * p1) % p, (3 * p2 + p3) % p, (a * (b - c) - d * p1) % p, -a * b % p, w * b % p, w * w % p,
                         (1 if w == 0 else 0) | 6, (w * (p2 - x3) - d * p1) % p))
        return rows
    if family == "zero":
        always = (1 << 4) | (1 << 5) | (1 << 6) | (1 << 7) | (1 << 8) | (1 << 11) | (1 << 13) | (1 << 14)
        rows = []
        for a, b, c, d, _ in tuples:
            fl = always
            if a == 0:
                fl |= 1 | 2
            if a == b:
                fl |= (1 << 2) | (1 << 3) | (1 << 9)
            if (a + c) % p == 0:
                fl |= (1 << 10) | (1 << 15)
            if a * b % p == 0:
                fl |= 1 << 12
            rows.append((fl,))
        return rows
    if family == "misc":
        R = (1 << info["rbits"]) % p
        inv2 = pow(2, -1, p)
        l29 = not info["fr"]
        return [(a * R % p, a, (a & 0xFFFFFFFF) % p, 0 if l29 else a * inv2 % p, 3) for a, b, c, d, _ in tuples]
    if family == "inverse":
        return [(pow(a, p - 2, p),) * 4 for a, b, c, d, _ in tuples]      # (the inverse of 0 is 0)
    raise KeyError(family)


def run_field(probe, name, family):
    info = field_info(name)
    tuples = field_tuples(info["p"])
    if family == "inverse":
        n_e = N_INVERSE * 7 // 8
        tuples = tuples[:n_e] + tuples[N_EDGE:N_EDGE + N_INVERSE - n_e]
    _, slots = FIELD_FAMILIES[family]
    nw = info["nw"]
    got = probe.field(name, family, tuples)
    want_rows = _field_expected(info, family, tuples)
    want = _words([v for r in want_rows for v in r], nw).reshape(got.shape)
    fails = []
    if got.tobytes() != want.tobytes():
        bad = np.argwhere((got != want).any(axis=2))
        for i, k in bad[:8]:
            a, b, c, d, mode = tuples[i]
            fails.append("%s %s: case %d a=%#x b=%#x c=%#x d=%#x mode=%#05x  got %#x  want %#x" %
                         (name, slots[k], i, a, b, c, d, mode, _ints(got[i, k], nw)[0], want_rows[i][k]))
        fails.append("%s %s: %d of %d results differ" % (name, family, len(bad), got.shape[0] * got.shape[1]))
    return fails, got.shape[0] * got.shape[1]


# ---- group cases -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_points(curve):
    cv = mo.CURVES[curve]
    rng = random.Random(cv.cid + 40)
    ks = [1, 2, 3, 5, 7, cv.q - 1, cv.q - 2, (cv.q - 1) // 2, (cv.q + 1) // 2] + [rng.randrange(1, cv.q) for _ in range(23)]
    return tuple(mo.pt_mul(cv, k, cv.G) for k in ks)


CLASSES = ["generic", "P+P", "P+(-P)", "infinity+Q", "P+infinity", "infinity+infinity"]


def _rand_z(rng, p, i):
    return (1, p - 1, 2, (p + 1) // 2)[i % 4] if i % 13 == 0 else rng.randrange(1, p)


def _xyzz(rng, p, P, z):
    if P is None:
        return (rng.randrange(p), rng.randrange(p), 0, 0)
    zz, zzz = z * z % p, z * z * z % p
    return (P[0] * zz % p, P[1] * zzz % p, zz, zzz)


def _jac(rng, p, P, z):
    if P is None:
        return (rng.randrange(p), rng.randrange(p), 0, 0)
    return (P[0] * z * z % p, P[1] * z * z * z % p, z, 0)


def _aff(P):
    return (0, 0, 0, 0) if P is None else (P[0], P[1], 0, 0)


def pair_cases(curve, n, uniform, seed):
    """(P, zP, Q, zQ, class, mode) per case.  uniform: the 16 cases of a wave (64 lanes = 16 quads) share class and mode; else neighbours differ"""
    cv = mo.CURVES[curve]
    rng = random.Random(seed)
    pts = base_points(curve)
    out = []
    for i in range(n):
        g = i // 16 if uniform else i
        cls, mode = g % 6, (g // 6) % 8
        P, Q = rng.choice(pts), rng.choice(pts)
        while Q == P or Q == mo.pt_neg(cv, P):
            Q = rng.choice(pts)
        if cls == 1:
            Q = P
        elif cls == 2:
            Q = mo.pt_neg(cv, P)
        elif cls == 3:
            P = None
        elif cls == 4:
            Q = None
        elif cls == 5:
            P = Q = None
        out.append((P, _rand_z(rng, cv.p, i), Q, _rand_z(rng, cv.p, i + 5), cls, mode))
    return out


def _check_xyzz(cv, got, want):
    p = cv.p
    X, Y, ZZ, ZZZ = got
    if max(got) >= p:
        return "a coordinate is not canonical"
    if want is None:
        return None if ZZ == 0 and ZZZ == 0 else "expected infinity (ZZ = 0, and ZZZ = 0 with it)"
    if ZZ == 0:
        return "infinity (ZZ = 0), expected a finite point"
    if pow(ZZ, 3, p) != ZZZ * ZZZ % p:
        return "ZZ^3 != ZZZ^2"
    if X != want[0] * ZZ % p or Y != want[1] * ZZZ % p:
        return "wrong point: X/ZZ = %#x, Y/ZZZ = %#x" % (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, p - 2, p) % p)
    return None


def _check_jac(cv, got, want):
    p = cv.p
    X, Y, Z, _ = got
    if max(got) >= p:
        return "a coordinate is not canonical"
    if want is None:
        return None if Z == 0 else "expected infinity (Z = 0)"
    if Z == 0:
        return "infinity (Z = 0), expected a finite point"
    if X != want[0] * Z * Z % p or Y != want[1] * Z * Z * Z % p:
        zi = pow(Z, -1, p)
        return "wrong point: X/Z^2 = %#x, Y/Z^3 = %#x" % (X * zi * zi % p, Y * zi * zi * zi % p)
    return None


def _fmt_pt(P):
    return "infinity" if P is None else "(%#x, %#x)" % P


def run_group(probe, curve, opname):
    cv = mo.CURVES[curve]
    p, op = cv.p, GROUP_OPS[opname]
    nw = field_info(curve + "_fq")["nw"]
    rng = random.Random(1000 + op)
    fails = []
    if opname == "aff_on_curve":
        pts = base_points(curve)
        E = edge_values(p)
        cases = []
        for i in range(N_GROUP):
            P = rng.choice(pts)
            k = i % 8
            xy = (P, (P[0], (P[1] + 1) % p), ((P[0] + 1) % p, P[1]), (0, 0), (0, P[1]), (P[0], 0), (rng.choice(E), rng.choice(E)), mo.pt_neg(cv, P))[k]
            cases.append((xy, (i // 8) % 8))
        got = probe.group(curve, op, [(x, y, y, x) for (x, y), _ in cases], [(0, 0, 0, 0)] * len(cases), [m << 4 for _, m in cases])
        for i, ((x, y), m) in enumerate(cases):
            want = 1 if (x, y) == (0, 0) or cv.is_on_curve((x, y)) else 0
            if int(got[i, 0, 0]) != want:
                fails.append("%s aff_on_curve: case %d (%#x, %#x) mode %d: got %d, want %d" % (curve, i, x, y, m, int(got[i, 0, 0]), want))
        return fails, len(cases)
    if opname in ("dbl_chain_250", "madd_run_300"):
        pts = base_points(curve)
        P_in, Q_in, aux, wants, notes = [], [], [], [], []
        for i in range(N_CHAIN):
            P, z, mode, neg = pts[i % len(pts)], _rand_z(rng, p, i), i % 8, (i // 2) & 1
            if opname == "dbl_chain_250":
                A = None if i % 16 == 15 else P
                want = mo.pt_mul(cv, pow(2, DBL_CHAIN_LEN, cv.q), A)
                Q = None
            else:
                s = -1 if neg else 1
                # the accumulator starts at k P: infinity, P + P at the first step, a run through infinity, a run that ends there
                k = (0, s, -s, -150 * s, -299 * s, -300 * s, rng.randrange(cv.q), 7)[(i // 4) % 8]
                A = mo.pt_mul(cv, k % cv.q, P)
                want = mo.pt_mul(cv, (k + s * MADD_RUN_LEN) % cv.q, P)
                Q = P
            P_in.append(_xyzz(rng, p, A, z))
            Q_in.append(_aff(Q))
            aux.append(neg | (mode << 4))
            wants.append(want)
            notes.append("start %s, operand %s, subtract %d, mode %d" % (_fmt_pt(A), _fmt_pt(Q), neg, mode))
        got = probe.group(curve, op, P_in, Q_in, aux)
        vals = _ints(got, nw)
        for i in range(N_CHAIN):
            err = _check_xyzz(cv, vals[4 * i:4 * i + 4], wants[i])
            if err:
                fails.append("%s %s: case %d %s: %s; want %s" % (curve, opname, i, notes[i], err, _fmt_pt(wants[i])))
        return fails, N_CHAIN
    cases = pair_cases(curve, N_GROUP, False, 7 * op + cv.cid)
    jac = opname.startswith("jac")
    enc_p = _jac if jac else _xyzz
    enc_q = (lambda r, pp, Q, z: _aff(Q)) if opname in ("xyzz_madd_signed", "jac_madd") else enc_p
    P_in = [enc_p(rng, p, P, zp) for P, zp, Q, zq, cls, mode in cases]
    Q_in = [enc_q(rng, p, Q, zq) for P, zp, Q, zq, cls, mode in cases]
    # (class = i % 6 and mode = (i // 6) % 8 in pair_cases: the sign changes every 48 cases, so every class meets every mode under both signs)
    negs = [((i // 48) & 1) if opname == "xyzz_madd_signed" else 0 for i in range(len(cases))]
    got = probe.group(curve, op, P_in, Q_in, [negs[i] | (c[5] << 4) for i, c in enumerate(cases)])
    vals = _ints(got, nw)
    for i, (P, zp, Q, zq, cls, mode) in enumerate(cases):
        if opname in ("xyzz_dbl", "jac_dbl"):
            want = mo.pt_add(cv, P, P)
        elif opname == "xyzz_to_jac":
            want = P
        else:
            want = mo.pt_add(cv, P, mo.pt_neg(cv, Q) if negs[i] else Q)
        err = (_check_jac if jac or opname == "xyzz_to_jac" else _check_xyzz)(cv, vals[4 * i:4 * i + 4], want)
        if err:
            fails.append("%s %s: case %d [%s%s, mode %d] P=%s z=%#x Q=%s z=%#x: %s; want %s; accumulator in %s" %
                         (curve, opname, i, CLASSES[cls], ", subtract" if negs[i] else "", mode, _fmt_pt(P), zp, _fmt_pt(Q), zq, err, _fmt_pt(want),
                          " ".join("%#x" % v for v in P_in[i])))
    return fails, len(cases)


def run_quad(probe, curve, opname, launch):
    """launch = 'divergent': every quad of a wave on a different class; 'uniform': the whole wave on the same class"""
    cv = mo.CURVES[curve]
    p, op = cv.p, QUAD_OPS[opname]
    nw = field_info(curve + "_fq")["nw"]
    uniform = launch == "uniform"
    rng = random.Random(2000 + op + (10 if uniform else 0))
    cases = pair_cases(curve, N_GROUP, uniform, 11 * op + cv.cid + (100 if uniform else 0))
    P_in = [_xyzz(rng, p, P, zp) for P, zp, Q, zq, cls, mode in cases]
    Q_in = [(_aff(Q) if opname == "xyzz_madd_quad" else _xyzz(rng, p, Q, zq)) for P, zp, Q, zq, cls, mode in cases]
    ons = []
    for i in range(len(cases)):
        g = i // 16 if uniform else i
        if opname == "xyzz_madd_quad":
            ons.append((1, 2, 1, 2, 0, 2, 1)[(g // 6 if uniform else g) % 7])
        else:
            ons.append(0 if (g // 6 if uniform else g) % 5 == 4 else 1)
    got = probe.group(curve, op, P_in, Q_in, [ons[i] | (c[5] << 4) for i, c in enumerate(cases)], quad=True)
    vals = _ints(got, nw)
    fails = []
    for i, (P, zp, Q, zq, cls, mode) in enumerate(cases):
        if ons[i] == 0:
            want = P
        elif opname == "xyzz_dbl_quad":
            want = mo.pt_add(cv, P, P)
        else:
            want = mo.pt_add(cv, P, mo.pt_neg(cv, Q) if ons[i] == 2 else Q)
        for lane in range(4):
            o = 16 * i + 4 * lane
            err = _check_xyzz(cv, vals[o:o + 4], want)
            if err:
                fails.append("%s %s (%s): case %d lane %d [%s, on %d, mode %d] P=%s z=%#x Q=%s z=%#x: %s; want %s" %
                             (curve, opname, launch, i, lane, CLASSES[cls], ons[i], mode, _fmt_pt(P), zp, _fmt_pt(Q), zq, err, _fmt_pt(want)))
    return fails, len(cases)


# ---- wave helpers ----------------------------------------------------------------------------------------------------------------------
def helper_rows(width, seed):
    """zeros, all ones, one hot lane, values whose sum crosses 2^16 and 2^31 (and 2^32), random values"""
    rng = np.random.RandomState(seed)
    rows = [np.zeros(width, dtype=np.uint32), np.full(width, 0xFFFFFFFF, dtype=np.uint32), np.ones(width, dtype=np.uint32)]
    for lane in range(width):
        for v in (1, 0x80000000):
            r = np.zeros(width, dtype=np.uint32)
            r[lane] = v
            rows.append(r)
    for total_bits in (16, 31, 32):
        each = (1 << total_bits) // width
        rows += [np.full(width, each, dtype=np.uint32), np.full(width, each + 1, dtype=np.uint32), np.full(width, each - 1, dtype=np.uint32)]
        rows.append(rng.randint(0, 2 * each, size=width).astype(np.uint32))
    for hi in (2, 1 << 8, 1 << 16, 1 << 26, 1 << 32):
        for _ in range(8):
            rows.append(rng.randint(0, hi, size=width, dtype=np.uint64).astype(np.uint32))
    return np.stack(rows)


def _diff(fails, what, got, want):
    if not np.array_equal(got, want):
        r = int(np.argwhere((got != want).reshape(got.shape[0], -1).any(axis=1))[0][0])
        fails.append("%s: row %d got %s want %s" % (what, r, " ".join("%x" % v for v in got[r].ravel()), " ".join("%x" % v for v in want[r].ravel())))


def run_wave_helpers(probe):
    rows = helper_rows(64, 5)
    got = probe.helpers(rows)
    n = rows.shape[0]
    fails = []
    incl = np.cumsum(rows.astype(np.uint64), axis=1).astype(np.uint32)      # (sums wrap modulo 2^32, as the 32-bit adds do)
    _diff(fails, "WaveCtx::excl_scan", got[:, :, 0], incl - rows)
    _diff(fails, "WaveCtx::max", got[:, :, 1], np.repeat(rows.max(axis=1)[:, None], 64, axis=1))
    _diff(fails, "WaveCtx::any", got[:, :, 2], np.repeat((rows != 0).any(axis=1).astype(np.uint32)[:, None], 64, axis=1))
    quads = rows.reshape(n, 16, 4)
    pair_b = (~rows + np.arange(64, dtype=np.uint32)[None, :]).astype(np.uint32).reshape(n, 16, 4)
    for k in (1, 2, 3):
        _diff(fails, "WaveCtx::quad_rot<%d>" % k, got[:, :, 2 + k], np.roll(quads, -k, axis=2).reshape(n, 64))
    for k in range(4):
        _diff(fails, "WaveCtx::quad_bcast<%d>" % k, got[:, :, 6 + k], np.repeat(quads[:, :, k:k + 1], 4, axis=2).reshape(n, 64))
        _diff(fails, "WaveCtx::quad_read<%d> word 0" % k, got[:, :, 10 + 2 * k], np.repeat(quads[:, :, k:k + 1], 4, axis=2).reshape(n, 64))
        _diff(fails, "WaveCtx::quad_read<%d> word 1" % k, got[:, :, 11 + 2 * k], np.repeat(pair_b[:, :, k:k + 1], 4, axis=2).reshape(n, 64))
    return fails, n


def run_block_helpers(probe):
    rows = helper_rows(256, 6)
    got = probe.helpers(rows, block=True)
    fails = []
    incl = np.cumsum(rows.astype(np.uint64), axis=1).astype(np.uint32)
    _diff(fails, "BlockCtx::excl_scan", got[:, :, 0], incl - rows)
    _diff(fails, "BlockCtx::max", got[:, :, 1], np.repeat(rows.max(axis=1)[:, None], 256, axis=1))
    return fails, rows.shape[0]


# ---- multi-scalar multiplication on exceptional inputs, through the public mp_msm --------------------------------------------------------
def run_msm_exceptional(eng, coracle, curve):
    """point sets full of duplicates, negatives and infinities under scalar patterns that make partial sums cancel, through the Straus
    path and the bucket path (several window widths); compared with the C++ oracle's MSM.  -> number of MSMs checked"""
    cv = mo.CURVES[curve]
    q, p, pb = cv.q, cv.p, eng.point_bytes
    fb = pb // 2
    gi = coracle.gen_inputs(curve, 2, 3, 5)
    t = eng.table(2, 3, gi["params"], gi["pk"])
    rng = random.Random(31 + cv.cid)
    base = eng.setup(2, 9, bytes([9] * 32))      # 12 points
    base = [base[pb * i:pb * (i + 1)] for i in range(12)]

    def neg(pt):
        y = int.from_bytes(pt[fb:], "little")
        return pt[:fb] + ((p - y) % p).to_bytes(fb, "little")

    inf = bytes(pb)
    K = 96
    # term i: base point i % 6 -- as it is, negated, or infinity
    pts_dup = [base[i % 6] for i in range(K)]
    pts_mixed = [(base[i % 6], neg(base[i % 6]), inf, base[i % 6])[(i // 6) % 4] for i in range(K)]
    pts_pairs = [base[(i // 2) % 12] for i in range(K)]                                  # the same point twice in a row
    pts_signs = [base[(i // 2) % 12] if i % 2 == 0 else neg(base[(i // 2) % 12]) for i in range(K)]      # P, -P, ...
    r = [rng.randrange(1, q) for _ in range(K)]
    low = rng.getrandbits(128)
    cases = [
        ("s and q - s on the same point", [r[i // 2] if i % 2 == 0 else q - r[i // 2] for i in range(K)], pts_pairs),
        ("s on P and on -P", [r[i // 2] for i in range(K)], pts_signs),
        ("s on P and q - s on -P", [r[i // 2] if i % 2 == 0 else q - r[i // 2] for i in range(K)], pts_signs),
        ("all scalars equal, duplicates", [r[0]] * K, pts_dup),
        ("all scalars equal, duplicates / negatives / infinities", [r[1]] * K, pts_mixed),
        ("all scalars 77", [77] * K, pts_mixed),
        ("0, 1, q - 1", [(0, 1, q - 1)[i % 3] for i in range(K)], pts_mixed),
        ("0, 1, q - 1 on duplicates", [(1, q - 1, 0, q - 1, 1)[i % 5] for i in range(K)], pts_dup),
        ("all 1", [1] * K, pts_dup),
        ("all q - 1", [q - 1] * K, pts_mixed),
        ("one bucket per window in the low half", [(low + (rng.getrandbits(120) << 128)) % q for _ in range(K)], pts_mixed),
        ("one bucket per window in the high half", [(rng.getrandbits(120) + ((low >> 8) << 128)) % q for _ in range(K)], pts_dup),
        ("random scalars on duplicates / negatives / infinities", r, pts_mixed),
        ("all zero", [0] * K, pts_mixed),
    ]
    checked = 0
    scb = b"".join(b"".join(s.to_bytes(32, "little") for s in sc) for _, sc, _ in cases)
    ptb = b"".join(b"".join(pts) for _, _, pts in cases)
    want = [coracle.msm(curve, scb[32 * K * j:32 * K * (j + 1)], ptb[pb * K * j:pb * K * (j + 1)]) for j in range(len(cases))]
    assert want[0] == inf and want[1] == inf and want[13] == inf      # (the patterns cancel as intended)
    for bucket_min, bits in ((0, 0), (16, 0), (16, 9), (16, 10), (16, 12)):      # 0: the Straus path; else the bucket method, 8- .. 12-bit windows
        t.set_bucket_min(bucket_min)
        t.set_bucket_bits(bits)
        got = t.msm(len(cases), K, scb, ptb)      # all the MSMs in one call ...
        for j, (what, sc, pts) in enumerate(cases):
            assert got[pb * j:pb * (j + 1)] == want[j], (curve, what, "bucket_min %d bits %d" % (bucket_min, bits), "batched")
            one = t.msm(1, K, scb[32 * K * j:32 * K * (j + 1)], ptb[pb * K * j:pb * K * (j + 1)])      # ... and each on its own
            assert one == want[j], (curve, what, "bucket_min %d bits %d" % (bucket_min, bits), "single")
            checked += 2
    t.set_bucket_bits(0)
    t.close()
    return checked
