"""Cases, references and checks for shuffle proofs on DEGENERATE inputs: decks whose cards coincide, cancel or vanish, masking factors
0 / 1 / q - 1 / r, -r, permutations with structure, aggregate keys +-G -- the inputs on which the kernels between the group-law
primitives and the proof (k_toom_points, k_table, k_normalize, the Karatsuba path, k_var_msm / k_wfold, k_combine, k_group_tile, the
gathering in front of the bucket kernels) meet P + P, P - P and O.  Shared by tests/test_shuffle_edge_emu.py (the kernel bodies under the
development emulator, CPU) and tests/test_gpu_shuffle_edge.py (the gfx950 build) -- same cases, same expectations: exact equality with
the C++ oracle (coracle.shuffle_and_remask, coracle.verify_shuffle), which run_oracles_agree compares with the Python oracle.

Decks, factors and permutations are built from Python integers with mp_oracle.  Every run_* function returns (failure messages, number
of checks made); the tests assert that the list is empty.  No class and no lane is skipped or excused.

Card (r, t) of an m x n deck is entry r n + t.  The Toom-Cook evaluation (kernels_msm.hpp body_toom_points) works on the SHUFFLED deck
-- deck[perm[i]] + E(0; rho_i) -- so a class that is to put special points into it fixes rho and the permutation as well: the `_fixed`
classes (rho = 0, identity: shuffled == deck) and the `multiples` classes (rho and the permutation keep the rows multiples of one row)."""
import os
from concurrent.futures import ThreadPoolExecutor

import mp_oracle as po

# (curve, m, n) of the GPU tests: the smallest shapes that reach every Toom-Cook node set (direct and reciprocal points), the Karatsuba
# path (m = 17), m = 2, and two rows / two columns
SHAPES = [("stark", 2, 3), ("stark", 3, 2), ("stark", 4, 3), ("stark", 5, 2), ("stark", 8, 2), ("stark", 9, 2), ("stark", 16, 2),
          ("stark", 17, 2), ("bn254", 3, 2), ("bn254", 4, 3), ("secp256k1", 3, 2), ("secp256k1", 4, 3), ("bls12_377", 3, 2)]
# under the emulator (most of a minute per shape and function, where the GPU takes a second) one shape: Toom-Cook on the throughput,
# medium and wide splits, Karatsuba on the small-batch ones
EMU_SHAPES = [("stark", 3, 2)]
SMALLEST = {"stark": (2, 3), "bn254": (3, 2), "secp256k1": (3, 2), "bls12_377": (3, 2)}
WAVE_SHAPE = ("stark", 5, 2)        # the shape whose batch is padded with generic lanes to cross 64 lanes (GPU only: the emulator has no waves)
TOOM_MAX_M = 16                     # layout.hpp
# the (split, plan parameters) of tests/test_gpu_round4.py test_window_lanes_match_oracle
PLAN_PARAMS = ((2, (4, 16, 16, 32, 3)), (0, (8, 64, 64, 64, 16)), (1, (1, 2, 2, 4, 5)), (5, (1, 1, 2, 4, 2)), (4, (4, 64, 32, 32, 7)),
               (3, (1, 1, 2, 4, 4)))

# deck classes, witness classes, and deck classes whose shuffled deck is degenerate too; the order matters only to the defects of
# run_verifier (lane k of the special lanes takes defect k % 4: all_equal_fixed has its cards swapped)
CLASSES = ["all_equal", "rows_equal", "all_equal_fixed", "row_neg", "cols_equal", "open_deck", "all_inf_fixed", "c1_inf", "all_inf",
           "one_inf_each", "cards_are_bases", "multiples", "multiples_rev", "rho0_id", "rho_qm1_rev", "rho_pm", "rho1_swap",
           "rows_equal_fixed", "row_neg_fixed"]
KEY_CLASSES = ["pk_is_G", "pk_is_minus_G"]


def _pmap(fn, items):
    """the C++ oracle takes up to 0.7 s per proof at m = 16: its calls (ctypes drops the interpreter lock) on up to 16 host threads"""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(fn, items))


def _sc(v):
    return int(v).to_bytes(32, "little")


def _scalars(vs):
    return b"".join(_sc(v) for v in vs)


# The Toom-Cook nodes: pair p of the plan evaluates at +-pair_x(p), on the coefficients in direct or in reversed order.  These are
# copies by hand of layout.hpp ToomPlan::pair_x / pair_rev and of the same two expressions in kernels_msm.hpp body_toom_points; the
# engine exposes neither, so the copies are tied to the source text: toom_nodes_are_the_engines() fails when one of those four lines
# changes, and whoever changes the node set has to change this model (and then the roots in multiples_coefficients) with it.
def pair_x(p):
    return 1 if p == 0 else (p + 1) // 2 + 1


def pair_rev(p):
    return p != 0 and p % 2 == 0


TOOM_NODE_SOURCE = {
    "layout.hpp": ("static uint32_t pair_x(uint32_t p) { return p == 0 ? 1u : (p + 1) / 2 + 1; }",
                   "static bool pair_rev(uint32_t p) { return p != 0 && (p & 1u) == 0; }",
                   "static const uint32_t TOOM_MAX_M = 16;"),
    "kernels_msm.hpp": ("const uint32_t x = p == 0 ? 1u : (p + 1) / 2 + 1, yy = x * x;",
                        "const bool rev = p != 0 && (p & 1u) == 0;"),
}


def toom_nodes_are_the_engines():
    """-> the lines of TOOM_NODE_SOURCE that the engine's source no longer has (none: pair_x / pair_rev here are the engine's)"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mental-poker_amd", "csrc")
    missing = []
    for name, lines in TOOM_NODE_SOURCE.items():
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        missing += ["%s: %s" % (name, ln) for ln in lines if ln not in text]
    return missing


def _poly(roots):
    """coefficients, lowest first, of prod (X - x_k)"""
    c = [1]
    for x in roots:
        c = [(c[i - 1] if i else 0) - x * (c[i] if i < len(c) else 0) for i in range(len(c) + 1)]
    return c


def multiples_coefficients(m, reverse):
    """a_r of the `multiples` classes: the coefficients of a product of (X - x_k) over Toom-Cook nodes, read so that the DIRECT pairs
    (reverse = False) or the REVERSED pairs (reverse = True) of the plan evaluate that product; padded with zeros (those rows are O)"""
    if m < 3 or m > TOOM_MAX_M:
        a = [1, -1] + [0] * (m - 2)
        return a[::-1] if reverse else a
    if not reverse or m == 3:
        g = _poly([1, -1] + ([2, -2] if m >= 5 else []))
        g += [0] * (m - len(g))
        return g if reverse else g[::-1]          # direct pairs: coefficient s is row m - 1 - s
    h = _poly([2, -2] + ([1, -1] if m >= 5 else []))
    return h + [0] * (m - len(h))                 # reversed pairs: coefficient s is row s


def small_mul(cv, k, P):
    """[k]P for a small integer k of either sign"""
    R = po.pt_mul_raw(cv, abs(k), P)
    return po.pt_neg(cv, R) if k < 0 else R


def toom_evaluations(cv, m, n, deck, t=0, comp=0):
    """the 2 (m - 1) points C(+-x) that body_toom_points computes for column t, component comp of a (shuffled) deck"""
    out = []
    for p in range(m - 1):
        x = pair_x(p)
        rows = [(s if pair_rev(p) else m - 1 - s) for s in range(m)]
        pts = [deck[r * n + t][comp] for r in rows]
        for sign in (1, -1):
            acc = None
            for s in range(m):
                acc = po.pt_add(cv, acc, small_mul(cv, (sign * x) ** s, pts[s]))
            out.append(acc)
    return out


class Cases:
    """the table's parameters and key, the lanes of one (curve, m, n) and what the oracle makes of them"""

    def __init__(self, coracle, curve, m, n, seed=8000, pad_to=0):
        self.co, self.curve, self.m, self.n, self.N = coracle, curve, m, n, m * n
        self.cv = cv = po.CURVES[curve]
        n_gen = max(len(CLASSES), pad_to - len(CLASSES))
        seeds = ([seed] + [seed + 1 + k for k in range(len(CLASSES))] + [seed + 100 + 10 * j + k for j in (0, 1) for k in range(len(KEY_CLASSES))] +
                 [seed + 200 + k for k in range(n_gen)])
        self._gen = dict(zip(seeds, _pmap(lambda s: coracle.gen_inputs(curve, m, n, s), seeds)))
        self.g0 = g0 = self._gen[seed]
        self.params, self.pk = g0["params"], g0["pk"]
        self.pb = coracle.point_size(curve)
        with po.curve_ctx(cv):
            w = po.point_bytes()
            pts = [po.pt_from_wire(self.params[i:i + w]) for i in range(0, len(self.params), w)]
            self.pp = po.Params(cv, m, n, pts[0], pts[1:1 + n], pts[1 + n], pts[2 + n])
            self.pk_pt = po.pt_from_wire(self.pk)
            special = [self._lane(name, self._gen[seed + 1 + k]) for k, name in enumerate(CLASSES)]
            self.key_lanes = []
            for k, name in enumerate(KEY_CLASSES):
                g = self._gen[seed + 100 + k]
                key = pts[0] if name == "pk_is_G" else po.pt_neg(cv, pts[0])
                self.key_lanes.append(dict(name=name, special=True, pk=po.pt_wire(key), deck=g["deck"], rho=g["rho"], perm=list(g["perm"]),
                                           seed=g["prover_seed"]))
                g = self._gen[seed + 110 + k]
                self.key_lanes.append(dict(name="generic key %d" % k, special=False, pk=g["pk"], deck=g["deck"], rho=g["rho"],
                                           perm=list(g["perm"]), seed=g["prover_seed"]))
        # special and generic lanes side by side in a wave
        self.lanes = []
        for k, ln in enumerate(special):
            self.lanes.append(ln)
            self.lanes.append(self._generic(seed + 200 + k))
        k = len(special)
        while len(self.lanes) < pad_to:
            self.lanes.append(self._generic(seed + 200 + k))
            k += 1
        every = self.lanes + self.key_lanes
        outs = _pmap(lambda ln: coracle.shuffle_and_remask(curve, m, n, self.params, ln["pk"], ln["deck"], ln["rho"], ln["perm"], ln["seed"]), every)
        for ln, (d, p) in zip(every, outs):
            ln["shuffled"], ln["proof"] = d, p
        self.B = len(self.lanes)
        self.dsz, self.psz = len(g0["deck"]), coracle.proof_size(m, n, curve)

    def _generic(self, s):
        g = self._gen[s]
        return dict(name="generic %d" % s, special=False, pk=self.pk, deck=g["deck"], rho=g["rho"], perm=list(g["perm"]), seed=g["prover_seed"])

    def _lane(self, name, g):
        """class `name` from the generic material g (called under curve_ctx)"""
        cv, m, n, N, q, pp = self.cv, self.m, self.n, self.N, self.cv.q, self.pp
        D = po.deck_from_bytes(g["deck"])
        rho = [int.from_bytes(g["rho"][32 * i:32 * i + 32], "little") for i in range(N)]
        perm = list(g["perm"])
        neg = lambda c: (po.pt_neg(cv, c[0]), po.pt_neg(cv, c[1]))
        mul = lambda k, c: (small_mul(cv, k, c[0]), small_mul(cv, k, c[1]))
        base = name[:-6] if name.endswith("_fixed") else name
        deck = list(D)
        if base == "all_equal":
            deck = [D[0]] * N
        elif base == "rows_equal":
            deck = [D[i % n] for i in range(N)]
        elif base == "row_neg":
            for r in ((1, 3) if m >= 4 else (1,)):
                for t in range(n):
                    deck[r * n + t] = neg(deck[(r - 1) * n + t])
        elif base == "cols_equal":
            deck = [D[(i // n) * n] for i in range(N)]
        elif base == "open_deck":
            deck = [(None, c[1]) for c in D]
        elif base == "c1_inf":
            deck = [(c[0], None) for c in D]
        elif base == "all_inf":
            deck = [(None, None)] * N
        elif base == "one_inf_each":
            for r in range(m):
                c = deck[r * n + r % n]
                deck[r * n + r % n] = (None, c[1]) if r % 2 == 0 else (c[0], None)
        elif base == "cards_are_bases":
            ck = pp.ck
            pool = [(pp.G, self.pk_pt), (self.pk_pt, pp.G), (pp.H, ck[0]), (ck[0], ck[1 % n]), (pp.H, ck[n - 1]), (ck[n - 1], ck[0])]
            deck = [pool[i % len(pool)] for i in range(N)]
        elif base in ("multiples", "multiples_rev"):
            # row r = [a_r] R for one generic row R (row 0 itself where a_0 = 1); the same column permutation in every row and
            # rho(r, t) = a_r rho_t keep the SHUFFLED rows the same multiples of R' = sigma(R) + E(0; rho)
            a = multiples_coefficients(m, base == "multiples_rev")
            sigma = sorted(range(n), key=lambda t: perm[t])
            deck = [mul(a[r], D[t]) for r in range(m) for t in range(n)]
            perm = [r * n + sigma[t] for r in range(m) for t in range(n)]
            rho = [a[r] * rho[t] % q for r in range(m) for t in range(n)]
        elif base == "rho0_id":
            rho, perm = [0] * N, list(range(N))
        elif base == "rho_qm1_rev":
            rho, perm = [q - 1] * N, list(range(N - 1, -1, -1))
        elif base == "rho_pm":
            rho = [(rho[0] if i % 2 == 0 else q - rho[0]) if i < N - N % 2 else 0 for i in range(N)]
            perm = [(i + n) % N for i in range(N)]
        elif base == "rho1_swap":
            rho, perm = [1] * N, [1, 0] + list(range(2, N))
        else:
            raise KeyError(name)
        if name.endswith("_fixed"):
            rho, perm = [0] * N, list(range(N))
        if base in ("multiples", "multiples_rev") and 3 <= m <= TOOM_MAX_M:
            stale = toom_nodes_are_the_engines()
            assert not stale, "the Toom-Cook nodes of the engine have changed, this module's copy has not: %s" % stale
            ev = toom_evaluations(cv, m, n, [po.remask(pp, self.pk_pt, deck[perm[i]], rho[i]) for i in range(N)])
            assert any(e is None for e in ev), "%s at m = %d: no Toom-Cook evaluation is the point at infinity" % (name, m)
            assert len(set(ev)) < len(ev), "%s at m = %d: no two Toom-Cook evaluations coincide" % (name, m)
        return dict(name=name, special=True, pk=self.pk, deck=po.deck_to_bytes(deck), rho=_scalars(rho), perm=perm, seed=g["prover_seed"])

    def cat(self, key, lanes=None):
        return b"".join(ln[key] for ln in (self.lanes if lanes is None else lanes))

    def prover_args(self, lanes=None):
        lanes = self.lanes if lanes is None else lanes
        return (self.cat("deck", lanes), self.cat("rho", lanes), [v for ln in lanes for v in ln["perm"]], self.cat("seed", lanes))

    def expect(self, ln, shuffled=None, proof=None):
        return self.co.verify_shuffle(self.curve, self.m, self.n, self.params, ln["pk"], ln["deck"], shuffled or ln["shuffled"], proof or ln["proof"])


_CACHE = {}


def _cases(coracle, curve, m, n):
    """the lanes of a shape and the oracle's outputs, made once and shared by the tests (nothing changes them)"""
    key = (curve, m, n)
    if key not in _CACHE:
        _CACHE[key] = Cases(coracle, curve, m, n, pad_to=66 if key == WAVE_SHAPE else 0)
    return _CACHE[key]


def run_oracles_agree(coracle, curve):
    """the Python oracle and the C++ oracle make the same shuffled deck and proof of every class at the curve's smallest shape, and
    give the same verdict on it (CPU only)"""
    m, n = SMALLEST[curve]
    c = _cases(coracle, curve, m, n)
    fails, checks = [], 0
    with po.curve_ctx(c.cv):
        for ln in [l for l in c.lanes + c.key_lanes if l["special"]]:
            pk = po.pt_from_wire(ln["pk"])
            deck = po.deck_from_bytes(ln["deck"])
            rho = [int.from_bytes(ln["rho"][32 * i:32 * i + 32], "little") for i in range(c.N)]
            sh, pf = po.shuffle_and_remask(c.pp, pk, deck, rho, ln["perm"], ln["seed"])
            if po.deck_to_bytes(sh) != ln["shuffled"] or po.proof_to_bytes(pf) != ln["proof"]:
                fails.append("%s %s (%d, %d): the oracles' outputs differ" % (curve, ln["name"], m, n))
            v_py, v_c = po.verify_shuffle(c.pp, pk, deck, sh, pf), c.expect(ln)
            if v_py != v_c or v_c != 0:
                fails.append("%s %s (%d, %d): verdict %d from the Python oracle, %d from the C++ oracle" % (curve, ln["name"], m, n, v_py, v_c))
            checks += 2
    return fails, checks


def _compare(fails, tag, c, lanes, out):
    d, p, st = out
    for b, ln in enumerate(lanes):
        if st[b] != 0:
            fails.append("%s: lane %d (%s): status %d" % (tag, b, ln["name"], st[b]))
        elif d[b * c.dsz:(b + 1) * c.dsz] != ln["shuffled"]:
            fails.append("%s: lane %d (%s): shuffled deck differs from the oracle's" % (tag, b, ln["name"]))
        elif p[b * c.psz:(b + 1) * c.psz] != ln["proof"]:
            fails.append("%s: lane %d (%s): proof differs from the oracle's" % (tag, b, ln["name"]))
    return len(lanes)


def run_prover(eng, coracle, curve, m, n, torch, device):
    """all classes in one batch under every plan: shuffled decks and proofs are the oracle's bytes.  The key classes run under their
    own aggregate key per proof, given as wire points (host buffers) and by index into a key set (device buffers: torch tensors on
    `device`, "cpu" under the emulator)"""
    c = _cases(coracle, curve, m, n)
    fails, checks = [], 0
    toomk = 3 <= m <= TOOM_MAX_M
    has4 = toomk or n >= 4          # an MSM of at least 4 variable-base terms: the 2m-term interpolation of Toom-Cook, or n >= 4

    def run(tag, lanes, prove, toom, want=()):
        """one prove call: the oracle's bytes on every lane, k_toom_points ran or not as the plan says, the kernels of `want` ran"""
        eng.profile_enable(True)
        out = prove()
        rep = eng.profile_report()
        eng.profile_enable(False)
        if ("k_toom_points" in rep) != (toomk and toom):
            fails.append("%s %s: k_toom_points %s" % (curve, tag, "ran" if "k_toom_points" in rep else "did not run"))
        for k in want:
            if k not in rep:
                fails.append("%s %s: %s did not run (%s)" % (curve, tag, k, sorted(rep)))
        return _compare(fails, "%s (%d, %d) %s" % (curve, m, n, tag), c, lanes, out) + 1 + len(want)

    # ---- the deck and witness classes: one table, the table's key
    args = c.prover_args()
    t = eng.table(m, n, c.params, c.pk)
    one = lambda tag, toom, want=(): run(tag, c.lanes, lambda: t.shuffle_and_remask_batch(*args), toom, want)
    # Toom-Cook is the throughput, medium and wide splits' (0, 2, 4); the small-batch splits keep Karatsuba (engine_core.hpp
    # build_plans), so every 3 <= m <= 16 goes through both.  By batch size these batches take the finest split (latency batch 8192),
    # or the throughput split (8: beyond 3.5 x 8 proofs; 0: always).  Everything up to the loop over PLAN_PARAMS runs with the
    # engine's own plan parameters
    for lb in (8192, 8, 0):
        t.set_latency_batch(lb)
        checks += one("latency batch %d" % lb, lb != 8192)
    t.set_toom_cook(False)
    for split in (0, 4):
        t.set_work_split(split)
        checks += one("Toom-Cook off, work split %d" % split, False)
    t.set_toom_cook(True)
    t.set_work_split(-1)
    t.set_latency_batch(0)
    for lanes in (1, 4):
        t.set_transcript_lanes(lanes)
        checks += one("transcript lanes %d" % lanes, True)
    t.set_transcript_lanes(0)
    # MSMs of at least 4 variable-base terms on the bucket kernel.  Where the prover has none ((2, 3), (17, 2): n terms per MSM) the
    # kernel is then also forced from 2 terms on
    t.set_bucket_min(4)
    checks += one("bucket kernel from 4 terms", True, want=("k_bucket_msm",) if has4 else ())
    if not has4:
        t.set_bucket_min(2)
        checks += one("bucket kernel from 2 terms", True, want=("k_bucket_msm",))
    t.set_bucket_min(2048)          # (the default)
    t.set_latency_batch(8192)
    for split, prm in PLAN_PARAMS:
        t.set_plan_params(split, *prm)
        t.set_work_split(split)
        for lanes in (1, 0, 4):
            t.set_group_lanes(lanes)
            checks += one("work split %d, group lanes %d" % (split, lanes), split in (0, 2, 4))
    t.close()

    # ---- the key classes (pk = G, pk = -G next to generic keys) on a table without a key: explicit keys, and a key set by index
    kl = c.key_lanes
    K = len(kl)
    dv = _Dev(torch, device)
    t = eng.table(m, n, c.params, None)
    keys, kargs = c.cat("pk", kl), c.prover_args(kl)
    ks = t.keyset(keys)
    d_idx, d_perm = dv.ints(list(range(K))), dv.ints(kargs[2])
    d_decks, d_rho, d_seeds = dv.bytes(kargs[0]), dv.bytes(kargs[1]), dv.bytes(kargs[3])

    def by_index():
        od, op, st = dv.bytes(bytes(K * c.dsz)), dv.bytes(bytes(K * c.psz)), dv.status(K)
        dv.sync()
        t.shuffle_and_remask_batch_keyset_dev(ks, K, d_idx.data_ptr(), d_decks.data_ptr(), d_rho.data_ptr(), d_perm.data_ptr(), d_seeds.data_ptr(),
                                              od.data_ptr(), op.data_ptr(), st.data_ptr())
        eng.sync()
        return bytes(od.cpu().numpy().tobytes()), bytes(op.cpu().numpy().tobytes()), st.cpu().tolist()

    def both(tag, toom, want=()):
        return (run("explicit keys, " + tag, kl, lambda: t.shuffle_and_remask_batch_keys(keys, *kargs), toom, want) +
                run("key set, " + tag, kl, by_index, toom, want))

    checks += both("latency batch 8192", False)
    t.set_latency_batch(0)
    checks += both("latency batch 0", True)
    t.set_latency_batch(8192)
    for split in (0, 1, 4):         # a Toom-Cook split, a Karatsuba split, the wide split
        t.set_work_split(split)
        checks += both("work split %d" % split, split != 1)
    t.set_work_split(0)
    t.set_toom_cook(False)
    checks += both("Toom-Cook off, work split 0", False)
    t.set_toom_cook(True)
    t.set_bucket_min(4)
    checks += both("bucket kernel from 4 terms, work split 0", True, want=("k_bucket_msm",) if has4 else ())
    ks.close()
    t.close()
    return fails, checks


class _Dev:
    """buffers for the _dev entry points: torch tensors on `device` ("cpu" under the emulator, whose device pointers are host pointers)"""

    def __init__(self, torch, device):
        self.torch, self.device = torch, device

    def bytes(self, raw):
        return self.torch.frombuffer(bytearray(raw), dtype=self.torch.uint8).to(self.device)

    def ints(self, vals):
        return self.torch.tensor(vals, dtype=self.torch.int32).to(self.device)

    def status(self, count):
        return self.torch.full((count,), 55, dtype=self.torch.int32, device=self.device)

    def sync(self):
        if self.device != "cpu":
            self.torch.cuda.synchronize()


def defects(c, lanes):
    """one defect per special lane, on the oracle's outputs -> (shuffled decks, proofs, expected status words).  Lane k of the special
    lanes: k % 4 = 0: a response scalar + 1 (of the zero, the single-value-product, the multi-exponentiation argument in turn); 1: a
    proof point replaced by G (Hadamard c_B, zero c_D, multi-exponentiation c_B in turn); 2: cards 0 and 1 of the shuffled deck swapped;
    3: the shuffled deck of the neighbouring lane.  Generic lanes stay honest."""
    q, m, n = c.cv.q, c.m, c.n
    sh, pf = [ln["shuffled"] for ln in lanes], [ln["proof"] for ln in lanes]
    cb = 2 * c.pb
    k = 0
    with po.curve_ctx(c.cv):
        for b, ln in enumerate(lanes):
            if not ln["special"]:
                continue
            kind, var = k % 4, (k // 4) % 3
            k += 1
            if kind < 2:
                p = po.proof_from_bytes(ln["proof"], m, n)
                if kind == 0:
                    d, key = ((p["product"]["had"]["zero"], "tbar"), (p["product"]["svp"], "rt"), (p["mexp"], "taubar"))[var]
                    d[key] = (d[key] + 1) % q
                else:
                    d, key, i = ((p["product"]["had"], "cB", 0), (p["product"]["had"]["zero"], "cD", m + 1), (p["mexp"], "cB", m))[var]
                    d[key][i] = c.pp.G if d[key][i] != c.pp.G else c.pp.H
                pf[b] = po.proof_to_bytes(p)
            elif kind == 2:
                s = ln["shuffled"]
                sh[b] = s[cb:2 * cb] + s[:cb] + s[2 * cb:]
            else:
                sh[b] = lanes[(b + 1) % len(lanes)]["shuffled"]
    exp = _pmap(lambda b: c.expect(lanes[b], sh[b], pf[b]), range(len(lanes)))
    return b"".join(sh), b"".join(pf), exp


def _looked(t, B, exp):
    """proofs that take the per-equation pass after a failed screen: the rejected ones (per-proof screen), or the members of the failing
    groups (lane b is a member of group b mod (B / group size))"""
    L = t.group_size(B)
    if L == 0:
        return sum(1 for v in exp if v)
    T = B // L
    return L * len({b % T for b, v in enumerate(exp) if v})


def run_verifier(eng, coracle, curve, m, n, torch, device):
    """the oracle's outputs, honest and with one defect per degenerate lane, under every verification strategy: the status words are
    the oracle's verdicts"""
    c = _cases(coracle, curve, m, n)
    fails, checks = [], 0
    lanes, B = c.lanes, c.B
    decks = c.cat("deck")
    good = (c.cat("shuffled"), c.cat("proof"), [0] * B)
    honest_exp = _pmap(c.expect, lanes)
    if honest_exp != good[2]:
        fails.append("%s (%d, %d): the oracle rejects its own proofs: %s" % (curve, m, n, honest_exp))
    bad = defects(c, lanes)
    if not ({0, 1, 2, 3, 4} <= set(bad[2])) or not any(v == 0 for ln, v in zip(lanes, bad[2]) if ln["special"]):
        fails.append("%s (%d, %d): the defects have collapsed: expected status words %s" % (curve, m, n, bad[2]))
    tag0 = "%s (%d, %d)" % (curve, m, n)
    dv = _Dev(torch, device)

    def check(tag, got, exp):
        if got != exp:
            fails.append("%s %s: status words %s, the oracle's %s" % (tag0, tag, [(b, lanes[b]["name"], v) for b, v in enumerate(got) if v != exp[b]][:8],
                                                                     [(b, exp[b]) for b, v in enumerate(got) if v != exp[b]][:8]))
        return len(exp)

    t = eng.table(m, n, c.params, c.pk)
    for lb in (8192, 0):                                  # (small batches skip the screening pass unless the throughput plan is forced)
        t.set_latency_batch(lb)
        for merged in (True, False):
            t.set_merged_verify(merged)
            for name, (s, p, exp) in (("honest", good), ("defects", bad)):
                checks += check("latency batch %d, merged %s, %s" % (lb, merged, name), t.verify_shuffle_batch(decks, s, p), exp)
    t.set_merged_verify(True)
    t.set_latency_batch(8192)
    # group equations: the whole batch, 2, and a size that does not divide the batch; the wave kernel and the split pipeline
    per = 4 * m * n + 11 * m + 8
    t.set_work_split(0)
    odd = 0                                               # a size that does not divide the batch and still gives groups (the engine
    for L in range(3, B):                                 # takes a divisor near it, or falls back to the per-proof screen)
        t.set_group_verify(L * per, 0)
        if B % L and t.group_size(B) >= 2:
            odd = L
            break
    if not odd:
        fails.append("%s (%d, %d): no group size that does not divide %d gives groups" % (curve, m, n, B))
        odd = B // 2
    for L in (B, 2, odd):
        for bits, split in ((0, 12), (9, 12), (10, 12), (12, 12), (10, 10)):
            t.set_bucket_split(split)
            t.set_bucket_bits(bits)
            t.set_group_verify(L * per, 0)
            tag = "groups of %d (%d), %d-bit windows, split from %d" % (L, t.group_size(B), bits, split)
            eng.profile_enable(True)
            for name, (s, p, exp) in (("honest", good), ("defects", bad)):
                before = t.reverified_count()
                checks += check("%s, %s" % (tag, name), t.verify_shuffle_batch(decks, s, p), exp)
                looked = t.reverified_count() - before
                if looked != _looked(t, B, exp):
                    fails.append("%s %s, %s: %d proofs took the per-equation pass, expected %d" % (tag0, tag, name, looked, _looked(t, B, exp)))
            rep = eng.profile_report()
            eng.profile_enable(False)
            gs = t.group_size(B)
            if gs < 2 or (B % L == 0 and gs != L):
                fails.append("%s %s: group size %d" % (tag0, tag, gs))
            for k in ("k_chain_scalars", "k_bucket_acc" if bits >= split else "k_bucket_msm"):
                if k not in rep:
                    fails.append("%s %s: %s did not run (%s)" % (tag0, tag, k, sorted(rep)))
            checks += 4
    t.set_bucket_split(12)
    t.set_bucket_bits(0)
    # pipelined, device pointers: the group pass is the deferred screen
    t.set_group_verify(2 * per, 0)
    t.set_pipeline(1)
    d_decks = dv.bytes(decks)
    held = []
    dv.sync()
    for name, (s, p, exp) in (("honest", good), ("defects", bad), ("honest again", good)):
        st, ds, dp = dv.status(B), dv.bytes(s), dv.bytes(p)
        dv.sync()
        held.append((name, st, ds, dp, exp))
        t.verify_shuffle_batch_dev(B, d_decks.data_ptr(), ds.data_ptr(), dp.data_ptr(), st.data_ptr())
    eng.sync()
    for name, st, _, _, exp in held:
        checks += check("pipelined, %s" % name, st.cpu().tolist(), exp)
    t.set_pipeline(0)
    t.set_group_verify(0, 0)
    checks += _run_chains(t, c, fails, tag0)
    t.close()
    checks += _run_keyed(eng, c, fails, tag0, dv)
    return fails, checks


def _run_keyed(eng, c, fails, tag0, dv):
    """the key classes (pk = G, pk = -G, next to generic keys): explicit keys and a key set, honest and with defects"""
    kl = c.key_lanes
    K = len(kl)
    t = eng.table(c.m, c.n, c.params, None)
    keys, decks = c.cat("pk", kl), c.cat("deck", kl)
    good = (c.cat("shuffled", kl), c.cat("proof", kl), [0] * K)
    bad = defects(c, kl)
    swapped_keys = b"".join(ln["pk"] for ln in kl[1:] + kl[:1])         # every proof under its neighbour's key
    exp_swapped = _pmap(lambda b: c.co.verify_shuffle(c.curve, c.m, c.n, c.params, kl[(b + 1) % K]["pk"], kl[b]["deck"], kl[b]["shuffled"], kl[b]["proof"]), range(K))
    if not any(bad[2]) or not all(exp_swapped):
        fails.append("%s keyed: the defects have collapsed: %s, %s" % (tag0, bad[2], exp_swapped))
    ks = t.keyset(keys)
    d_idx, d_rot, d_decks = dv.ints(list(range(K))), dv.ints([(b + 1) % K for b in range(K)]), dv.bytes(decks)
    n = 0
    for lb in (8192, 0):
        t.set_latency_batch(lb)
        for name, ky, idx, (s, p, exp) in (("honest", keys, d_idx, good), ("defects", keys, d_idx, bad), ("neighbour's key", swapped_keys, d_rot, (good[0], good[1], exp_swapped))):
            got = t.verify_shuffle_batch_keys(ky, decks, s, p)
            st, ds, dp = dv.status(K), dv.bytes(s), dv.bytes(p)
            dv.sync()
            t.verify_shuffle_batch_keyset_dev(ks, K, idx.data_ptr(), d_decks.data_ptr(), ds.data_ptr(), dp.data_ptr(), st.data_ptr())
            eng.sync()
            for form, g in (("explicit keys", got), ("key set", st.cpu().tolist())):
                if g != exp:
                    fails.append("%s keyed, %s, latency batch %d, %s: status words %s, the oracle's %s" % (tag0, form, lb, name, g, exp))
                n += K
    ks.close()
    t.close()
    return n


def _run_chains(t, c, fails, tag0):
    """3-link chains the oracle makes from rho0_id (every deck of the chain the same bytes), all_equal, open_deck, and a generic chain
    whose middle deck is replaced: mp_verify_shuffle_chain, alone and with two tables per equation, gives the oracle's verdict link by link"""
    co, cv, m, n, L = c.co, c.curve, c.m, c.n, 3
    by = {ln["name"]: ln for ln in c.lanes}
    gen = [ln for ln in c.lanes if not ln["special"]]
    starts = [by["rho0_id"], by["all_equal"], by["open_deck"], gen[0]]
    T = len(starts)
    chain, proofs = [[s["deck"] for s in starts]], []
    def link(jk):
        j, k = jk
        w = starts[k] if starts[k]["name"] == "rho0_id" else gen[1 + (j * T + k) % (len(gen) - 1)]     # the witness of link j: rho = 0, identity; or generic
        return co.shuffle_and_remask(cv, m, n, c.params, c.pk, chain[j][k], w["rho"], w["perm"], bytes([j + 1]) + w["seed"][1:])
    for j in range(L):
        outs = _pmap(link, [(j, k) for k in range(T)])
        chain.append([o[0] for o in outs])
        proofs.append([o[1] for o in outs])
    if not (chain[0][0] == chain[1][0] == chain[3][0]):
        fails.append("%s chains: rho = 0 and the identity do not keep the deck" % tag0)
    tampered = [row[:] for row in chain]
    tampered[2][3] = gen[-1]["deck"]                      # a valid deck, the wrong one: links 1 and 2 of table 3
    n_checks = 0
    for name, ch in (("honest", chain), ("tampered middle deck", tampered)):
        exp = _pmap(lambda jk: co.verify_shuffle(cv, m, n, c.params, c.pk, ch[jk[0]][jk[1]], ch[jk[0] + 1][jk[1]], proofs[jk[0]][jk[1]]),
                    [(j, k) for j in range(L) for k in range(T)])
        if (name == "honest") != (not any(exp)) or (name != "honest" and [i for i, v in enumerate(exp) if v] != [1 * T + 3, 2 * T + 3]):
            fails.append("%s chains, %s: the oracle's verdicts are %s" % (tag0, name, exp))
        decks, pf = b"".join(b"".join(r) for r in ch), b"".join(b"".join(r) for r in proofs)
        for group in (0, 2):
            t.set_chain_group(group)
            got = t.verify_shuffle_chain(T, L, decks, pf)
            if got != exp:
                fails.append("%s chains, %s, %d tables per equation: status words %s, the oracle's %s" % (tag0, name, group, got, exp))
            n_checks += L * T
        t.set_chain_group(0)
    return n_checks
