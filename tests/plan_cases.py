"""Cases and checks for the static plans of layout.hpp on the engine: the smallest shapes at which PhaseBuilder::end and make_prove_plan /
make_verify_plan take each of their branches -- the cap of 128 sub-jobs per MSM and kind, the two-level combine tree at its sqrt rounding
edges, window-split jobs with and without the range-by-range pre-combine, the bucket threshold, late combines, keyed plans, Toom-Cook /
Karatsuba -- proved and verified against the C++ oracle.  Shared by tests/test_plan_emu.py (the kernel bodies under the development
emulator, CPU) and tests/test_gpu_plan.py (the gfx950 build); tests/test_plan_check.py asks the stand-alone plan checker
(tests/cpp/plan_check.cpp --features) whether every case still takes the branch it is listed for.

run_case returns (failure messages, number of checks made); nothing is skipped, and checks_expected gives the count the tests assert."""
import collections
import copy
import os
import subprocess

import mp_oracle as po
from shuffle_edge_cases import _pmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUCKET_MIN = 2048                   # engine_core.hpp: the engine's default threshold
BUCKET_MIN_SMALL_BATCH = 512        # engine_core.hpp: the finest split (3) takes min(threshold, this)
TOOM_SPLITS = (0, 2, 4)             # engine_core.hpp build_plans: the other splits keep Karatsuba
TOOM_MAX_M = 16                     # layout.hpp
B = 3

# params: (fixed terms, variable terms, bases per table lane, points per inversion, window lanes) of mp_set_plan_params for `split`;
# bucket_min None = the engine's default; branch: (phase, key, op, value) on the checker's --features line of that phase -- op "has" /
# "none" for the sets (flat = piece counts of combines without a tree, tree = pieces/group size, bucket = terms per bucket job), ">0" /
# "=0" for the counts (direct, cap_fixed, cap_var, wsplit_single, wsplit_multi, late)
Case = collections.namedtuple("Case", "name curve m n split params bucket_min keyed toom group_lanes branch")


def _c(name, m, n, split, params, branch, bucket_min=None, keyed=False, toom=True, group_lanes=(0,), curve="stark"):
    return Case(name, curve, m, n, split, params, bucket_min, keyed, toom, group_lanes, tuple(branch))


MERGED, PER_EQ = "verify.merged", "verify.per-equation"
CASES = [
    # the cap of 128 sub-jobs: 130 fixed terms per commitment at one term per job; 551 terms of the merged equation and 134 of the
    # ciphertext checks at one variable-base term per job
    _c("cap-fixed", 2, 129, 5, (1, 16, 2, 4, 1), [("prove.A", "cap_fixed", ">0"), (PER_EQ, "cap_fixed", ">0"), (MERGED, "cap_fixed", ">0")],
       group_lanes=(1, 4)),
    _c("cap-var", 2, 65, 1, (1, 1, 2, 4, 1), [(PER_EQ, "cap_var", ">0"), (MERGED, "cap_var", ">0")], group_lanes=(1, 4)),
    # the combine tree from 12 pieces on, groups of ceil(sqrt(pieces)): the merged equation of (2, 3) has 8 fixed and 54 variable terms
    _c("tree-11", 2, 3, 2, (4, 6, 8, 16, 1), [(MERGED, "flat", "has", "11"), (MERGED, "tree", "none")]),
    _c("tree-12", 2, 3, 2, (8, 5, 8, 16, 1), [(MERGED, "tree", "has", "12/4")], group_lanes=(1, 4)),
    _c("tree-13", 2, 3, 2, (4, 5, 8, 16, 1), [(MERGED, "tree", "has", "13/4")]),
    _c("tree-16", 2, 3, 2, (4, 4, 8, 16, 1), [(MERGED, "tree", "has", "16/4")]),
    _c("tree-17", 2, 3, 2, (3, 4, 8, 16, 1), [(MERGED, "tree", "has", "17/5")], group_lanes=(1, 4)),
    _c("tree-12-keyed", 2, 3, 2, (8, 5, 8, 16, 1), [(MERGED, "tree", "has", "12/4")], keyed=True),
    # a tree in the prover, next to the late combines of m = 2 in the same phase
    _c("tree-and-late", 2, 11, 5, (1, 8, 2, 4, 1), [("prove.A", "tree", "has", "12/4"), ("prove.B", "tree", "has", "12/4"), ("prove.B", "late", ">0")],
       group_lanes=(1, 4)),
    # window lanes: one sub-job per MSM (no pre-combine) and several; 2, 3 (51 windows: shares of 17), 16 lanes on one-term jobs (a
    # share of 3 windows for a job that has a single term), 5 lanes under Toom-Cook
    _c("lanes-2-single", 3, 2, 1, (1, 64, 4, 8, 2), [("prove.B", "wsplit_single", ">0"), ("prove.B", "wsplit_multi", "=0"), ("prove.B", "late", ">0")],
       group_lanes=(1, 4)),
    _c("lanes-2-single-keyed", 3, 2, 1, (1, 64, 4, 8, 2), [("prove.B", "wsplit_single", ">0"), ("prove.B", "late", ">0")], keyed=True),
    _c("lanes-3-multi", 3, 2, 5, (1, 2, 2, 4, 3), [(PER_EQ, "wsplit_multi", ">0"), (MERGED, "wsplit_multi", ">0")], group_lanes=(1, 4)),
    _c("lanes-16-one-term", 2, 3, 1, (1, 1, 2, 4, 16), [("prove.B", "wsplit_multi", ">0"), (MERGED, "wsplit_multi", ">0")], group_lanes=(1, 4)),
    _c("lanes-5-toom", 4, 3, 4, (4, 64, 16, 32, 5), [("prove.B", "wsplit_single", ">0"), ("prove.B2", "wsplit_single", ">0"), (MERGED, "wsplit_multi", ">0")]),
    # the bucket threshold at the merged equation's 54 terms and one above, on the finest split and on the latency split
    _c("bucket-at-finest", 2, 3, 3, (1, 1, 2, 4, 1), [(MERGED, "bucket", "has", "54")], bucket_min=54),
    _c("bucket-above-finest", 2, 3, 3, (1, 1, 2, 4, 1), [(MERGED, "bucket", "none")], bucket_min=55),
    _c("bucket-at-latency", 2, 3, 1, (1, 16, 4, 8, 16), [(MERGED, "bucket", "has", "54"), (PER_EQ, "bucket", "none")], bucket_min=54,
       group_lanes=(1, 4)),
    _c("bucket-above-latency", 2, 3, 1, (1, 16, 4, 8, 16), [(MERGED, "bucket", "none"), (MERGED, "wsplit_multi", ">0")], bucket_min=55),
    # Toom-Cook on and off at its smallest and largest m, Karatsuba beyond
    _c("toom-3", 3, 2, 0, (8, 64, 64, 64, 1), [("prove.B", "direct", ">0"), ("prove.B2", "flat", "has", "2"), ("prove.B", "late", "=0")]),
    _c("toom-off-3", 3, 2, 0, (8, 64, 64, 64, 1), [("prove.B", "late", ">0")], toom=False),
    _c("toom-16", 16, 2, 2, (4, 32, 8, 16, 4), [("prove.B2", "wsplit_single", ">0"), ("prove.B", "late", "=0")], group_lanes=(1, 4)),
    _c("toom-off-16", 16, 2, 2, (4, 32, 8, 16, 4), [("prove.B", "late", ">0"), ("prove.A2", "flat", "has", "2")], toom=False),
    _c("karatsuba-17", 17, 2, 4, (4, 64, 16, 32, 16), [("prove.B", "late", ">0"), ("prove.A2", "flat", "has", "2")], group_lanes=(1, 4)),
    # the other base fields
    _c("bn254", 3, 2, 2, (4, 16, 16, 32, 3), [("prove.B2", "wsplit_single", ">0")], curve="bn254"),
    _c("secp256k1", 3, 2, 5, (1, 2, 2, 4, 2), [(PER_EQ, "wsplit_multi", ">0")], curve="secp256k1"),
    _c("bls12_377", 3, 2, 0, (8, 64, 64, 64, 16), [("prove.B2", "wsplit_single", ">0")], curve="bls12_377"),
]
EMU_MAX_N = 34          # under the emulator: the cases of at most this many cards (the two sub-job cap cases are GPU-only)
# the four mutations of tests/test_gpu_parity.py test_merged_and_per_equation_verification_agree: one response scalar + 1 in each sub-argument
MUTATIONS = ((("product", "had", "zero"), "tbar", None), (("product", "svp"), "rt", None), (("mexp",), "taubar", None), (("mexp",), "abar", 1))
STAT_KEYS = ("fixed_terms", "var_terms", "fixed_jobs", "var_jobs", "table_bases", "combine_terms")


def executed(case):
    """the arguments of plan_check --features for the plan the engine executes on the case's split"""
    bmin = BUCKET_MIN if case.bucket_min is None else case.bucket_min
    if case.split == 3 and bmin:
        bmin = min(bmin, BUCKET_MIN_SMALL_BATCH)
    p = case.params
    return (case.m, case.n, p[0], p[1], p[4], bmin, int(case.keyed), int(case.toom and case.split in TOOM_SPLITS))


def described(case):
    """... and for the plan mp_plan_stats describes once the case's parameters are those of split 0: the throughput plan of the
    table's own key, Toom-Cook as set, the threshold as set"""
    p = case.params
    return (case.m, case.n, p[0], p[1], p[4], BUCKET_MIN if case.bucket_min is None else case.bucket_min, 0, int(case.toom))


def build_checker():
    exe = os.path.join(ROOT, "tests", "cpp", "_plan_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "plan_check.cpp"), os.path.join(ROOT, "mental-poker_amd", "csrc", "layout.hpp"),
            os.path.join(ROOT, "tools", "hostemu", "rt.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-include", srcs[2], "-I" + os.path.dirname(srcs[2]), "-I" + os.path.dirname(srcs[1]),
                               srcs[0], "-o", exe])
    return exe


_FEATURES = {}


def features(exe, args):
    """plan_check --features -> {"phase": {name: {key: value}}, "stats": {name: {key: int}}, "largest_msm": int}"""
    if args not in _FEATURES:
        r = subprocess.run([exe, "--features"] + [str(a) for a in args], stdout=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 0, "plan_check --features %s: %s" % (args, r.stdout)
        out = {"phase": {}, "stats": {}}
        for line in r.stdout.splitlines():
            w = line.split()
            if w[0] == "largest_msm":
                out["largest_msm"] = int(w[1])
            else:
                kv = dict(x.split("=") for x in w[2:])
                out[w[0]][w[1]] = kv if w[0] == "phase" else {k: int(v) for k, v in kv.items()}
        _FEATURES[args] = out
    return _FEATURES[args]


def branch_failures(exe, case):
    """the branches the case is listed for that its plan does not take (none: the list has not rotted)"""
    f = features(exe, executed(case))
    fails = []
    for phase, key, op, *val in case.branch:
        got = f["phase"].get(phase, {}).get(key)
        if got is None:
            ok = False
        elif op in ("has", "none"):
            have = set() if got == "-" else set(got.split(","))
            ok = (val[0] in have) if op == "has" else not have
        else:
            ok = (int(got) > 0) == (op == ">0")
        if not ok:
            fails.append("%s: %s %s is %s, expected %s %s" % (case.name, phase, key, got, op, " ".join(val)))
    if case.name.startswith("bucket-"):      # exactly at the largest MSM of the shape, or one above
        want = f["largest_msm"] + (1 if "-above-" in case.name else 0)
        if case.bucket_min != want:
            fails.append("%s: bucket_min %d, the merged equation has %d terms" % (case.name, case.bucket_min, f["largest_msm"]))
    return fails


class Material:
    """B generic witnesses of one (curve, m, n) from coracle.gen_inputs, the oracle's shuffled decks and proofs, lane 1's proof with each
    mutation and the oracle's verdicts -- under the table's key, or under one key per lane (keyed)"""

    def __init__(self, co, curve, m, n, keyed):
        self.cv = cv = po.CURVES[curve]
        gen = _pmap(lambda s: co.gen_inputs(curve, m, n, 9100 + s), range(B))
        self.params = gen[0]["params"]
        self.pks = [g["pk"] if keyed else gen[0]["pk"] for g in gen]
        self.decks, self.rho, self.seeds = [g["deck"] for g in gen], [g["rho"] for g in gen], [g["prover_seed"] for g in gen]
        self.perms = [v for g in gen for v in g["perm"]]
        outs = _pmap(lambda b: co.shuffle_and_remask(curve, m, n, self.params, self.pks[b], self.decks[b], self.rho[b], gen[b]["perm"], self.seeds[b]), range(B))
        self.shuffled, self.proofs = [o[0] for o in outs], [o[1] for o in outs]
        self.mutated = []
        with po.curve_ctx(cv):
            pf = po.proof_from_bytes(self.proofs[1], m, n)
            for path, key, idx in MUTATIONS:
                p2 = copy.deepcopy(pf)
                d = p2
                for k in path:
                    d = d[k]
                if idx is None:
                    d[key] = (d[key] + 1) % cv.q
                else:
                    d[key][idx] = (d[key][idx] + 1) % cv.q
                self.mutated.append(po.proof_to_bytes(p2))
        verdict = lambda b, p: co.verify_shuffle(curve, m, n, self.params, self.pks[b], self.decks[b], self.shuffled[b], p)
        self.honest = _pmap(lambda b: verdict(b, self.proofs[b]), range(B))
        self.verdicts = _pmap(lambda p: verdict(1, p), self.mutated)


_MATERIAL = {}


def material(co, case):
    """made once per (curve, m, n, keyed) and shared by the cases of that shape (nothing changes it)"""
    key = (case.curve, case.m, case.n, case.keyed)
    if key not in _MATERIAL:
        _MATERIAL[key] = Material(co, *key)
    return _MATERIAL[key]


def _kernels_ran(fails, tag, rep, f, split, gl):
    """an honest batch under merged verification ran the phase the plan says, on the kernels the plan and the group lanes say: the
    merged equation (on the finest split only where it is a bucket job: engine_core.hpp screens), its bucket job or window folds, and
    the one-lane or four-lane combine / fold kernels"""
    screens = split != 3 or f["phase"][MERGED]["bucket"] != "-"
    ph = f["phase"][MERGED if screens else PER_EQ]
    bucket, folds = ph["bucket"] != "-", int(ph["wsplit_single"]) + int(ph["wsplit_multi"]) > 0
    if ("k_verify_merge" in rep) != screens:
        fails.append("%s: the merged equation %s" % (tag, "did not run" if screens else "ran"))
    if ("k_bucket_recode" in rep) != bucket:
        fails.append("%s: the bucket kernels %s" % (tag, "did not run" if bucket else "ran"))
    quad = {1: (False,), 4: (True,)}.get(gl, (False, True))
    for kernel, wanted in (("k_combine", True), ("k_wfold", folds)):
        ran = {q for q in (False, True) if kernel + ("_q" if q else "") in rep}
        if (wanted and not (ran and ran <= set(quad))) or (not wanted and ran):
            fails.append("%s: %s: %s ran, expected %s of %s" % (tag, kernel, sorted(ran), "one" if wanted else "none", quad))
    return 4


def checks_expected(case):
    """per group-lane setting: B lanes proved, 2 x B honest status words, 4 mutations x 2 x B status words, 4 on the kernels that ran;
    then the 12 counts, the two
    bucket counts and the Toom-Cook word of mp_plan_stats; and the oracle's own verdicts (honest batch, the four mutations)"""
    return len(case.group_lanes) * (B + 2 * B + len(MUTATIONS) * 2 * B + 4) + 2 * len(STAT_KEYS) + 3 + 2


def run_case(eng, co, exe, case):
    """`eng`: an Engine of the case's curve"""
    m, n = case.m, case.n
    mt = material(co, case)
    tag = "%s (%s %d x %d, split %d %s)" % (case.name, case.curve, m, n, case.split, case.params)
    fails, checks = [], 0
    if mt.honest != [0] * B:
        fails.append("%s: the oracle rejects its own proofs: %s" % (tag, mt.honest))
    if not all(mt.verdicts):
        fails.append("%s: the oracle accepts a mutated proof: %s" % (tag, mt.verdicts))
    checks += 2
    cat = b"".join
    t = eng.table(m, n, mt.params, None if case.keyed else mt.pks[0], fb_bits=8)
    try:
        t.set_plan_params(case.split, *case.params)
        t.set_work_split(case.split)
        if case.bucket_min is not None:
            t.set_bucket_min(case.bucket_min)
        t.set_toom_cook(case.toom)
        keys, decks = cat(mt.pks), cat(mt.decks)
        dsz, psz = len(mt.decks[0]), len(mt.proofs[0])
        for gl in case.group_lanes:
            t.set_group_lanes(gl)
            gtag = "%s, group lanes %d" % (tag, gl)
            args = (decks, cat(mt.rho), mt.perms, cat(mt.seeds))
            d, p, st = t.shuffle_and_remask_batch_keys(keys, *args) if case.keyed else t.shuffle_and_remask_batch(*args)
            for b in range(B):
                if st[b] != 0:
                    fails.append("%s: prover lane %d: status %d" % (gtag, b, st[b]))
                elif d[b * dsz:(b + 1) * dsz] != mt.shuffled[b]:
                    fails.append("%s: prover lane %d: the shuffled deck differs from the oracle's" % (gtag, b))
                elif p[b * psz:(b + 1) * psz] != mt.proofs[b]:
                    fails.append("%s: prover lane %d: the proof differs from the oracle's" % (gtag, b))
                checks += 1
            batches = [("honest", mt.proofs, [0] * B)]
            batches += [("mutation %d" % k, [mt.proofs[0], mp, mt.proofs[2]], [0, mt.verdicts[k], 0]) for k, mp in enumerate(mt.mutated)]
            for merged in (True, False):
                t.set_merged_verify(merged)
                for name, proofs, exp in batches:
                    vargs = (decks, cat(mt.shuffled), cat(proofs))
                    profiled = merged and name == "honest"
                    if profiled:
                        eng.profile_enable(True)
                    got = t.verify_shuffle_batch_keys(keys, *vargs) if case.keyed else t.verify_shuffle_batch(*vargs)
                    if profiled:
                        rep = eng.profile_report()
                        eng.profile_enable(False)
                        checks += _kernels_ran(fails, gtag, rep, features(exe, executed(case)), case.split, gl)
                    if list(got) != exp:
                        fails.append("%s: %s, merged %s: status words %s, the oracle's %s" % (gtag, name, merged, list(got), exp))
                    checks += B
            t.set_merged_verify(True)
        # mp_plan_stats reads split 0 of the table's own key: give that split the case's parameters and compare with the checker's
        # reading of the same plan
        t.set_plan_params(0, *case.params)
        st, f = t.plan_stats(), features(exe, described(case))
        for side, name in (("prove", "prove"), ("verify", MERGED)):
            for k in STAT_KEYS:
                if st[side][k] != f["stats"][name][k]:
                    fails.append("%s: mp_plan_stats %s %s = %d, the checker counts %d" % (tag, side, k, st[side][k], f["stats"][name][k]))
                checks += 1
        for k in ("bucket_terms", "bucket_jobs"):
            want = f["stats"]["prove"][k] + f["stats"][MERGED][k]
            if st[k] != want:
                fails.append("%s: mp_plan_stats %s = %d, the checker counts %d" % (tag, k, st[k], want))
            checks += 1
        want = m if case.toom and 3 <= m <= TOOM_MAX_M else 0
        if st["toom_points_m"] != want:
            fails.append("%s: mp_plan_stats toom_points_m = %d, expected %d" % (tag, st["toom_points_m"], want))
        checks += 1
    finally:
        t.close()
    return fails, checks
