"""Cases for the screening pass of the sigma verifiers (mp_set_sigma_screen): mp_unmask_batch[_dev], mp_verify_mask_batch[_dev],
mp_aggregate_keys_batch and mp_sigma_verify_batch with the checks of a group of lanes added up into one weighted equation, and the lanes
of a failing group re-verified one by one.  Shared by tests/test_sigma_screen_emu.py (the kernel bodies under the development emulator,
CPU) and tests/test_gpu_sigma_screen.py (the gfx950 build).

Two kinds of cases.  (1) The case functions of open_cases.py and deal_cases.py unmodified: they create their tables through
`eng.table(...)`, and `Screened(eng, g)` is an engine whose tables come back with set_sigma_screen(g, 1) applied -- the comparisons
with the C++ and Python oracles stay what they are; the proxy also notes, per verifying call, the lanes of the call and what the call
added to sigma_screen_stats.  (2) run_* functions of this file: a screened and an unscreened table side by side on the same inputs.
Every run_* function returns (failure messages, number of checks made)."""
import deal_cases as dc
import open_cases as oc
from trait_cases import Ctx

GROUP = 64                    # lanes per group: the shapes 1, 63, 64, 65 and 257 of the case files are a lone short group, a full group,
                              # a full group plus a group of one, and four groups with a tail of one
CHAUM_PEDERSEN, SCHNORR = 6, 5
BAD_ARGUMENT = -3
AUTO = 0xFFFFFFFF


class ScreenedTable:
    """a _native.Table with the screen on; everything else goes to the table itself"""
    VERIFIERS = {"unmask_batch": lambda a: len(a[3]), "unmask_batch_dev": lambda a: a[2] * a[4], "verify_mask_batch": lambda a: len(a[2]),
                 "verify_mask_batch_dev": lambda a: a[3], "aggregate_keys_batch": lambda a: a[0] * a[1], "sigma_verify_batch": lambda a: len(a[4]) // 32}

    def __init__(self, table, log, lanes, min_lanes):
        self._t, self._log = table, log
        table.set_sigma_screen(lanes, min_lanes)

    def __getattr__(self, name):
        f = getattr(self._t, name)
        lanes_of = self.VERIFIERS.get(name)
        if lanes_of is None:
            return f

        def call(*args):
            before = self._t.sigma_screen_stats()
            out = f(*args)
            if name.endswith("_dev"):
                self._t.eng.sync()
            after = self._t.sigma_screen_stats()
            self._log.append((name, lanes_of(args), [x - y for x, y in zip(after, before)]))
            return out
        return call


class Screened:
    """an engine whose tables screen their sigma verifiers with groups of `lanes` lanes"""

    def __init__(self, eng, lanes=GROUP, min_lanes=1):
        self._eng, self._lanes, self._min = eng, lanes, min_lanes
        self.log = []         # (call, lanes of the call, what it added to sigma_screen_stats)

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def table(self, *args, **kw):
        return ScreenedTable(self._eng.table(*args, **kw), self.log, self._lanes, self._min)


def honest_log_failures(log, group=GROUP):
    """after honest batches: every verifying call was screened in full, in ceil(lanes / group) equations, and no group failed"""
    fails = []
    if not log:
        fails.append("no verifying call was made")
    for name, lanes, d in log:
        if d != [lanes, (lanes + group - 1) // group, 0, 0]:
            fails.append("%s of %d lanes: sigma_screen_stats grew by %s" % (name, lanes, d))
    return fails


def screened_log_failures(log):
    """batches with defects: every verifying call went through the screen (call-level refusals never reach it: 0 lanes then)"""
    return ["%s of %d lanes: sigma_screen_stats grew by %s" % (n, l, d) for n, l, d in log if d[0] not in (0, l)] + \
        ([] if any(d[0] for _, _, d in log) else ["no call was screened"])


class Pair:
    """a screened and an unscreened table of one Ctx"""

    def __init__(self, eng, coracle, curve, lanes=GROUP, min_lanes=1):
        self.c = Ctx(eng, coracle, curve)
        self.off = self.c.t
        self.on = eng.table(self.off.m, self.off.n, self.c.params, self.c.pk)
        self.on.set_sigma_screen(lanes, min_lanes)

    def both(self, fails, tag, f):
        """f(table) on both tables: the results must be equal; -> (result, what the screened call added to the counters)"""
        want = f(self.off)
        before = self.on.sigma_screen_stats()
        got = f(self.on)
        d = [x - y for x, y in zip(self.on.sigma_screen_stats(), before)]
        if got != want:
            fails.append("%s: the screened call differs from the unscreened one (stats +%s)" % (tag, d))
        return want, d

    def close(self):
        self.on.close()
        self.c.close()


def _z_plus(c, p, k, nb=2):
    return p[:nb * c.pb] + c.sc((int.from_bytes(p[nb * c.pb:], "little") + k) % c.q)


def _a0_plus(c, p, D):
    return c.add(p[:c.pb], D) + p[c.pb:]


def run_equal(eng, coracle, curve):
    """the same inputs, with a few defects of every kind, through the five verifying calls on both tables: status words and outputs equal"""
    p = Pair(eng, coracle, curve)
    c, fails, checks = p.c, [], 0
    # opening: 65 lanes, a wrong token, a response >= q, a signer past the keys
    C, T = 13, 5
    b = oc.Batch(c, C, T, salt=51)
    d = oc._inputs(b)
    d["tokens"][3 * T + 2] = c.pool[0]
    d["proofs"][7 * T + 4] = d["proofs"][7 * T + 4][:2 * c.pb] + c.sc(c.q)
    d["signer"][12 * T + 4] = b.K
    lst = b.card_list(True)
    (plain, idx, ts, cs), st = p.both(fails, "%s unmask" % curve, lambda t: b.unmask(t, lst, signer=d["signer"], tokens=d["tokens"], proofs=d["proofs"]))
    if [(l, v) for l, v in enumerate(ts) if v] != [(3 * T + 2, CHAUM_PEDERSEN), (7 * T + 4, oc.BAD_ENCODING), (12 * T + 4, BAD_ARGUMENT)]:
        fails.append("%s unmask: token status %s" % (curve, [(l, v) for l, v in enumerate(ts) if v]))
    if st[:3] != [C * T, 2, 2] or st[3] != C * T:
        fails.append("%s unmask: stats +%s" % (curve, st))
    # ... and as mp_sigma_verify_batch takes the same statements (two bases, neither known to be G)
    rows = [oc._statement(c, d, l, T) for l in range(C * T - 1)]      # (without the lane whose signer names no key)
    fs = eng.blake2s(oc.REVEAL) * len(rows)
    sv, st = p.both(fails, "%s sigma_verify nbases 2" % curve,
                    lambda t: t.sigma_verify_batch(2, b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[2] for r in rows), fs))
    if sv != ts[:len(rows)] or st[0] != len(rows):
        fails.append("%s sigma_verify nbases 2: %s, stats +%s" % (curve, [(l, v) for l, v in enumerate(sv) if v], st))
    checks += 2 * C * T
    # dealing, both kinds: 65 lanes, a wrong response and a commitment off the curve
    for kind in dc.KINDS:
        db = dc.Deal(c, kind, 65, 7, salt=52)
        proofs = list(db.proofs)
        proofs[9] = _z_plus(c, proofs[9], 1)
        proofs[64] = c.off_curve(proofs[64][:c.pb]) + proofs[64][c.pb:]
        words, st = p.both(fails, "%s verify %s" % (curve, dc.KIND_NAME[kind]), lambda t: db.verify(t, proofs=proofs))
        if [(l, v) for l, v in enumerate(words) if v] != [(9, CHAUM_PEDERSEN), (64, dc.BAD_ENCODING)] or st != [65, 2, 2, 65]:
            fails.append("%s verify %s: status %s, stats +%s" % (curve, dc.KIND_NAME[kind], [(l, v) for l, v in enumerate(words) if v], st))
        checks += 65
    # seating: 65 lanes, a wrong response
    s = dc.Seating(c, 13, 5, salt=53)
    proofs = list(s.proofs)
    proofs[2 * 5 + 3] = _z_plus(c, proofs[2 * 5 + 3], 1, nb=1)
    (keys, ps, tst), st = p.both(fails, "%s seating" % curve, lambda t: s.run(t, proofs=proofs))
    if [(l, v) for l, v in enumerate(ps) if v] != [(13, SCHNORR)] or st != [65, 2, 1, 64]:
        fails.append("%s seating: player status %s, stats +%s" % (curve, [(l, v) for l, v in enumerate(ps) if v], st))
    fs1 = b"".join(c.fs_digest(s.fs_raw(l)) for l in range(65))
    sv, st = p.both(fails, "%s sigma_verify nbases 1" % curve, lambda t: t.sigma_verify_batch(1, c.G * 65, b"".join(s.pk), b"".join(proofs), fs1))
    if sv != ps or st != [65, 2, 1, 64]:
        fails.append("%s sigma_verify nbases 1: %s, stats +%s" % (curve, [(l, v) for l, v in enumerate(sv) if v], st))
    checks += 130
    p.close()
    return fails, checks


def run_localisation(eng, coracle, curve):
    """257 lanes in groups of 64: one tampered commitment at the first lane of a group, at the last lane of a group and at the single lane
    of the tail group; two defects in one group; a defect in every group.  Words and outputs equal the unscreened call's each time; a
    single defect fails one group and re-verifies that group's lanes only."""
    p = Pair(eng, coracle, curve)
    c, fails = p.c, []
    C = 257
    b = oc.Batch(c, C, 1, salt=61, edges=False)
    lst = [b.plain[0], b.plain[C - 1]]
    D = c.pool[2]
    for name, lanes, groups, relanes in (("first lane of a group", [128], 1, 64), ("last lane of a group", [127], 1, 64), ("the tail group's lane", [256], 1, 1),
                                         ("two defects in one group", [70, 100], 1, 64), ("a defect in every group", [5, 69, 133, 197, 256], 5, 257)):
        proofs = list(b.proofs)
        for l in lanes:
            proofs[l] = _a0_plus(c, proofs[l], D)
        (_, _, ts, _), st = p.both(fails, "%s %s" % (curve, name), lambda t: b.unmask(t, lst, proofs=proofs))
        if [l for l, v in enumerate(ts) if v] != lanes or any(ts[l] != CHAUM_PEDERSEN for l in lanes):
            fails.append("%s %s: token status %s" % (curve, name, [(l, v) for l, v in enumerate(ts) if v]))
        if st != [C, 5, groups, relanes] or (len(lanes) == 1 and not (st[2] == 1 and 1 <= st[3] <= 64)):
            fails.append("%s %s: stats +%s, expected %s" % (curve, name, st, [C, 5, groups, relanes]))
    p.close()
    return fails, 5 * C


def run_cancelling(eng, coracle, curve):
    """forgeries an unweighted sum of the checks would accept: A_0 + D in one lane and A_0 - D in another of the same group; two tokens of
    one card (same bases c0 and G) with z + 1 and z - 1.  Both lanes read 6 "Chaum-Pedersen", as in the unscreened call."""
    p = Pair(eng, coracle, curve)
    c, fails = p.c, []
    C, T = 8, 2
    b = oc.Batch(c, C, T, salt=71, edges=False)
    D = c.pool[3]
    for name, edits in (("A_0 + D and A_0 - D", {3: lambda q: _a0_plus(c, q, D), 12: lambda q: _a0_plus(c, q, c.neg(D))}),
                        ("z + 1 and z - 1 on one card", {6: lambda q: _z_plus(c, q, 1), 7: lambda q: _z_plus(c, q, -1)})):
        proofs = list(b.proofs)
        for l, f in edits.items():
            proofs[l] = f(proofs[l])
        (_, _, ts, _), st = p.both(fails, "%s %s" % (curve, name), lambda t: b.unmask(t, [], proofs=proofs))
        if [(l, v) for l, v in enumerate(ts) if v] != [(l, CHAUM_PEDERSEN) for l in sorted(edits)]:
            fails.append("%s %s: token status %s" % (curve, name, [(l, v) for l, v in enumerate(ts) if v]))
        if st != [C * T, 1, 1, C * T]:
            fails.append("%s %s: stats +%s" % (curve, name, st))
    p.close()
    return fails, 4 * C * T


def run_cofactor(eng, coracle, curve):
    """with mp_set_subgroup_check off the screen does not run on a curve with a cofactor (BLS12-377), and runs as before on the others"""
    p = Pair(eng, coracle, curve)
    c, fails = p.c, []
    C, T = 13, 5
    b = oc.Batch(c, C, T, salt=81, edges=False)
    toks = list(b.tokens)
    toks[9] = c.pool[0]
    for t in (p.on, p.off):
        t.set_subgroup_check(False)
    (_, _, ts, _), st = p.both(fails, "%s subgroup test off" % curve, lambda t: b.unmask(t, [], tokens=toks))
    want = [0, 0, 0, 0] if curve == "bls12_377" else [C * T, 2, 1, 64]
    if st != want or [(l, v) for l, v in enumerate(ts) if v] != [(9, CHAUM_PEDERSEN)]:
        fails.append("%s subgroup test off: stats +%s, expected %s; token status %s" % (curve, st, want, [(l, v) for l, v in enumerate(ts) if v]))
    for t in (p.on, p.off):
        t.set_subgroup_check(True)
    _, st = p.both(fails, "%s subgroup test on again" % curve, lambda t: b.unmask(t, [], tokens=toks))
    if st != [C * T, 2, 1, 64]:
        fails.append("%s subgroup test on again: stats +%s" % (curve, st))
    p.close()
    return fails, 2 * C * T


def run_usage(eng, coracle, curve):
    """a group too large for one bucket job is refused; min_lanes above the batch and the switch off leave the counters alone; the setter
    resets them"""
    p = Pair(eng, coracle, curve)
    c, fails = p.c, []
    for lanes in (98305, 1 << 20, AUTO - 1):
        try:
            p.on.set_sigma_screen(lanes, 1)
            fails.append("%s: %d lanes per group accepted" % (curve, lanes))
        except Exception as e:
            if getattr(e, "code", None) != BAD_ARGUMENT:
                fails.append("%s: %d lanes per group gives %r" % (curve, lanes, e))
    b = oc.Batch(c, 13, 5, salt=91, edges=False)
    run = lambda t: b.unmask(t, [b.plain[1]])      # noqa: E731
    _, st = p.both(fails, "%s after refused settings" % curve, run)      # (a refused call changes nothing: still groups of 64)
    if st != [65, 2, 0, 0]:
        fails.append("%s after refused settings: stats +%s" % (curve, st))
    for name, args, want in (("min_lanes above the batch", (GROUP, 66), [0, 0, 0, 0]), ("min_lanes = the batch", (GROUP, 65), [65, 2, 0, 0]),
                             ("one group larger than the batch", (98304, 1), [65, 1, 0, 0]), ("off", (0, 1), [0, 0, 0, 0])):
        p.on.set_sigma_screen(*args)
        if p.on.sigma_screen_stats() != [0, 0, 0, 0]:
            fails.append("%s %s: the setter left the counters at %s" % (curve, name, p.on.sigma_screen_stats()))
        _, st = p.both(fails, "%s %s" % (curve, name), run)
        if st != want:
            fails.append("%s %s: stats +%s, expected %s" % (curve, name, st, want))
    p.close()
    return fails, 8


def run_paths(eng, coracle, curve, lanes, kernel):
    """GPU: one opening call of `lanes` tokens under SIGMA_SCREEN_AUTO, tokens and proofs by the library's own reveal_batch; the engine's
    rule sizes the groups, and the kernels the call launched say which bucket path its equations took: `kernel` = "k_bucket_msm" (one
    wave per window), "k_bucket_sort" (the split pipeline) or None (this curve does not screen a call of this size under AUTO).  Once
    honest and once with three tampered lanes: words and outputs equal the unscreened call's."""
    import hashlib
    import random
    p = Pair(eng, coracle, curve, lanes=AUTO, min_lanes=1)
    c, fails = p.c, []
    T = 8
    C = lanes // T
    rng = random.Random(1234 + c.cv.cid)
    sk = [rng.randrange(3, c.q - 1) for _ in range(T)]
    keys = b"".join(c.mul(k, c.G) for k in sk)
    cards = b"".join(c.pool[1 + i % 15] + c.pool[1 + (3 * i + 1) % 15] for i in range(C))
    signer = [j for _ in range(C) for j in range(T)]
    seeds = b"".join(hashlib.blake2s(b"path seed %d" % l).digest() for l in range(lanes))
    tok, prf, st = p.off.reveal_batch(keys, b"".join(c.sc(k) for k in sk), cards, T, signer, seeds)
    if any(st):
        fails.append("%s: reveal status %s" % (curve, [(l, v) for l, v in enumerate(st) if v][:8]))
    psz = 2 * c.pb + 32
    for bad in ([], [0, lanes // 2 + 1, lanes - 1]):
        pf = bytearray(prf)
        for l in bad:
            pf[l * psz:(l + 1) * psz] = _z_plus(c, bytes(pf[l * psz:(l + 1) * psz]), 1)
        pf = bytes(pf)
        eng.profile_enable(True)
        (_, _, ts, _), d = p.both(fails, "%s %d lanes, tampered %s" % (curve, lanes, bad), lambda t: t.unmask_batch(keys, cards, T, signer, tok, pf))
        ran = eng.profile_report()
        eng.profile_enable(False)
        print("%s %d lanes, tampered %s: stats +%s, bucket kernels %s" % (curve, lanes, bad, d, sorted(k for k in ran if k.startswith("k_bucket"))))
        if [l for l, v in enumerate(ts) if v] != bad or any(ts[l] != CHAUM_PEDERSEN for l in bad):
            fails.append("%s %d lanes: token status %s, tampered %s" % (curve, lanes, [(l, v) for l, v in enumerate(ts) if v][:8], bad))
        if kernel is None:
            if d != [0, 0, 0, 0]:
                fails.append("%s %d lanes: screened under AUTO, stats +%s" % (curve, lanes, d))
            continue
        other = "k_bucket_sort" if kernel == "k_bucket_msm" else "k_bucket_msm"
        if kernel not in ran or other in ran:
            fails.append("%s %d lanes: expected %s, the call launched %s" % (curve, lanes, kernel, sorted(ran)))
        g = (lanes + d[1] - 1) // d[1] if d[1] else 0      # lanes per group as the engine chose them
        if d[0] != lanes or not d[1] or not (1 <= d[2] <= 3 if bad else d[2] == 0) or not (len(bad) <= d[3] <= d[2] * g):
            fails.append("%s %d lanes, tampered %s: stats +%s (groups of %d lanes)" % (curve, lanes, bad, d, g))
    p.close()
    return fails, 2 * lanes
