"""Cases, references and checks for the secrets drawn on the device from seeds ("mpshuffle secret stream v1", include/mpshuffle.h):
mp_sample_secrets_batch[_dev], mp_shuffle_and_remask_batch_seeded[_dev] and mp_keygen_batch, on every curve.  Shared by
tests/test_sample_emu.py (the kernel bodies under the development emulator, CPU) and tests/test_gpu_sample.py (the gfx950 build) -- same
cases, same expectations.

The expected stream is written out here on the Python oracle's pieces -- po.blake2s, po.ChaCha20Rng, po.fr_rand -- and the Fisher-Yates
rule of the header; points and proofs come from the C++ oracle (coracle.msm, coracle.sigma_prove, coracle.shuffle_and_remask) and, for one
tiny case each, from the Python oracle (po.shuffle_and_remask, po.player_keygen, po.sigma_prove).  Nothing here takes an expectation from
the engine; where agreement with another engine call is checked (the unseeded prover, mp_sigma_prove_batch, mp_msm), that call gets the
oracle-derived witness.

Every run_* function takes an engine (_native.Engine), the coracle module and a curve name, and returns (failure messages, number of
checks made); the tests assert that the list is empty."""
import ctypes
import functools
import hashlib
import struct

import mp_oracle as po
from trait_cases import CURVES  # noqa: F401  (for the test files)

TAG = b"mpshuffle secret stream v1"
LANES = (1, 63, 64, 65, 257)                                # around a wave and a block
# (S, P): a key; the shortest permutations; a small and a 52-card witness; scalars alone and a permutation alone; (3, 5): an odd S is
# the only way to a permutation that starts in the middle of a block on a curve that never rejects a candidate (secp256k1)
SHAPES = [(1, 0), (0, 2), (0, 1), (6, 6), (52, 52), (0, 52), (52, 0), (3, 5)]
LONG = [((1024, 1024), 5), ((1, 4096), 2)]                  # STARK only: (shape, lanes)
BAD_ARGUMENT, BAD_ENCODING, SCHNORR = -3, -1, 5
BIG = 1048576
SEARCH_BOUND = 600                                          # seeds tried for the properties below: deterministic, bounded
M_, N_ = 2, 3                                               # the table the sampler and keygen calls go through (they use only its G)


# ---------------------------------------------------------------------------------------------------------------- the stream
def stream(cv, seed, S, P):
    """-> (S scalars, permutation of length P): the definition, on the oracle's ChaCha20Rng and fr_rand"""
    rng = po.ChaCha20Rng(po.blake2s(TAG + bytes(seed)))
    scalars = [po.fr_rand(cv, rng) for _ in range(S)]
    perm = list(range(P))
    for i in range(P - 1, 0, -1):
        j = rng.next_u64() % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return scalars, perm


def trace(cv, seed, S, P):
    """what the stream of `seed` does on its way, read off the block function: which candidates are rejected, where the last accepted
    one sits, and whether the high word of some next_u64 changes j.  (A second walk over the same words, for choosing seeds only.)"""
    key = struct.unpack("<8I", po.blake2s(TAG + bytes(seed)))
    blocks = {}

    def word(i):
        if i // 16 not in blocks:
            blocks[i // 16] = po.chacha20_block(key, i // 16)
        return blocks[i // 16][i % 16]
    rejected, c = [], 0
    while len(rejected) - sum(rejected) < S:
        v = sum(word(8 * c + i) << (32 * i) for i in range(8))
        if cv.fr_shave:
            v &= (1 << (256 - cv.fr_shave)) - 1
        rejected.append(v >= cv.q)
        c += 1
    run = best = 0
    for r in rejected:
        run = run + 1 if r else 0
        best = max(best, run)
    w = 8 * c
    high = False
    for i in range(P - 1, 0, -1):
        lo, hi = word(w), word(w + 1)
        w += 2
        high |= (lo | hi << 32) % (i + 1) != lo % (i + 1)
    return dict(first_rejected=bool(rejected and rejected[0]), longest_run=best, start_mid_block=c % 2 == 1 and P > 1,
                start_at_boundary=c % 2 == 0 and c > 0 and P > 1, high_word_matters=high)


PROPERTIES = ("first_rejected", "three_rejections_in_a_row", "start_mid_block", "start_at_boundary", "high_word_matters")


def attainable(cv, S, P, prop):
    """can a seed have the property at all?  secp256k1's q is 2^256 - 2^128.., so no search finds a rejected candidate there; without
    scalars nothing is rejected and the draws start with block 0; 2^32 is a multiple of i + 1 = 2, so a high word first counts at P = 3"""
    rejects = cv.q < (1 << (256 - cv.fr_shave)) - (1 << 200)
    if prop in ("first_rejected", "three_rejections_in_a_row"):
        return S > 0 and rejects
    if prop == "start_mid_block":
        return P > 1 and S > 0 and (rejects or S % 2 == 1)
    if prop == "start_at_boundary":
        return P > 1 and S > 0 and (rejects or S % 2 == 0)
    return P >= 3


def _candidate(k):
    return hashlib.blake2s(b"sample case seed %d" % k).digest()


@functools.lru_cache(maxsize=None)
def searched_seeds(curve, S, P):
    """{property: seed}: the first of the candidate seeds 0 .. SEARCH_BOUND - 1 that has it, for every attainable property"""
    cv = po.CURVES[curve]
    want = [p for p in PROPERTIES if attainable(cv, S, P, p)]
    found = {}
    for k in range(SEARCH_BOUND):
        if len(found) == len(want):
            break
        seed = _candidate(k)
        t = trace(cv, seed, S, P)
        t["three_rejections_in_a_row"] = t["longest_run"] >= 3
        for p in want:
            if p not in found and t[p]:
                found[p] = seed
    return found


@functools.lru_cache(maxsize=None)
def seeds_for(curve, S, P, search=True):
    """257 seeds: all-zero, all-0xFF, the searched ones, then ordinary ones; a call of L lanes takes the first L"""
    special = [bytes(32), b"\xff" * 32] + (list(searched_seeds(curve, S, P).values()) if search else [])
    return tuple(special + [hashlib.blake2s(b"sample lane %d %d %d" % (S, P, i)).digest() for i in range(257 - len(special))])


@functools.lru_cache(maxsize=None)
def expected(curve, S, P, lanes, search=True):
    """the stream of the first `lanes` seeds of seeds_for, computed once and shared"""
    cv = po.CURVES[curve]
    return tuple(stream(cv, s, S, P) for s in seeds_for(curve, S, P, search)[:lanes])


def _table(eng, coracle, curve, m=M_, n=N_, keyless=False):
    gi = coracle.gen_inputs(curve, m, n, 77)
    return gi, eng.table(m, n, gi["params"], None if keyless else gi["pk"])


def _sc(v):
    return int(v).to_bytes(32, "little")


def _check_lanes(fails, tag, exp, sc, pm, S, P):
    for l, (es, ep) in enumerate(exp):
        if sc[l * S * 32:(l + 1) * S * 32] != b"".join(_sc(v) for v in es):
            fails.append("%s lane %d: scalars differ from the stream" % (tag, l))
        if list(pm[l * P:(l + 1) * P]) != ep:
            fails.append("%s lane %d: permutation differs from the stream" % (tag, l))
    return 2 * len(exp)


def run_stream(eng, coracle, curve, shape, mp):
    """one (S, P) at every lane count: scalars and permutations word for word; the searched seeds have their properties; every
    permutation is one; protocol.secret_stream agrees"""
    S, P = shape
    cv = po.CURVES[curve]
    fails, checks = [], 0
    found = searched_seeds(curve, S, P)
    for prop in PROPERTIES:
        if attainable(cv, S, P, prop) and prop not in found:
            fails.append("%s (%d, %d): no seed among %d with the property '%s'" % (curve, S, P, SEARCH_BOUND, prop))
    for prop, seed in found.items():      # the chosen seeds are what they are chosen for (a 32-bit remainder cannot pass on 'high_word_matters')
        t = trace(cv, seed, S, P)
        t["three_rejections_in_a_row"] = t["longest_run"] >= 3
        if not t[prop]:
            fails.append("%s (%d, %d): the seed chosen for '%s' does not have it" % (curve, S, P, prop))
        checks += 1
    exp = expected(curve, S, P, 257)
    for l, (es, ep) in enumerate(exp):
        if sorted(ep) != list(range(P)) or any(not 0 <= v < cv.q for v in es):
            fails.append("%s (%d, %d) lane %d: the expected stream is not %d scalars below q and a permutation" % (curve, S, P, l, S))
    seeds = seeds_for(curve, S, P)
    for l in range(0, 257, 16):
        if mp.secret_stream(curve, seeds[l], S, P) != (list(exp[l][0]), list(exp[l][1])):
            fails.append("%s (%d, %d) lane %d: protocol.secret_stream differs from the stream" % (curve, S, P, l))
        checks += 1
    gi, t = _table(eng, coracle, curve)
    for L in LANES:
        sc, pm = t.sample_secrets_batch(b"".join(seeds[:L]), S, P)
        for l in range(L):
            if sorted(pm[l * P:(l + 1) * P]) != list(range(P)):
                fails.append("%s (%d, %d) L = %d lane %d: not a permutation" % (curve, S, P, L, l))
        checks += _check_lanes(fails, "%s (%d, %d) L = %d" % (curve, S, P, L), exp[:L], sc, pm, S, P)
    t.close()
    return fails, checks


def run_long(eng, coracle, curve="stark"):
    """(1024, 1024) with 5 lanes and (1, 4096) with 2: many blocks per lane, the longest permutation"""
    fails, checks = [], 0
    gi, t = _table(eng, coracle, curve)
    for (S, P), L in LONG:
        exp = expected(curve, S, P, L, False)
        sc, pm = t.sample_secrets_batch(b"".join(seeds_for(curve, S, P, False)[:L]), S, P)
        checks += _check_lanes(fails, "%s (%d, %d) L = %d" % (curve, S, P, L), exp, sc, pm, S, P)
    t.close()
    return fails, checks


# ---------------------------------------------------------------------------------------------------------------- seeded proving
PROVE_SHAPES = {"stark": [((2, 3), 1), ((2, 3), 65), ((2, 3), 257), ((2, 26), 64)], "bn254": [((2, 4), 65)]}      # ((m, n), B)


def _decks(coracle, curve, m, n, B):
    """B decks: three distinct ones in turn (a deck is 2 N points of the oracle's making)"""
    three = [coracle.gen_inputs(curve, m, n, 300 + k)["deck"] for k in range(3)]
    return [three[b % 3] for b in range(B)]


def _keys(coracle, curve, G, B):
    """one aggregate key per proof: five distinct ones in turn"""
    five = [coracle.msm(curve, _sc(1000 + 7 * k), G) for k in range(5)]
    return [five[b % 5] for b in range(B)]


def run_seeded(eng, coracle, curve, mn, B, keyed, python_oracle=False):
    """decks, proofs and status of the seeded call equal the unseeded call's on the oracle-derived witness and the oracle's own for the
    first proofs; the verifier accepts them; the optional outputs are the stream"""
    m, n = mn
    N = m * n
    cv = po.CURVES[curve]
    fails = []
    gi, t = _table(eng, coracle, curve, m, n, keyless=keyed)
    G = gi["params"][:eng.point_bytes]
    seeds = seeds_for(curve, N, N)[:B]
    exp = expected(curve, N, N, B)
    rho = b"".join(_sc(v) for es, _ in exp for v in es)
    perms = [v for _, ep in exp for v in ep]
    decks = _decks(coracle, curve, m, n, B)
    keys = _keys(coracle, curve, G, B) if keyed else None
    tag = "%s (%d, %d) B = %d%s" % (curve, m, n, B, " keyed" if keyed else "")
    got = t.shuffle_and_remask_batch_seeded(b"".join(decks), b"".join(seeds), b"".join(keys) if keyed else None, witness=True)
    if keyed:
        ref = t.shuffle_and_remask_batch_keys(b"".join(keys), b"".join(decks), rho, perms, b"".join(seeds))
    else:
        ref = t.shuffle_and_remask_batch(b"".join(decks), rho, perms, b"".join(seeds))
    if got[2] != [0] * B or ref[2] != [0] * B:
        fails.append("%s: status %s, unseeded %s" % (tag, [v for v in got[2] if v][:4], [v for v in ref[2] if v][:4]))
    if got[0] != ref[0] or got[1] != ref[1]:
        fails.append("%s: decks or proofs differ from the unseeded call's on the stream's witness" % tag)
    if got[3] != perms or got[4] != rho:
        fails.append("%s: out_perms / out_factors are not the stream" % tag)
    plain = t.shuffle_and_remask_batch_seeded(b"".join(decks), b"".join(seeds), b"".join(keys) if keyed else None)
    if plain != got[:3]:
        fails.append("%s: the call without the optional outputs gives other bytes" % tag)
    dsz, psz = 2 * N * eng.point_bytes, t.proof_bytes
    for b in range(min(B, 2)):
        pk = keys[b] if keyed else gi["pk"]
        want = coracle.shuffle_and_remask(curve, m, n, gi["params"], pk, decks[b], rho[b * N * 32:(b + 1) * N * 32], perms[b * N:(b + 1) * N], seeds[b])
        if got[0][b * dsz:(b + 1) * dsz] != want[0] or got[1][b * psz:(b + 1) * psz] != want[1]:
            fails.append("%s proof %d: differs from the oracle's" % (tag, b))
    if python_oracle:
        with po.curve_ctx(cv):
            pts = [po.pt_from_wire(gi["params"][i * eng.point_bytes:(i + 1) * eng.point_bytes]) for i in range(n + 3)]
            pp = po.Params(cv, m, n, pts[0], pts[1:1 + n], pts[1 + n], pts[2 + n])
            pk = po.pt_from_wire(keys[0] if keyed else gi["pk"])
            shuffled, proof = po.shuffle_and_remask(pp, pk, po.deck_from_bytes(decks[0]), list(exp[0][0]), list(exp[0][1]), seeds[0])
            if po.deck_to_bytes(shuffled) != got[0][:dsz] or po.proof_to_bytes(proof) != got[1][:psz]:
                fails.append("%s proof 0: differs from the Python oracle's" % tag)
    if keyed:
        vs = t.verify_shuffle_batch_keys(b"".join(keys), b"".join(decks), got[0], got[1])
    else:
        vs = t.verify_shuffle_batch(b"".join(decks), got[0], got[1])
    if vs != [0] * B:
        fails.append("%s: the verifier says %s" % (tag, [(i, v) for i, v in enumerate(vs) if v][:4]))
    t.close()
    return fails, 6 * B


def run_seeded_dev(eng, coracle, curve, mn, B, keyed, torch, device):
    """the device-pointer form gives the bytes of the host form ("cpu": the emulator, whose device pointers are host pointers), with
    and without the optional outputs, and mp_sample_secrets_batch_dev the stream"""
    m, n = mn
    N = m * n
    fails = []
    gi, t = _table(eng, coracle, curve, m, n, keyless=keyed)
    G = gi["params"][:eng.point_bytes]
    seeds = seeds_for(curve, N, N)[:B]
    exp = expected(curve, N, N, B)
    decks = _decks(coracle, curve, m, n, B)
    keys = _keys(coracle, curve, G, B) if keyed else None
    tag = "%s (%d, %d) B = %d%s dev" % (curve, m, n, B, " keyed" if keyed else "")
    host = t.shuffle_and_remask_batch_seeded(b"".join(decks), b"".join(seeds), b"".join(keys) if keyed else None, witness=True)
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)      # noqa: E731
    raw = lambda x: bytes(x.cpu().numpy().tobytes())      # noqa: E731
    d_decks, d_seeds = dev(b"".join(decks)), dev(b"".join(seeds))
    d_keys = dev(b"".join(keys)) if keyed else None
    sync = (lambda: None) if device == "cpu" else torch.cuda.synchronize
    for with_witness in (True, False):
        od = torch.zeros(len(host[0]), dtype=torch.uint8, device=device)
        op = torch.zeros(len(host[1]), dtype=torch.uint8, device=device)
        st = torch.full((B,), 7, dtype=torch.int32, device=device)
        pm = torch.zeros(B * N, dtype=torch.int32, device=device)
        rho = torch.zeros(B * N * 32, dtype=torch.uint8, device=device)
        sync()
        t.shuffle_and_remask_batch_seeded_dev(B, d_keys.data_ptr() if keyed else None, d_decks.data_ptr(), d_seeds.data_ptr(), od.data_ptr(),
                                              op.data_ptr(), st.data_ptr(), pm.data_ptr() if with_witness else None,
                                              rho.data_ptr() if with_witness else None)
        eng.sync()
        if (raw(od), raw(op), st.cpu().tolist()) != host[:3]:
            fails.append("%s (optional outputs: %s): differs from the host form" % (tag, with_witness))
        if with_witness and (pm.cpu().tolist() != host[3] or raw(rho) != host[4]):
            fails.append("%s: d_out_perms / d_out_factors differ from the host form's" % tag)
    sc = torch.zeros(B * N * 32, dtype=torch.uint8, device=device)
    pm = torch.zeros(B * N, dtype=torch.int32, device=device)
    sync()
    t.sample_secrets_batch_dev(B, d_seeds.data_ptr(), N, N, sc.data_ptr(), pm.data_ptr())
    eng.sync()
    _check_lanes(fails, tag + " sampler", exp, raw(sc), pm.cpu().tolist(), N, N)
    t.close()
    return fails, 5 * B


# ---------------------------------------------------------------------------------------------------------------- key generation
KEYGEN = (1, 64, 65, 257)


def run_keygen(eng, coracle, curve, K):
    """sk and pk are the oracle's; the proofs are mp_sigma_prove_batch's and (first lanes) the oracle's; without fs_init the same keys;
    mp_aggregate_keys_batch seats the players; two players who swap their keys are refused with 5"""
    cv = po.CURVES[curve]
    fails = []
    gi, t = _table(eng, coracle, curve)
    pb = eng.point_bytes
    G = gi["params"][:pb]
    seeds = seeds_for(curve, 1, 0)[:K]
    sks = [es[0] for es, _ in expected(curve, 1, 0, K)]
    pks = [coracle.msm(curve, _sc(x), G) for x in sks]
    infos = [b"player %d" % l + b"!" * (l % 5) for l in range(K)]
    fs_raw = [po.KEY_OWN_RNG_SEED + i for i in infos]
    fs = b"".join(hashlib.blake2s(r).digest() for r in fs_raw)
    tag = "%s keygen K = %d" % (curve, K)
    pk, sk, prf, st = t.keygen_batch(b"".join(seeds), fs)
    if st != [0] * K:
        fails.append("%s: status %s" % (tag, [v for v in st if v][:4]))
    if sk != b"".join(_sc(x) for x in sks):
        fails.append("%s: secret keys differ from the stream" % tag)
    if pk != b"".join(pks):
        fails.append("%s: public keys differ from the oracle's sk G" % tag)
    if pk != t.msm(K, 1, sk, G * K):
        fails.append("%s: public keys differ from mp_msm's" % tag)
    want, wst = t.sigma_prove_batch(1, G * K, b"".join(pks), b"".join(_sc(x) for x in sks), fs, b"".join(seeds))
    if prf != want or wst != [0] * K:
        fails.append("%s: proofs differ from mp_sigma_prove_batch's" % tag)
    psz = pb + 32
    for l in range(min(K, 3)):
        if prf[l * psz:(l + 1) * psz] != coracle.sigma_prove(curve, 1, G, pks[l], _sc(sks[l]), fs_raw[l], seeds[l]):
            fails.append("%s lane %d: proof differs from the oracle's" % (tag, l))
    if K == 1:      # the Python oracle's keygen and proof, once
        with po.curve_ctx(cv):
            pts = [po.pt_from_wire(gi["params"][i * pb:(i + 1) * pb]) for i in range(N_ + 3)]
            pp = po.Params(cv, M_, N_, pts[0], pts[1:1 + N_], pts[1 + N_], pts[2 + N_])
            ppk, psk = po.player_keygen(pp, po.ChaCha20Rng(po.blake2s(TAG + seeds[0])))
            proof = po.sigma_prove(cv, [pp.G], [ppk], psk, fs_raw[0], seeds[0])
            if (po.pt_wire(ppk), _sc(psk), po.sigma_proof_bytes(proof)) != (pk[:pb], sk[:32], prf[:psz]):
                fails.append("%s: differs from the Python oracle's player_keygen / sigma_prove" % tag)
    if t.keygen_batch(b"".join(seeds))[:2] != (pk, sk):
        fails.append("%s: without fs_init the keys differ" % tag)
    keys, ps, ts = t.aggregate_keys_batch(K, 1, pk, prf, fs)
    if ps != [0] * K or ts != [0] * K or keys != pk:
        fails.append("%s: mp_aggregate_keys_batch refuses the generated players (%s)" % (tag, [(i, v) for i, v in enumerate(ps) if v][:4]))
    if K >= 2:
        a, b = 0, K - 1
        sw = [pks[b] if l == a else pks[a] if l == b else pks[l] for l in range(K)]
        _, ps, ts = t.aggregate_keys_batch(K, 1, b"".join(sw), prf, fs)
        if ps != [SCHNORR if l in (a, b) else 0 for l in range(K)] or ts != ps or eng.check_name(SCHNORR) != "Schnorr Identification":
            fails.append("%s: two swapped keys give %s" % (tag, [(i, v) for i, v in enumerate(ps) if v][:4]))
    t.close()
    return fails, 8 * K


# ---------------------------------------------------------------------------------------------------------------- refusals, threads
def run_refusals(eng, coracle, curve):
    """shapes outside the limits and null pointers are MP_ERR_BAD_ARGUMENT for the call; a bad deck point in one seeded proof is that
    proof's status alone"""
    fails, checks = [], 0
    gi, t = _table(eng, coracle, curve)
    lib, h = t.lib, t.h
    buf = (ctypes.c_uint8 * 4096)()
    for name, (L, S, P) in (("S = P = 0", (1, 0, 0)), ("S = 4097", (1, 4097, 0)), ("P = 4097", (1, 0, 4097)), ("S = 4097 and P = 1", (1, 4097, 1)),
                            ("L = 0", (0, 1, 1)), ("L over the limit", (BIG + 1, 1, 0))):
        for fn in (lib.mp_sample_secrets_batch, lib.mp_sample_secrets_batch_dev):
            rc = fn(h, L, buf, S, P, buf, buf)
            if rc != BAD_ARGUMENT:
                fails.append("%s mp_sample_secrets_batch[_dev], %s: %d, expected %d" % (curve, name, rc, BAD_ARGUMENT))
            checks += 1
    for name, args in (("null seeds", (1, None, 1, 1, buf, buf)), ("null scalars with S = 1", (1, buf, 1, 0, None, buf)),
                       ("null permutations with P = 2", (1, buf, 0, 2, buf, None))):
        for fn in (lib.mp_sample_secrets_batch, lib.mp_sample_secrets_batch_dev):
            if fn(h, *args) != BAD_ARGUMENT:
                fails.append("%s mp_sample_secrets_batch[_dev], %s: not refused" % (curve, name))
            checks += 1
    for name, rc in (("K = 0", lib.mp_keygen_batch(h, 0, buf, buf, buf, buf, buf, buf)),
                     ("K over the limit", lib.mp_keygen_batch(h, BIG + 1, buf, buf, buf, buf, buf, buf)),
                     ("null seeds", lib.mp_keygen_batch(h, 1, None, buf, buf, buf, buf, buf)),
                     ("fs_init without out_proofs", lib.mp_keygen_batch(h, 1, buf, buf, buf, buf, None, buf)),
                     ("seeded: B = 0", lib.mp_shuffle_and_remask_batch_seeded(h, 0, None, buf, buf, buf, buf, buf, None, None)),
                     ("seeded: null seeds", lib.mp_shuffle_and_remask_batch_seeded(h, 1, None, buf, None, buf, buf, buf, None, None)),
                     ("seeded dev: B = 0", lib.mp_shuffle_and_remask_batch_seeded_dev(h, 0, None, buf, buf, buf, buf, buf, None, None)),
                     ("seeded dev: null decks", lib.mp_shuffle_and_remask_batch_seeded_dev(h, 1, None, None, buf, buf, buf, buf, None, None))):
        if rc != BAD_ARGUMENT:
            fails.append("%s %s: %d, expected %d" % (curve, name, rc, BAD_ARGUMENT))
        checks += 1
    # a keyless table needs keys
    gk, tk = _table(eng, coracle, curve, keyless=True)
    if lib.mp_shuffle_and_remask_batch_seeded(tk.h, 1, None, buf, buf, buf, buf, buf, None, None) != BAD_ARGUMENT:
        fails.append("%s: a seeded call without keys on a keyless table is not refused" % curve)
    tk.close()
    # one bad deck point: that proof's status alone, the others as before
    N, B = M_ * N_, 5
    pb = eng.point_bytes
    seeds = seeds_for(curve, N, N)[:B]
    decks = _decks(coracle, curve, M_, N_, B)
    good = t.shuffle_and_remask_batch_seeded(b"".join(decks), b"".join(seeds))
    bad = list(decks)
    bad[2] = bad[2][:3 * pb] + bytes([bad[2][3 * pb] ^ 1]) + bad[2][3 * pb + 1:]      # one bit of an x coordinate: off the curve
    if coracle.on_curve(curve, bad[2][3 * pb:4 * pb]):
        fails.append("%s: the damaged point is still on the curve" % curve)
    got = t.shuffle_and_remask_batch_seeded(b"".join(bad), b"".join(seeds))
    dsz, psz = 2 * N * pb, t.proof_bytes
    if got[2] != [0, 0, BAD_ENCODING, 0, 0] or good[2] != [0] * B:
        fails.append("%s: status %s with a bad point in proof 2" % (curve, got[2]))
    for b in (0, 1, 3, 4):
        if got[0][b * dsz:(b + 1) * dsz] != good[0][b * dsz:(b + 1) * dsz] or got[1][b * psz:(b + 1) * psz] != good[1][b * psz:(b + 1) * psz]:
            fails.append("%s: proof %d changes with a bad point in proof 2" % (curve, b))
    t.close()
    return fails, checks + 10


def run_threads(eng, coracle, curve, threading):
    """two host threads sample on ONE table, four calls each: the bytes are the single-threaded ones, which are the stream"""
    fails = []
    gi, t = _table(eng, coracle, curve)
    jobs = [((6, 6), 65), ((52, 0), 64)]
    want = []
    for (S, P), L in jobs:
        exp = expected(curve, S, P, L)
        want.append((b"".join(_sc(v) for es, _ in exp for v in es), [v for _, ep in exp for v in ep]))
    single = [t.sample_secrets_batch(b"".join(seeds_for(curve, S, P)[:L]), S, P) for (S, P), L in jobs]
    got, errors = [[], []], []

    def work(k):
        try:
            (S, P), L = jobs[k]
            for _ in range(4):
                got[k].append(t.sample_secrets_batch(b"".join(seeds_for(curve, S, P)[:L]), S, P))
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
            fails.append("%s thread %d: the bytes differ from the single-threaded call's or from the stream" % (curve, k))
    t.close()
    return fails, 10
