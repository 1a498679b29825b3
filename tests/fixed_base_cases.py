"""Cases and checks for the tables and kernels BEHIND the digits of tests/digit_cases.py, through the C ABI: every entry class of the
fixed-base tables (k_fb_windows / k_fb_fill / k_fb_widen, read by k_fixed_msm and k_remask), the 8-bit tables of a key set and the signed
5-bit tables of a per-proof key (k_key_windows, the keyed branches of k_remask), and the recoders inside the MSM kernels (k_recode +
k_var_msm, k_bucket_recode + the bucket kernels) on the scalar families of digit_cases.  Shared by tests/test_digit_emu.py (the kernel
bodies under the development emulator, CPU) and tests/test_gpu_digit.py (the gfx950 build): exact equality with the C++ oracle
(coracle.commit, coracle.remask_deck, coracle.msm, coracle.shuffle_and_remask), byte for byte.

Every run_* function returns (failure messages, number of checks made); the tests assert that the list is empty."""
import random
import time

import digit_cases as dc
import mp_oracle as mo
from shuffle_edge_cases import _Dev, _pmap

M_, N_ = 2, 2                       # the fewest bases a table can have: ck_0, ck_1, H, G, pk, the generator, the key sum
N_RANDOM_DIGITS = 16                # per window
K_MSM = 96                          # terms of one MSM (as prim_cases.run_msm_exceptional)

# what the emulator runs: the 8-bit tables.  The 16-bit tables take 7 x 16 x 65 535 entries through k_fb_widen and k_normalize on the CPU: 10 s
# (STARK) to 16 s (BLS12-377) per table where test_bucket_msm_edge_scalars_under_emulation takes 8 s, so they are gfx950 only, like the
# 20- and 21-bit ones (16 and 32 times the entries).  Every MSM path runs under the emulator too
EMU_FB_BITS = (8,)
GPU_FB_BITS = {"stark": (8, 16, 20, 21), "bn254": (8, 16), "secp256k1": (8, 16, 20, 21), "bls12_377": (8, 16)}
MSM_PATHS = ((0, 0), (16, 0), (16, 8), (16, 9), (16, 10), (16, 11), (16, 12), (16, 13), (16, 14))      # (bucket_min, bucket bits): 0 = Straus
EMU_MSM_PATHS = MSM_PATHS


def path_id(path):
    return "straus" if path[0] == 0 else ("bucket-by-size" if path[1] == 0 else "bucket-%d" % path[1])


def _sc(v):
    return int(v).to_bytes(32, "little")


# ---- what the four orders make of the window geometry ---------------------------------------------------------------------------------
def top_digit(q, bits):
    """the largest digit of the top fixed-base window"""
    return (q - 1) >> (bits * (dc.windows(q, dc.KIND_FIXED, bits) - 1))


def check_order_table():
    """why the cases are what they are: only secp256k1 fills its top fixed-base window (8 and 16 bits); 21-bit windows save a window on
    STARK and not on secp256k1; on both a 20- and a 21-bit window straddles into the last word, and the top one of secp256k1 runs past it"""
    fails, n = [], 0
    for curve in dc.CURVES:
        q = dc.order(curve)
        for bits in dc.FB_BITS:
            full = top_digit(q, bits) == (1 << bits) - 1
            if full != (curve == "secp256k1" and bits in (8, 16)):
                fails.append("%s %d-bit: the top window's largest digit is %d" % (curve, bits, top_digit(q, bits)))
            n += 1
    ws = {c: [dc.windows(dc.order(c), dc.KIND_FIXED, b) for b in (20, 21)] for c in dc.CURVES}
    if ws["stark"][0] != ws["stark"][1] + 1 or ws["secp256k1"][0] != ws["secp256k1"][1]:
        fails.append("windows of 20 / 21 bits: %s" % ws)
    for curve in ("secp256k1", "stark"):
        for bits in (20, 21):
            starts = [bits * w for w in range(dc.windows(dc.order(curve), dc.KIND_FIXED, bits))]
            if not any(b // 32 == 6 and b % 32 + bits > 32 for b in starts):
                fails.append("%s %d-bit: no window straddles into the last word" % (curve, bits))
            if curve == "secp256k1" and starts[-1] + bits <= 256:
                fails.append("%s %d-bit: the top window ends inside the last word" % (curve, bits))
            n += 1
    return fails, n + 1


# ---- fixed-base entries ----------------------------------------------------------------------------------------------------------------
def fixed_scalars(q, bits):
    """-> [(window, digit, scalar)]: per window the digits {1, 2, 2^h - 1, 2^h, 2^h + 1, 2^bits - 2^h, 2^bits - 2, 2^bits - 1} (h: the
    narrow width the wide entry is put together from) and seeded random ones, clipped to the window's largest digit that keeps the scalar
    below q, and that digit itself; then q - 1 and the all-ones pattern truncated below q (window -1)"""
    h, full = dc.narrow_bits(bits), 1 << bits
    rng = random.Random(q % 1000003 + bits)
    out, seen = [], set()
    for w in range(dc.windows(q, dc.KIND_FIXED, bits)):
        dmax = min(full - 1, (q - 1) >> (w * bits))
        ds = [1, 2, (1 << h) - 1, 1 << h, (1 << h) + 1, full - (1 << h), full - 2, full - 1]
        ds += [rng.randrange(1, full) for _ in range(N_RANDOM_DIGITS)] + [dmax]
        for d in ds:
            d = min(d, dmax)
            if (w, d) not in seen:
                seen.add((w, d))
                out.append((w, d, d << (w * bits)))
    out += [(-1, 0, q - 1), (-1, 0, (1 << (q.bit_length() - 1)) - 1)]
    assert all(0 < s < q for _, _, s in out)
    return out


class FixedTable:
    """a table of (2, 2) with `bits`-wide fixed-base windows and the seconds its construction took"""

    def __init__(self, eng, coracle, curve, bits):
        self.eng, self.co, self.curve, self.bits = eng, coracle, curve, bits
        self.gi = coracle.gen_inputs(curve, M_, N_, 4100 + bits)
        self.params, self.pk = self.gi["params"], self.gi["pk"]
        self.pb = eng.point_bytes
        t0 = time.time()
        self.t = eng.table(M_, N_, self.params, self.pk, fb_bits=bits)
        eng.sync()
        self.build_seconds = time.time() - t0
        print("table build: %s (%d, %d) %d-bit windows: %.2f s" % (curve, M_, N_, bits, self.build_seconds))
        assert self.t.fb_bits == bits

    def close(self):
        self.t.close()


def run_fixed_entries(ft):
    """every scalar d 2^(w bits) as the only non-zero value of a commitment at position 0 and at position 1 (bases ck_0, ck_1), as its
    blinder alone (base H), and as the factor of a re-encryption of a card at infinity (bases G and pk)"""
    co, curve, pb = ft.co, ft.curve, ft.pb
    q = dc.order(curve)
    cases = fixed_scalars(q, ft.bits)
    zero = _sc(0)
    rows = []
    for w, d, s in cases:
        rows += [(_sc(s) + zero, zero, "ck_0"), (zero + _sc(s), zero, "ck_1"), (zero + zero, _sc(s), "H")]
    got = ft.t.commit_batch(len(rows), N_, b"".join(v for v, _, _ in rows), b"".join(r for _, r, _ in rows))
    want = _pmap(lambda row: co.commit(curve, N_, ft.params, row[0], row[1]), rows)
    fails = []
    inf = bytes(pb)
    for i, (v, r, base) in enumerate(rows):
        w, d, s = cases[i // 3]
        if want[i] == inf:
            fails.append("%s %d-bit: the oracle's %#x %s is the point at infinity" % (curve, ft.bits, s, base))
        if got[pb * i:pb * (i + 1)] != want[i]:
            fails.append("%s %d-bit tables: window %d digit %#x on base %s (scalar %#x): differs from the oracle's commitment" %
                         (curve, ft.bits, w, d, base, s))
    cb = 2 * pb
    factors = b"".join(_sc(s) for _, _, s in cases)
    cards = bytes(cb * len(cases))
    got = ft.t.remask_batch(cards, factors)
    want = co.remask_deck(curve, ft.params[:pb], ft.pk, cards, factors)
    for i, (w, d, s) in enumerate(cases):
        for half, base in ((0, "G"), (1, "pk")):
            o = cb * i + pb * half
            if got[o:o + pb] != want[o:o + pb]:
                fails.append("%s %d-bit tables: window %d digit %#x on base %s (scalar %#x): differs from the oracle's re-encryption" %
                             (curve, ft.bits, w, d, base, s))
    return fails[:40], 5 * len(cases)


# ---- the recoders inside the MSM kernels -------------------------------------------------------------------------------------------------
_WANT = {}


def _msm_want(co, curve, scb, ptb):
    key = (curve, scb, ptb)
    if key not in _WANT:
        n = len(scb) // (32 * K_MSM)
        _WANT[key] = _pmap(lambda j: co.msm(curve, scb[32 * K_MSM * j:32 * K_MSM * (j + 1)], ptb), range(n))
    return _WANT[key]


def run_msm_families(eng, coracle, curve, path):
    """the scalar families of digit_cases for the path's recoder, each spread over MSMs of 96 terms on 96 different points (the last one
    padded with zeros), all the MSMs of a family in one mp_msm call; path = (bucket_min, bucket bits), (0, 0): Straus"""
    bucket_min, bits = path
    q, pb = dc.order(curve), eng.point_bytes
    kind, width = (dc.KIND_STRAUS, dc.STRAUS_BITS) if bucket_min == 0 else (dc.KIND_BUCKET, bits or 8)      # (by size: 8 bits below 6 000 terms)
    gi = coracle.gen_inputs(curve, 2, 3, 5)
    t = eng.table(2, 3, gi["params"], gi["pk"])
    ptb = eng.setup(2, K_MSM - 3, bytes([9] * 32))
    assert len(ptb) == pb * K_MSM
    fails, n = [], 0
    t.set_bucket_min(bucket_min)
    t.set_bucket_bits(bits)
    fams = dc.families(q, kind, width)
    if (curve, kind, width) == ("secp256k1", dc.KIND_BUCKET, 8) and not any((q - 1) // 2 in vals for _, vals in fams):
        fails.append("secp256k1, 8-bit windows: (q - 1) / 2 -- the last bucket of the top window -- is not among the scalars")
    eng.profile_enable(True)
    for name, vals in fams:
        vals = list(vals) + [0] * (-len(vals) % K_MSM)
        scb = b"".join(_sc(v) for v in vals)
        n_msm = len(vals) // K_MSM
        want = _msm_want(coracle, curve, scb, ptb)
        got = t.msm(n_msm, K_MSM, scb, ptb * n_msm)
        for j in range(n_msm):
            if got[pb * j:pb * (j + 1)] != want[j]:
                fails.append("%s %s [%s] MSM %d of %d (scalars %#x ...): differs from the oracle's" %
                             (curve, path_id(path), name, j, n_msm, vals[K_MSM * j]))
        n += n_msm
    rep = eng.profile_report()
    eng.profile_enable(False)
    ran_bucket = "k_bucket_recode" in rep
    if ran_bucket != (bucket_min != 0) or ("k_recode" in rep) == ran_bucket:
        fails.append("%s %s: the kernels that ran are %s" % (curve, path_id(path), sorted(rep)))
    t.set_bucket_bits(0)
    t.close()
    return fails[:40], n


# ---- key sets (8-bit tables per key) and per-proof keys (signed 5-bit digits of rho over k_key_windows) ---------------------------------
KEYED_SHAPE = (2, 3)


def keyed_factors(q):
    """the masking factors of the keyed proofs: the per-window digit set of the 8-bit tables (what a key set indexes with) and the Straus
    boundary scalars (what a per-proof key's signed windows are indexed with)"""
    vals = [s for _, _, s in fixed_scalars(q, 8)]
    for name, fam in dc.families(q, dc.KIND_STRAUS, dc.STRAUS_BITS):
        if name in ("one boundary digit per window", "every window on a boundary"):
            vals += fam
    return vals


def run_keyed(eng, coracle, curve, torch, device):
    """proofs of (2, 3) with the identity permutation whose masking factors run through keyed_factors, under a generic key, G and -G in
    turn: mp_shuffle_and_remask_batch_keys (explicit keys) and the key-set form give the oracle's shuffled deck and proof under that key"""
    m, n = KEYED_SHAPE
    N = m * n
    q, pb = dc.order(curve), eng.point_bytes
    gi = coracle.gen_inputs(curve, m, n, 4300)
    params, deck = gi["params"], gi["deck"]
    G = params[:pb]
    y = int.from_bytes(G[pb // 2:], "little")
    minus_G = G[:pb // 2] + (mo.CURVES[curve].p - y).to_bytes(pb // 2, "little")
    key_set = [gi["pk"], G, minus_G]
    vals = keyed_factors(q)
    vals += [1] * (-len(vals) % N)
    B = len(vals) // N
    rho = [b"".join(_sc(v) for v in vals[N * b:N * (b + 1)]) for b in range(B)]
    kidx = [b % 3 for b in range(B)]
    seeds = [bytes([b & 0xFF, b >> 8]) + gi["prover_seed"][2:] for b in range(B)]
    perm = list(range(N))
    want = _pmap(lambda b: coracle.shuffle_and_remask(curve, m, n, params, key_set[kidx[b]], deck, rho[b], perm, seeds[b]), range(B))
    dsz, psz = len(deck), coracle.proof_size(m, n, curve)
    t = eng.table(m, n, params, None)
    ks = t.keyset(b"".join(key_set))
    fails = []

    def compare(form, d, p, st):
        for b in range(B):
            if st[b] != 0 or d[dsz * b:dsz * (b + 1)] != want[b][0] or p[psz * b:psz * (b + 1)] != want[b][1]:
                fails.append("%s %s: proof %d (key %d, factors %s): status %d, deck %s, proof %s" %
                             (curve, form, b, kidx[b], " ".join("%#x" % v for v in vals[N * b:N * (b + 1)]), st[b],
                              "equal" if d[dsz * b:dsz * (b + 1)] == want[b][0] else "differs",
                              "equal" if p[psz * b:psz * (b + 1)] == want[b][1] else "differs"))

    keys = b"".join(key_set[k] for k in kidx)
    compare("explicit keys", *t.shuffle_and_remask_batch_keys(keys, deck * B, b"".join(rho), perm * B, b"".join(seeds)))
    dv = _Dev(torch, device)
    d_idx, d_perm = dv.ints(kidx), dv.ints(perm * B)
    d_decks, d_rho, d_seeds = dv.bytes(deck * B), dv.bytes(b"".join(rho)), dv.bytes(b"".join(seeds))
    od, op, st = dv.bytes(bytes(B * dsz)), dv.bytes(bytes(B * psz)), dv.status(B)
    dv.sync()
    t.shuffle_and_remask_batch_keyset_dev(ks, B, d_idx.data_ptr(), d_decks.data_ptr(), d_rho.data_ptr(), d_perm.data_ptr(), d_seeds.data_ptr(),
                                          od.data_ptr(), op.data_ptr(), st.data_ptr())
    eng.sync()
    compare("key set", bytes(od.cpu().numpy().tobytes()), bytes(op.cpu().numpy().tobytes()), st.cpu().tolist())
    ks.close()
    t.close()
    return fails[:20], 2 * B
