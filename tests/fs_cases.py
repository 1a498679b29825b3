"""Cases, references and checks for the Fiat-Shamir probe (tools/fscheck/fs_check.hip): the device BLAKE2s over the staging buffer (one
lane and four), the four-lane absorb, the ChaCha20 block, `Fr::rand`, the chain / group weights, the lane digests of the sigma screen and
the weights of the merged equation, compared with hashlib and the Python oracle.  Shared by tests/test_fs_emu.py (the probe built against
the development emulator, CPU) and tests/test_gpu_fs.py (the gfx950 build) -- same cases, same expectations, exact equality.

References: BLAKE2s is hashlib.blake2s(digest_size=32) on the unpadded message; ChaCha20 is mp_oracle.chacha20_block (pinned by
tests/golden/fs_kats.json).  The weight tables need ~10^6 blocks per curve, so `chacha_blocks` evaluates the same block function on numpy
arrays; `check_chacha_reference` (run by both test files) holds it to mp_oracle.chacha20_block word for word.

Every run_* function returns (failure messages, number of comparisons); the tests assert that the first is empty."""
import ctypes
import functools
import hashlib
import os
import random
import subprocess
from fractions import Fraction

import numpy as np

import mp_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tools", "fscheck")
GPU_LIB = os.path.join(PROBE_DIR, "libfscheck.so")
EMU_LIB = os.path.join(PROBE_DIR, "libfscheck_emu.so")

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
LPPS = [4, 8, 16, 32, 64]
NEXT_N, TRY_N = 48, 96                      # fs_check.hip
CW_BLOCK = 64                               # kernels_proto.hpp
PAT_NAMES = ["bytes", "point65", "point97", "words-after-bytes", "pieces"]
FILL = 0xA5C3F00F                           # pattern of the output buffers a kernel must overwrite
M32 = 0xFFFFFFFF


def H(data):
    return hashlib.blake2s(bytes(data), digest_size=32).digest()


def words(b):
    return np.frombuffer(bytes(b), dtype="<u4").astype(np.uint32)


def le256(v):
    return int(v).to_bytes(32, "little")


def _not_pow2(v):
    while v & (v - 1) == 0:
        v += 1
    return v


# ---- the probe -----------------------------------------------------------------------------------------------------------------------
def build_emu_probe():
    """the probe against the development emulator (kernel bodies as CPU loops): the recipe of prim_cases.build_emu_probe"""
    src = os.path.join(PROBE_DIR, "fs_check.hip")
    csrc = os.path.join(ROOT, "mental-poker_amd", "csrc")
    emu = os.path.join(ROOT, "tools", "hostemu")
    deps = [src, os.path.join(emu, "rt.hpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(EMU_LIB) or os.path.getmtime(EMU_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-x", "c++", "-include", os.path.join(emu, "rt.hpp"),
                               "-I" + emu, "-I" + csrc, src, "-o", EMU_LIB])
    return EMU_LIB


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


class Probe:
    def __init__(self, path):
        if not os.path.exists(path):
            raise ImportError("%s is not built" % path)
        self.lib = lib = ctypes.CDLL(path)
        u, vp = ctypes.c_uint32, ctypes.c_void_p
        lib.fc_rt_name.restype = ctypes.c_char_p
        lib.fc_vc_count.restype = u
        lib.fc_verify_lay_mr.restype = u
        lib.fc_verify_lay_mr.argtypes = [u, u]
        lib.fc_blake2s.argtypes = [ctypes.c_int, u, u, u, vp, vp, vp, vp]
        lib.fc_chacha.argtypes = [u, vp, vp, vp]
        for c in CURVES:
            getattr(lib, "fc_error_" + c).restype = ctypes.c_char_p
            getattr(lib, "fc_frstream_" + c).argtypes = [u, vp, vp, vp, vp]
            getattr(lib, "fc_fsq_absorb_" + c).argtypes = [u, u, u, u, u, vp, vp, vp, vp]
            getattr(lib, "fc_chain_weights_" + c).argtypes = [u, u, u, u, vp, vp, vp]
            getattr(lib, "fc_screen_digest_" + c).argtypes = [u, u, u, u, u, vp, vp, vp, vp, vp]
            getattr(lib, "fc_merge_weights_" + c).argtypes = [ctypes.c_int, u, u, u, u, u, vp, vp, vp, vp]
        self.rt_name = lib.fc_rt_name().decode()
        self.vc_count = lib.fc_vc_count()

    def _chk(self, rc, curve="stark"):
        if rc != 0:
            raise RuntimeError(getattr(self.lib, "fc_error_" + curve)().decode())

    def blake2s(self, mode, stride, maxlen, data, lens, pats):
        n = len(pats)
        out = np.zeros((n, 2, 4 if mode else 1, 8), np.uint32)
        self._chk(self.lib.fc_blake2s(mode, n, stride, maxlen, _p(data), _p(lens), _p(pats), _p(out)))
        return out

    def chacha(self, keys, ctr):
        out = np.zeros((len(keys), 16), np.uint32)
        self._chk(self.lib.fc_chacha(len(keys), _p(keys), _p(ctr), _p(out)))
        return out

    def frstream(self, curve, keys):
        n = len(keys)
        nxt, flag, val = np.zeros((n, NEXT_N, 8), np.uint32), np.zeros((n, TRY_N), np.uint32), np.zeros((n, TRY_N, 8), np.uint32)
        self._chk(getattr(self.lib, "fc_frstream_" + curve)(n, _p(keys), _p(nxt), _p(flag), _p(val)), curve)
        return nxt, flag, val

    def fsq_absorb(self, curve, lpp, Bpad, pts, tail, seed_in):
        B, npts = pts.shape[0], pts.shape[1]
        out = np.zeros((B, 2, 8), np.uint32)
        self._chk(getattr(self.lib, "fc_fsq_absorb_" + curve)(B, lpp, npts, tail.shape[1], Bpad, _p(pts), _p(tail), _p(seed_in), _p(out)), curve)
        return out

    def chain_weights(self, curve, T, L, Tpad, Bpad, seed):
        nb = (L + CW_BLOCK - 1) // CW_BLOCK
        CW, dig = np.full((L, Tpad, 8), FILL, np.uint32), np.zeros((nb, 8, Tpad), np.uint32)
        self._chk(getattr(self.lib, "fc_chain_weights_" + curve)(T, L, Tpad, Bpad, _p(seed), _p(CW), _p(dig)), curve)
        return CW, dig

    def screen_digest(self, curve, B, g, nw, Bpad, Tpad, seed, S):
        T, L = (B + g - 1) // g, g * nw
        nb = (L + CW_BLOCK - 1) // CW_BLOCK
        out, CW, dig = np.full((8, L * T), FILL, np.uint32), np.full((L, Tpad, 8), FILL, np.uint32), np.zeros((nb, 8, Tpad), np.uint32)
        self._chk(getattr(self.lib, "fc_screen_digest_" + curve)(B, g, nw, Bpad, Tpad, _p(seed), _p(S), _p(out), _p(CW), _p(dig)), curve)
        return out, CW, dig

    def merge_weights(self, curve, mode, m, n, lpp, Bpad, scal, seed_in):
        B = scal.shape[1]
        mr, seed = np.zeros((B, self.vc_count, 8), np.uint32), np.zeros((B, 8), np.uint32)
        self._chk(getattr(self.lib, "fc_merge_weights_" + curve)(mode, B, m, n, lpp, Bpad, _p(scal), _p(seed_in), _p(mr), _p(seed)), curve)
        return mr, seed


# ---- ChaCha20 and Fr::rand on arrays ----------------------------------------------------------------------------------------------------
def chacha_blocks(keys, counters):
    """mp_oracle.chacha20_block for keys [n][8] and counters [n] at once -> [n][16]"""
    keys = np.asarray(keys, np.uint32)
    counters = np.asarray(counters, np.uint64)
    n = len(keys)
    st = np.empty((16, n), np.uint32)
    for i, c in enumerate((0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)):
        st[i] = c
    st[4:12] = keys.T
    st[12] = (counters & np.uint64(M32)).astype(np.uint32)
    st[13] = (counters >> np.uint64(32)).astype(np.uint32)
    st[14] = 0
    st[15] = 0
    x = st.copy()

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    x += st
    return np.ascontiguousarray(x.T)


EDGE_COUNTERS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1]


def _chacha_keys():
    rng = random.Random(20)
    keys = [[rng.getrandbits(32) for _ in range(8)] for _ in range(10)] + [[0] * 8, [M32] * 8]
    return [(k, c) for k in keys for c in EDGE_COUNTERS]


def check_chacha_reference():
    """the array form above against mp_oracle.chacha20_block: the edge counters and 200 random (key, counter) pairs"""
    rng = random.Random(21)
    kc = _chacha_keys() + [([rng.getrandbits(32) for _ in range(8)], rng.getrandbits(rng.choice((6, 31, 33, 64)))) for _ in range(200)]
    got = chacha_blocks([k for k, _ in kc], [c for _, c in kc])
    fails = ["chacha_blocks differs from mp_oracle.chacha20_block: key %s counter %d" % (k, c)
             for (k, c), g in zip(kc, got) if list(map(int, g)) != mo.chacha20_block(k, c)]
    return fails, len(kc)


def candidates(curve, keys, nblk):
    """the first 2 nblk candidates of Fr::rand on ChaCha20(key), per key: 8 consecutive stream words each (two per block, limb 0 first),
    bits from BITS up cleared -> (values [n][2 nblk][8], accepted [n][2 nblk]: candidate < q)"""
    q = mo.CURVES[curve].q
    bits = q.bit_length()
    keys = np.asarray(keys, np.uint32).reshape(-1, 8)
    n = len(keys)
    blocks = chacha_blocks(np.repeat(keys, nblk, axis=0), np.tile(np.arange(nblk, dtype=np.uint64), n))
    c = blocks.reshape(n, 2 * nblk, 8).copy()
    if bits < 256:
        c[..., 7] &= np.uint32(M32 >> (256 - bits))
    lt, eq = np.zeros(c.shape[:2], bool), np.ones(c.shape[:2], bool)
    for i in range(7, -1, -1):
        qi = np.uint32((q >> (32 * i)) & M32)
        lt |= eq & (c[..., i] < qi)
        eq &= c[..., i] == qi
    return c, lt


def accept_rate(curve):
    q = mo.CURVES[curve].q
    return Fraction(q, 1 << q.bit_length())


def fr_draws(curve, keys, count):
    """the first `count` accepted candidates per key, as the 8 stored words (the raw candidate: no Montgomery conversion) -> [n][count][8]"""
    keys = np.asarray(keys, np.uint32).reshape(-1, 8)
    nblk = int(count / (2 * float(accept_rate(curve))) * 1.3) + 12
    while True:
        c, acc = candidates(curve, keys, nblk)
        if acc.sum(axis=1).min() >= count:
            break
        nblk *= 2
    order = np.argsort(~acc, axis=1, kind="stable")[:, :count]
    return np.take_along_axis(c, order[:, :, None], axis=1)


def to_int(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def mont_words(curve, z):
    """the memory format of a scalar: z 2^256 mod q as 8 words"""
    q = mo.CURVES[curve].q
    return words(le256(z % q * (1 << 256) % q))


def scalar_edges(curve):
    q = mo.CURVES[curve].q
    rng = random.Random(q % 1000003)
    return [0, 1, q - 1, 2, q - 2, (q - 1) // 2, (q + 1) // 2, M32, 1 << 32, (1 << 64) - 1, 1 << 128, (1 << (q.bit_length() - 1)) - 1,
            1 << (q.bit_length() - 1)] + [rng.randrange(q) for _ in range(19)]


def _rand_words(rng, *shape):
    n = int(np.prod(shape))
    return np.frombuffer(rng.randbytes(4 * n), dtype="<u4").astype(np.uint32).reshape(shape)


# ---- BLAKE2s over the staging buffer ----------------------------------------------------------------------------------------------------
B2S_LENGTHS = list(range(261)) + [64 * k + d for k in range(5, 18) for d in (-1, 0, 1)] + [65 * 64 + 32]
B2S_LONG = 2 * 1024 * 65 + 16 + 32      # the statement of a 1024-card proof


def _b2s_call(probe, mode, cases, tag):
    """cases: (len_a, len_b, pattern) per lane / quad; message A is staged and hashed first, B into the same buffer afterwards"""
    rng = random.Random(1000 * mode + len(cases))
    n = len(cases)
    maxlen = max(max(a, b) for a, b, _ in cases) + 1
    data = np.zeros((n, 2, maxlen), np.uint8)
    for x, (la, lb, _) in enumerate(cases):
        for s, ln in enumerate((la, lb)):      # (no zero bytes: what the hasher pads with must come from the hasher)
            data[x, s, :ln] = np.frombuffer(bytes(1 + b % 255 for b in rng.randbytes(ln)), np.uint8)
    lens = np.array([[a, b] for a, b, _ in cases], np.uint32)
    pats = np.array([p for _, _, p in cases], np.uint32)
    stride = _not_pow2(n + 3) | 1
    out = probe.blake2s(mode, stride, maxlen, data, lens, pats)
    fails = []
    for x, (la, lb, p) in enumerate(cases):
        for s, ln in enumerate((la, lb)):
            want = words(H(data[x, s, :ln].tobytes()))
            for j in range(out.shape[2]):
                if not np.array_equal(out[x, s, j], want):
                    fails.append("%s: %s message of %d bytes (%s, case %d, lane %d of the quad, staged %s a message of %d bytes): %s, expected %s"
                                 % (tag, "AB"[s], ln, PAT_NAMES[p], x, j, "before" if s == 0 else "after", (lb, la)[s],
                                    out[x, s, j].tobytes().hex(), want.tobytes().hex()))
    return fails, n * 2 * out.shape[2]


def run_blake2s(probe, mode):
    """mode 0: blake2s_staged, one case per lane; mode 1: blake2s_staged_quad, one case per quad, one length per wave"""
    if mode == 0:
        cases = [(ln + 1 + (7 * i) % 131, ln, p) for i, ln in enumerate(B2S_LENGTHS) for p in range(5)]
        long_cases = [(B2S_LONG + 77, B2S_LONG, p) for p in range(5)]
    else:
        cases = [(ln + 1 + (7 * i) % 131, ln, k % 5) for i, ln in enumerate(B2S_LENGTHS) for k in range(16)]
        long_cases = [(B2S_LONG + 77, B2S_LONG, k % 5) for k in range(16)]
    tag = "blake2s_staged_quad" if mode else "blake2s_staged"
    f1, c1 = _b2s_call(probe, mode, cases, tag)
    f2, c2 = _b2s_call(probe, mode, long_cases, tag)
    return f1 + f2, c1 + c2


# ---- fsq_absorb -------------------------------------------------------------------------------------------------------------------------
def absorb_batch(lpp):
    """proofs in the batch: not a multiple of the proofs per wave (64 / lpp), so that the clamped dead lanes of the last wave run"""
    per = 64 // lpp
    return 2 * per + 1 if per > 1 else 3


def run_fsq_absorb(probe, curve, lpp):
    nw = 12 if curve == "bls12_377" else 8
    rng = random.Random(31 * lpp + len(curve))
    B = absorb_batch(lpp)
    Bpad = _not_pow2(B + 6)
    fails, count = [], 0
    for npts in range(71):
        for tail_words in range(4):
            pts = _rand_words(rng, B, npts, 2 * nw + 1)
            tail = _rand_words(rng, B, tail_words)
            seed = _rand_words(rng, B, 8)
            got = probe.fsq_absorb(curve, lpp, Bpad, pts, tail, seed)
            for b in range(B):
                msg = b"".join(pts[b, i, :2 * nw].tobytes() + bytes([int(pts[b, i, 2 * nw]) & 0xFF]) for i in range(npts)) + tail[b].tobytes()
                s1 = H(msg + seed[b].tobytes())
                s2 = H(msg + s1)
                for r, want in enumerate((s1, s2)):
                    count += 1
                    if got[b, r].tobytes() != want:
                        fails.append("fsq_absorb %s lpp %d: %d points, %d tail words, proof %d of %d, absorb %d: %s, expected %s"
                                     % (curve, lpp, npts, tail_words, b, B, r + 1, got[b, r].tobytes().hex(), want.hex()))
    return fails, count


# ---- ChaCha20 and Fr::rand --------------------------------------------------------------------------------------------------------------
def run_chacha(probe):
    kc = _chacha_keys()
    keys = np.array([k for k, _ in kc], np.uint32)
    ctr = np.array([[c & M32, c >> 32] for _, c in kc], np.uint32)
    got = probe.chacha(keys, ctr)
    fails = ["chacha20_block key %s counter %d: %s" % (k, c, g.tobytes().hex())
             for (k, c), g in zip(kc, got) if list(map(int, g)) != mo.chacha20_block(k, c)]
    return fails, len(kc)


REJECT_RUN = {"stark": 8, "bn254": 4, "bls12_377": 6}
KEY_SEARCH_CAP = 200000


@functools.lru_cache(maxsize=None)
def frstream_keys(curve):
    """keys chosen by the reference alone: blake2s(b"fscheck key %d"), searched in order for streams whose first TRY_N candidates (a) start
    with a rejection, (b) have a rejection in half 1 of a block, so that the next candidate needs a refill, (c) have a run of at least
    REJECT_RUN consecutive rejections that crosses a block boundary -> (keys [n][8], {class: index of the first key found})"""
    found, keys = {}, [words(H(b"fscheck key %d" % i)) for i in range(8)]
    if curve in REJECT_RUN:
        run = REJECT_RUN[curve]
        # the cap is generous: a candidate is rejected with probability 1 - q / 2^BITS, a run can start at ~TRY_N places
        assert (1 - accept_rate(curve)) ** run * TRY_N * KEY_SEARCH_CAP > 1000
        i = 0
        while len(found) < 3 and i < KEY_SEARCH_CAP:
            batch = np.array([words(H(b"fscheck key %d" % k)) for k in range(i, min(i + 256, KEY_SEARCH_CAP))], np.uint32)
            _, acc = candidates(curve, batch, TRY_N // 2)
            for r, a in enumerate(acc):
                rej = ~a
                cls = []
                if rej[0]:
                    cls.append("starts with a rejection")
                if rej[1:TRY_N - 1:2].any():
                    cls.append("rejection in half 1, then a refill")
                for s in range(TRY_N - run):
                    if rej[s:s + run].all() and any(t % 2 == 1 for t in range(s, s + run - 1)):
                        cls.append("run of %d rejections across a block boundary" % run)
                        break
                for c in cls:
                    if c not in found:
                        found[c] = len(keys)
                        keys.append(batch[r])
            i += 256
    return np.array(keys, np.uint32), found


def run_frstream(probe, curve):
    keys, _ = frstream_keys(curve)
    nxt, flag, val = probe.frstream(curve, keys)
    want_next = fr_draws(curve, keys, NEXT_N)
    c, acc = candidates(curve, keys, TRY_N // 2)
    q = mo.CURVES[curve].q
    fails = []
    for i in range(len(keys)):
        assert all(to_int(w) < q for w in want_next[i][:4])
        if not np.array_equal(nxt[i], want_next[i]):
            k = int(np.flatnonzero((nxt[i] != want_next[i]).any(axis=1))[0])
            fails.append("frstream_next %s key %d: value %d is %x, expected %x" % (curve, i, k, to_int(nxt[i, k]), to_int(want_next[i, k])))
        if not np.array_equal(flag[i], acc[i].astype(np.uint32)):
            k = int(np.flatnonzero(flag[i] != acc[i])[0])
            fails.append("frstream_try %s key %d: candidate %d accepted = %d, expected %d" % (curve, i, k, flag[i, k], acc[i, k]))
        if not np.array_equal(val[i], c[i]):
            k = int(np.flatnonzero((val[i] != c[i]).any(axis=1))[0])
            fails.append("frstream_try %s key %d: candidate %d is %x, expected %x" % (curve, i, k, to_int(val[i, k]), to_int(c[i, k])))
    return fails, len(keys) * (NEXT_N + 2 * TRY_N)


# ---- chain / group weights --------------------------------------------------------------------------------------------------------------
CHAIN_L = [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 1024, 1025, 4097]
CHAIN_T = [1, 3, 65]


def chain_reference(curve, seeds):
    """seeds: [L][T][8] words.  dig_k = H(seed_{64k} || .. || seed_{min(L, 64k + 64) - 1}); table key = H(dig_0 || .. || dig_{nb-1});
    block key = H(table key || le32(k)); rho_j = the (j - 64k)-th accepted draw of ChaCha20(block key) -> (weights [L][T][8], digests
    [nb][T][8])"""
    L, T = seeds.shape[:2]
    nb = (L + CW_BLOCK - 1) // CW_BLOCK
    digs = np.zeros((nb, T, 8), np.uint32)
    bkeys = np.zeros((nb, T, 8), np.uint32)
    for t in range(T):
        col = np.ascontiguousarray(seeds[:, t, :])
        d = [H(col[64 * k:min(L, 64 * k + 64)].tobytes()) for k in range(nb)]
        tkey = H(b"".join(d))
        for k in range(nb):
            digs[k, t] = words(d[k])
            bkeys[k, t] = words(H(tkey + k.to_bytes(4, "little")))
    draws = fr_draws(curve, bkeys.reshape(-1, 8), min(L, CW_BLOCK)).reshape(nb, T, -1, 8)
    W = np.zeros((L, T, 8), np.uint32)
    for k in range(nb):
        cnt = min(L, 64 * k + 64) - 64 * k
        W[64 * k:64 * k + cnt] = draws[k, :, :cnt].transpose(1, 0, 2)
    return W, digs


def _seed_buffer(seeds, Bpad):
    L, T = seeds.shape[:2]
    buf = np.full((8, Bpad), 0x5EED5EED, np.uint32)
    buf[:, :L * T] = seeds.reshape(L * T, 8).T      # link j of table t at j T + t
    return buf


def check_weight_table(tag, CW, dig, W, digs, T):
    """device CW [L][Tpad][8], dig [nb][8][Tpad] against the reference; every weight non-zero, all pairwise distinct, padding untouched"""
    fails = []
    L = W.shape[0]
    if not np.array_equal(CW[:, :T], W):
        j, t = (int(v[0]) for v in np.nonzero((CW[:, :T] != W).any(axis=2)))
        fails.append("%s: weight of link %d, table %d is %x, expected %x (%d of %d weights differ)"
                     % (tag, j, t, to_int(CW[j, t]), to_int(W[j, t]), int((CW[:, :T] != W).any(axis=2).sum()), L * T))
    if not np.array_equal(dig[:, :, :T].transpose(0, 2, 1), digs):
        fails.append("%s: block digests differ" % tag)
    if not (CW[:, T:] == FILL).all():
        fails.append("%s: a weight was written into the padding columns" % tag)
    flat = np.ascontiguousarray(CW[:, :T]).reshape(L * T, 8)
    if not flat.any(axis=1).all():
        fails.append("%s: a weight is zero" % tag)
    if len(np.unique(flat.view(np.uint64).reshape(-1, 4), axis=0)) != L * T:
        fails.append("%s: weights repeat" % tag)
    return fails


def run_chain_weights(probe, curve, T):
    rng = random.Random(100 * T + len(curve))
    fails, count = [], 0
    for L in CHAIN_L:
        seeds = _rand_words(rng, L, T, 8)
        Tpad, Bpad = T + 2, L * T + 5
        CW, dig = probe.chain_weights(curve, T, L, Tpad, Bpad, _seed_buffer(seeds, Bpad))
        W, digs = chain_reference(curve, seeds)
        fails += check_weight_table("chain weights %s T %d L %d" % (curve, T, L), CW, dig, W, digs, T)
        count += L * T
    return fails, count


def run_chain_bit_flip(probe, curve):
    """one bit of one link's seed: every weight of that table changes, none of any other"""
    rng = random.Random(77 + len(curve))
    T, L, Tpad = 3, 130, 5
    Bpad = L * T + 5
    seeds = _rand_words(rng, L, T, 8)
    CW0, _ = probe.chain_weights(curve, T, L, Tpad, Bpad, _seed_buffer(seeds, Bpad))
    fails = []
    for j, t, w, bit in ((0, 0, 0, 0), (63, 1, 7, 31), (64, 2, 3, 5), (129, 1, 4, 17)):
        s2 = seeds.copy()
        s2[j, t, w] ^= np.uint32(1 << bit)
        CW1, dig1 = probe.chain_weights(curve, T, L, Tpad, Bpad, _seed_buffer(s2, Bpad))
        W, digs = chain_reference(curve, s2)
        fails += check_weight_table("chain weights %s after a bit flip" % curve, CW1, dig1, W, digs, T)
        changed = (CW0[:, :T] != CW1[:, :T]).any(axis=2)
        for tt in range(T):
            if tt == t and not changed[:, tt].all():
                fails.append("chain weights %s: bit %d of word %d of link %d's seed flipped, %d weights of table %d did not change"
                             % (curve, bit, w, j, int((~changed[:, tt]).sum()), t))
            if tt != t and changed[:, tt].any():
                fails.append("chain weights %s: a seed of table %d changed weights of table %d" % (curve, t, tt))
    return fails, 4 * L * T


# ---- lane digests of the sigma screen -----------------------------------------------------------------------------------------------------
SCREEN_G = [1, 63, 64, 65]


def run_screen_digest(probe, curve, nw):
    q = mo.CURVES[curve].q
    rng = random.Random(5 * nw + len(curve))
    fails, count = [], 0
    for g in SCREEN_G:
        B = 3 * g + g // 2 + 1 if g > 1 else 5      # not a multiple of g: the last group is short
        T, L = (B + g - 1) // g, g * nw
        Bpad, Tpad = B + 3, T + 2
        z = ([0, 1, q - 1] + [rng.randrange(q) for _ in range(B)])[:B]
        seeds = _rand_words(rng, B, 8)
        seed_buf = np.full((8, Bpad), 0x5EED5EED, np.uint32)
        seed_buf[:, :B] = seeds.T
        S = _rand_words(rng, 3, Bpad, 8)
        for x in range(B):
            S[2, x] = mont_words(curve, z[x])
        out, CW, dig = probe.screen_digest(curve, B, g, nw, Bpad, Tpad, seed_buf, S)
        lane = np.zeros((T * g, 8), np.uint32)      # H(seed || le256(z)); lanes past the end of the call hash as zeros
        for x in range(B):
            lane[x] = words(H(seeds[x].tobytes() + le256(z[x])))
        link = np.zeros((L, T, 8), np.uint32)       # row (j nw + i) T + t
        for t in range(T):
            for j in range(g):
                for i in range(nw):
                    link[j * nw + i, t] = lane[t * g + j]
        tag = "screen digest %s g %d nw %d B %d" % (curve, g, nw, B)
        if not np.array_equal(out, link.reshape(L * T, 8).T):
            bad = np.flatnonzero((out != link.reshape(L * T, 8).T).any(axis=0))
            fails.append("%s: %d of %d rows differ, first row %d" % (tag, len(bad), L * T, int(bad[0])))
        W, digs = chain_reference(curve, link)
        # (the nw checks of a lane share a digest and the zero lanes of a short group one another's: distinct WEIGHTS is the property)
        fails += check_weight_table(tag + " weights", CW, dig, W, digs, T)
        count += L * T
    return fails, count


# ---- weights of the merged equation ---------------------------------------------------------------------------------------------------
MERGE_N = [2, 3, 5, 26, 128]
MERGE_M = 2


def merge_reference(curve, z, seed, vc_count):
    """z: [5n + 9][B] integers, seed: [B][8] -> seed' = H(le256(z_0) || .. || le256(z_{5n+8}) || seed), r_k = the k-th draw of ChaCha20(seed')"""
    B = len(seed)
    s2 = np.array([words(H(b"".join(le256(z[i][b]) for i in range(len(z))) + seed[b].tobytes())) for b in range(B)], np.uint32)
    return fr_draws(curve, s2, vc_count), s2


def _merge_inputs(curve, n, B, rng):
    E = scalar_edges(curve)
    nsc = 5 * n + 9
    z = [[E[(i * B + b) % len(E)] if (i + b) % 3 else rng.randrange(mo.CURVES[curve].q) for b in range(B)] for i in range(nsc)]
    scal = np.array([[mont_words(curve, z[i][b]) for b in range(B)] for i in range(nsc)], np.uint32)
    return z, scal, _rand_words(rng, B, 8)


def run_merge_weights(probe, curve, n):
    """fs_merge_weights (one lane) and fsq_merge_weights (every lanes-per-proof) on the same arena: both equal the reference, hence
    each other word for word"""
    rng = random.Random(9 * n + len(curve))
    B = 9                                   # not a multiple of 64 / lpp for lpp < 64
    Bpad = 13
    z, scal, seed = _merge_inputs(curve, n, B, rng)
    want_r, want_s = merge_reference(curve, z, seed, probe.vc_count)
    fails, count = [], 0
    one = None
    for mode, lpp in [(0, 0)] + [(1, v) for v in LPPS]:
        mr, s2 = probe.merge_weights(curve, mode, MERGE_M, n, lpp, Bpad, scal, seed)
        tag = "merge weights %s n %d %s" % (curve, n, "one lane" if mode == 0 else "lpp %d" % lpp)
        if not np.array_equal(s2, want_s):
            fails.append("%s: f.seed differs for proofs %s" % (tag, np.flatnonzero((s2 != want_s).any(axis=1)).tolist()))
        if not np.array_equal(mr, want_r):
            b, k = (int(v[0]) for v in np.nonzero((mr != want_r).any(axis=2)))
            fails.append("%s: r_%d of proof %d is %x, expected %x" % (tag, k, b, to_int(mr[b, k]), to_int(want_r[b, k])))
        if not mr.any(axis=2).all():
            fails.append("%s: a weight is zero" % tag)
        if mode == 0:
            one = (mr, s2)
        elif not (np.array_equal(mr, one[0]) and np.array_equal(s2, one[1])):
            fails.append("%s: differs from the one-lane kernel" % tag)
        count += B * (probe.vc_count + 1)
    return fails, count


def run_merge_scalar_flips(probe, curve, mode, lpp):
    """n = 3: lane 0 is the base, lane 1 + i has one bit of response scalar i flipped: every r_k must change"""
    n = 3
    nsc = 5 * n + 9
    rng = random.Random(3 + len(curve))
    q = mo.CURVES[curve].q
    z0, _, seed0 = _merge_inputs(curve, n, 1, rng)
    B = nsc + 1
    z = [[z0[i][0]] * B for i in range(nsc)]
    for i in range(nsc):
        z[i][1 + i] = (z0[i][0] ^ 1) % q
        assert z[i][1 + i] != z0[i][0]
    scal = np.array([[mont_words(curve, z[i][b]) for b in range(B)] for i in range(nsc)], np.uint32)
    seed = np.repeat(seed0, B, axis=0)
    mr, s2 = probe.merge_weights(curve, mode, MERGE_M, n, lpp, _not_pow2(B + 2), scal, seed)
    want_r, want_s = merge_reference(curve, z, seed, probe.vc_count)
    fails = []
    if not (np.array_equal(mr, want_r) and np.array_equal(s2, want_s)):
        fails.append("merge weights %s mode %d: differ from the reference for proofs %s"
                     % (curve, mode, np.flatnonzero((mr != want_r).any(axis=(1, 2)) | (s2 != want_s).any(axis=1)).tolist()))
    for i in range(nsc):
        same = np.flatnonzero(~(mr[1 + i] != mr[0]).any(axis=1))
        if len(same):
            fails.append("merge weights %s mode %d: a bit of response scalar %d flipped, r_%s did not change" % (curve, mode, i, same.tolist()))
    return fails, nsc * probe.vc_count


# ---- black box: every element of a proof is enforced under both transcript kernels ---------------------------------------------------------
ELEMENT_SHAPES = [("stark", 2, 3), ("bls12_377", 2, 5)]


def wire_map(m, n, pb):
    """byte offsets of the 11m + 8 points and of the 5n + 9 response scalars of a wire proof (mp_oracle.proof_to_bytes: the arguments'
    points and responses alternate)"""
    pts, scs, o = [], [], 0
    for kind, cnt in (("p", 3 * m + 1 + 2 + 2 * m + 1), ("s", 2 * n + 3), ("p", 3), ("s", 2 * n + 2), ("p", 1 + 6 * m), ("s", n + 4)):
        for _ in range(cnt):
            (pts if kind == "p" else scs).append(o)
            o += pb if kind == "p" else 32
    assert len(pts) == 11 * m + 8 and len(scs) == 5 * n + 9
    return pts, scs, o


def run_element_tamper(eng, coracle, curve, m, n):
    """one honest proof plus a copy per element -- each of the 11m + 8 points replaced by a DIFFERENT valid point (one of the commitment
    key), each of the 5n + 9 scalars + 1 mod q -- verified in one batch with merged verification on, under one-lane and four-lane
    transcripts: every copy is rejected with exactly the oracle's check code"""
    q = mo.CURVES[curve].q
    pb = eng.point_bytes
    g0 = coracle.gen_inputs(curve, m, n, 4242)
    out_deck, proof = coracle.shuffle_and_remask(curve, m, n, g0["params"], g0["pk"], g0["deck"], g0["rho"], g0["perm"], g0["prover_seed"])
    pts, scs, size = wire_map(m, n, pb)
    assert len(proof) == size
    key_pts = [g0["params"][i * pb:(i + 1) * pb] for i in range(n + 3)]
    copies, names = [proof], ["honest"]
    for i, o in enumerate(pts):
        new = next(p for p in key_pts[1:] + key_pts[:1] if p != proof[o:o + pb])
        copies.append(proof[:o] + new + proof[o + pb:])
        names.append("point %d" % i)
    for i, o in enumerate(scs):
        copies.append(proof[:o] + le256((int.from_bytes(proof[o:o + 32], "little") + 1) % q) + proof[o + 32:])
        names.append("scalar %d" % i)
    B = len(copies)
    want = [coracle.verify_shuffle(curve, m, n, g0["params"], g0["pk"], g0["deck"], out_deck, c) for c in copies]
    fails = []
    if want[0] != 0 or not all(w > 0 for w in want[1:]):
        fails.append("%s (%d, %d): the oracle's verdicts are %s" % (curve, m, n, want))
    t = eng.table(m, n, g0["params"], g0["pk"])
    try:
        t.set_latency_batch(0)
        t.set_merged_verify(True)
        for lanes in (1, 4):
            t.set_transcript_lanes(lanes)
            got = t.verify_shuffle_batch(g0["deck"] * B, out_deck * B, b"".join(copies))
            for i in range(B):
                if got[i] != want[i]:
                    fails.append("%s (%d, %d), %d-lane transcripts: %s gives status %d, the oracle %d" % (curve, m, n, lanes, names[i], got[i], want[i]))
    finally:
        t.close()
    return fails, 2 * B


# ---- black box: a weight is applied at every position of a group equation and of a chain equation ------------------------------------------
BB_CURVE, BB_M, BB_N = "stark", 2, 3
BB_PER = 4 * BB_M * BB_N + 11 * BB_M + 8      # points a proof brings into a group equation: 54
GROUP_L = [65, 129]


def _prove(t, eng, torch, decks, seed):
    """one batched prover call on device tensors -> (shuffled decks, proofs)"""
    B, dev, N = decks.shape[0], decks.device, BB_M * BB_N
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    rho = torch.randint(0, 256, (B, N, 32), dtype=torch.uint8, device=dev, generator=gen)
    rho[:, :, 31] &= 7
    perm = torch.argsort(torch.rand(B, N, device=dev, generator=gen), dim=1).to(torch.int32).contiguous()
    seeds = torch.randint(0, 256, (B, 32), dtype=torch.uint8, device=dev, generator=gen)
    od = torch.empty_like(decks)
    op = torch.empty(B, t.proof_bytes, dtype=torch.uint8, device=dev)
    sp = torch.empty(B, dtype=torch.int32, device=dev)
    t.shuffle_and_remask_batch_dev(B, decks.data_ptr(), rho.data_ptr(), perm.data_ptr(), seeds.data_ptr(), od.data_ptr(), op.data_ptr(), sp.data_ptr())
    eng.sync()
    assert int(sp.abs().sum().item()) == 0
    return od, op


def run_group_members(eng, coracle, torch, dev, L):
    """B = L^2 six-card proofs in T = L group equations of L members (lane of (member j, group t) = j T + t); the proof at lane t (T + 1)
    has the low bit of one response scalar flipped, so group t has exactly member t bad and every member position 0 .. L - 1 -- both sides
    of the 64-link blocks of the weights -- is hit once.  The status words are those of equation-by-equation verification, eight lanes are
    checked against the oracle, and every group was flagged: none was waved through"""
    T, B = L, L * L
    scalars = wire_map(BB_M, BB_N, 64)[1]
    g0 = coracle.gen_inputs(BB_CURVE, BB_M, BB_N, 7100 + L)
    t = eng.table(BB_M, BB_N, g0["params"], g0["pk"], fb_bits=8)
    fails = []
    try:
        decks = torch.frombuffer(bytearray(g0["deck"]), dtype=torch.uint8).to(dev).repeat(B, 1).contiguous()
        od, op = _prove(t, eng, torch, decks, 7100 + L)
        sv = torch.full((B,), 55, dtype=torch.int32, device=dev)

        def verify():
            sv.fill_(55)
            t.verify_shuffle_batch_dev(B, decks.data_ptr(), od.data_ptr(), op.data_ptr(), sv.data_ptr())
            eng.sync()
            return sv.cpu().tolist()
        t.set_group_adapt(False)
        # the honest batch first: every equation holds, so no group is flagged -- an equation that drops or doubles a member's term
        # fails for honest groups too and would hide behind the per-equation pass
        t.set_group_verify(BB_PER * L, 0)
        t.set_group_refine(0, 1 << 30)      # (flagged groups go straight to the per-equation pass: sub-group equations would clear them unseen)
        before = t.reverified_count()
        if verify() != [0] * B or t.reverified_count() != before:
            fails.append("groups of %d, honest batch: %d proofs rejected, %d looked at again" % (L, sum(1 for v in sv.cpu().tolist() if v), t.reverified_count() - before))
        bad = [k * (T + 1) for k in range(T)]
        for k, lane in enumerate(bad):
            op[lane, scalars[k % len(scalars)]] ^= 1
        t.set_merged_verify(False)
        want = verify()
        if [i for i, v in enumerate(want) if v] != bad or not all(want[i] > 0 for i in bad):
            fails.append("equation by equation: rejected lanes %s, tampered lanes %s" % ([i for i, v in enumerate(want) if v][:9], bad[:9]))
        deck_b = bytes(g0["deck"])
        spot = [bad[0], bad[63], bad[64], bad[L - 1], 1, T, B - 2, bad[1] + 1]
        od_c, op_c = od[spot].cpu().numpy(), op[spot].cpu().numpy()
        for k, lane in enumerate(spot):
            o = coracle.verify_shuffle(BB_CURVE, BB_M, BB_N, g0["params"], g0["pk"], deck_b, od_c[k].tobytes(), op_c[k].tobytes())
            if o != want[lane]:
                fails.append("lane %d: status %d, the oracle says %d" % (lane, want[lane], o))
        t.set_merged_verify(True)
        t.set_group_verify(BB_PER * L, 0)
        if t.group_size(B) != L:
            fails.append("group_size(%d) is %d, not %d" % (B, t.group_size(B), L))
        # a failing group's members go straight to the per-equation pass (no sub-group equations in between), so that the count of
        # proofs looked at again says how many GROUPS failed; then once more with the default refinement: same status words
        for refine, tag in (((0, 1 << 30), "groups of %d" % L), ((0, 0), "groups of %d, refined by sub-groups" % L)):
            t.set_group_refine(*refine)
            before = t.reverified_count()
            got = verify()
            for i in range(B):
                if got[i] != want[i]:
                    fails.append("%s: lane %d (member %d of group %d) has status %d, equation by equation %d" % (tag, i, i // T, i % T, got[i], want[i]))
            looked = t.reverified_count() - before
            if refine[1] and looked != B:
                fails.append("%s: %d proofs were looked at again, not all %d" % (tag, looked, B))
            if not refine[1] and not L <= looked <= B:
                fails.append("%s: %d proofs were looked at again" % (tag, looked))
    finally:
        t.close()
    return fails, 4 * B + 8


def run_chain_links(eng, coracle, torch, dev, T, L):
    """T tables of L links, one chain equation per table; link t of table t is tampered: the verdicts are those of the per-link verifier"""
    scalars = wire_map(BB_M, BB_N, 64)[1]
    g0 = coracle.gen_inputs(BB_CURVE, BB_M, BB_N, 7300)
    t = eng.table(BB_M, BB_N, g0["params"], g0["pk"], fb_bits=8)
    fails = []
    try:
        chain = [torch.frombuffer(bytearray(g0["deck"]), dtype=torch.uint8).to(dev).repeat(T, 1).contiguous()]
        proofs = []
        for j in range(L):
            od, op = _prove(t, eng, torch, chain[j], 7300 + j)
            chain.append(od)
            proofs.append(op)
        decks = torch.cat(chain).contiguous()              # deck j of table t at j T + t
        pf = torch.cat(proofs).contiguous()                # link j of table t at lane j T + t
        bad = [k * T + k for k in range(min(T, L))]
        for k, lane in enumerate(bad):
            pf[lane, scalars[k % len(scalars)]] ^= 1
        sv = torch.full((L * T,), 55, dtype=torch.int32, device=dev)
        t.verify_shuffle_batch_dev(L * T, decks[:L * T].data_ptr(), decks[T:].data_ptr(), pf.data_ptr(), sv.data_ptr())
        eng.sync()
        want = sv.cpu().tolist()
        if [i for i, v in enumerate(want) if v] != bad or not all(want[i] > 0 for i in bad):
            fails.append("link by link: rejected lanes %s, tampered lanes %s" % ([i for i, v in enumerate(want) if v][:9], bad[:9]))
        t.set_chain_max_links(L)
        t.set_chain_group(1)
        if t.chain_group_size(T, L) != 1:
            fails.append("chain_group_size is %d" % t.chain_group_size(T, L))
        sv.fill_(55)
        t.verify_shuffle_chain_dev(T, L, None, decks.data_ptr(), pf.data_ptr(), sv.data_ptr())
        eng.sync()
        got = sv.cpu().tolist()
        for i in range(L * T):
            if got[i] != want[i]:
                fails.append("chain: link %d of table %d has status %d, link by link %d" % (i // T, i % T, got[i], want[i]))
    finally:
        t.close()
    return fails, 2 * L * T
