"""Cases, models and checks for the digit probe (tools/digitcheck/digit_check.hip): one scalar per lane, cut into digits by the engine's own
fb_digit (fixed-base tables, unsigned 8 / 16 / 20 / 21-bit windows), k_recode (Straus, signed 5-bit) and k_bucket_recode (bucket method,
signed c-bit digits of min(k, q - k), c = 8 .. 14), compared digit for digit with the Python-integer statement of each recoding below.
Shared by tests/test_digit_emu.py (the probe built against the development emulator, CPU) and tests/test_gpu_digit.py (the gfx950 build)
-- same cases, same expectations, exact equality -- and by tests/fixed_base_cases.py, which sends the same scalar families through the
MSM kernels.

The models are written from the comments of kernels_msm.hpp / kernels_bucket.hpp / layout.hpp, not from the code:
  fixed base  window w of the canonical scalar: bits [w bits, (w + 1) bits), ceil(BITS / bits) windows;
  Straus      v = window + carry in [0, 32]; v > 16 becomes v - 32 with a carry into the next window: digits in [-15, 16],
              ceil((BITS + 1) / 5) windows;
  bucket      k or q - k, whichever is smaller (k = 0 stays), the signs of the digits flipped in the second case; a window + carry that
              reaches 2^(c-1) becomes negative with a carry, except in the top window, which is 0 .. 2^(c-1), the last bucket included;
              ceil(BITS / c) windows.
Every number that depends on a group order is computed here from mp_oracle.CURVES.

Every run_* function returns (failure messages, number of comparisons); the tests assert that the first is empty."""
import ctypes
import functools
import os
import random
import subprocess

import numpy as np

import mp_oracle as mo
import prim_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tools", "digitcheck")
GPU_LIB = os.path.join(PROBE_DIR, "libdigitcheck.so")
EMU_LIB = os.path.join(PROBE_DIR, "libdigitcheck_emu.so")

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
KIND_FIXED, KIND_STRAUS, KIND_BUCKET = 0, 1, 2
FB_BITS = (8, 16, 20, 21)
STRAUS_BITS = 5
BUCKET_BITS = tuple(range(8, 15))
STRIDE = 64                     # digits per scalar in the probe's output (>= the 52 Straus windows of secp256k1)
N_RANDOM = 3000


def order(curve):
    return mo.CURVES[curve].q


def windows(q, kind, width):
    bits = q.bit_length()
    return -(-(bits + 1) // width) if kind == KIND_STRAUS else -(-bits // width)


def narrow_bits(bits):
    """the width of the low half of a wide fixed-base window (engine_core.hpp build_fixed_tables): 8 for 16-bit tables, 10 for 20-bit
    ones, 11 (low) + 10 (high) for 21-bit ones; 8-bit tables are not split (4: a digit in the middle)"""
    return 4 if bits == 8 else (bits + 1) // 2


# ---- the recodings on Python integers -------------------------------------------------------------------------------------------------
def model_fixed(k, q, bits):
    return [(k >> (w * bits)) & ((1 << bits) - 1) for w in range(windows(q, KIND_FIXED, bits))]


def model_straus(k, q):
    out, carry = [], 0
    for w in range(windows(q, KIND_STRAUS, STRAUS_BITS)):
        v = ((k >> (STRAUS_BITS * w)) & 31) + carry
        carry = 1 if v > 16 else 0
        out.append(v - 32 if carry else v)
    return out


def model_bucket(k, q, c):
    """-> (flip, digits as the kernel stores them: after the flip)"""
    flip = q - k < k
    u = q - k if flip else k
    nwin = windows(q, KIND_BUCKET, c)
    out, carry = [], 0
    for w in range(nwin):
        v = ((u >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 0
        if w + 1 < nwin and v >= 1 << (c - 1):
            v -= 1 << c
            carry = 1
        out.append(-v if flip else v)
    return flip, out


def model(kind, k, q, width):
    if kind == KIND_FIXED:
        return model_fixed(k, q, width)
    if kind == KIND_STRAUS:
        return model_straus(k, q)
    return model_bucket(k, q, width)[1]


def boundaries(kind, width):
    """the recoding boundaries h of a width: 16 and 17 for Straus (a window of 16 stays, one of 17 carries), 2^(c-1) for the bucket widths,
    2^(narrow width) for the fixed-base windows (the first digit whose high half is not zero)"""
    if kind == KIND_STRAUS:
        return (16, 17)
    if kind == KIND_BUCKET:
        return (1 << (width - 1),)
    return (1 << narrow_bits(width),)


# ---- scalar families ---------------------------------------------------------------------------------------------------------------------
def _below(q, vals):
    seen, out = set(), []
    for v in vals:
        if 0 <= v < q and v not in seen:
            seen.add(v)
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def families(q, kind, width):
    """-> ((name, scalars), ...), every scalar below q, no scalar twice in a family"""
    bits = q.bit_length()
    nwin = windows(q, kind, width)
    ones = (1 << width) - 1
    fam = [("edge values", list(pc.edge_values(q)))]
    per_window, chains = [], []
    for h in boundaries(kind, width):
        for w in range(nwin):
            for d in (h - 1, h, h + 1, ones, 1):
                v = d << (w * width)
                per_window += [v, q - v]                  # (the negative mod q; _below drops what is not in [0, q))
        for d in (h - 1, h, ones):
            v = sum(d << (w * width) for w in range(nwin))
            chains += [v % q, v & ((1 << (bits - 1)) - 1), v & ((1 << bits) - 1), q - v % q]
    fam.append(("one boundary digit per window", _below(q, per_window)))
    fam.append(("every window on a boundary", _below(q, chains)))
    half = [(q - 1) // 2, (q + 1) // 2]
    for j in range(bits):
        half += [(q - 1) // 2 + (1 << j), (q - 1) // 2 - (1 << j)]
    fam.append(("around the middle", _below(q, half)))
    rng = random.Random(q % 1000003 + 7)                  # (the same for every width: the MSM tests compute their reference once)
    fam.append(("random", _below(q, [rng.randrange(q) for _ in range(N_RANDOM)])))
    return tuple((name, tuple(vals)) for name, vals in fam)


# ---- the probe -----------------------------------------------------------------------------------------------------------------------
def build_emu_probe():
    """the probe against the development emulator (kernel bodies as CPU loops): the recipe of prim_cases.build_emu_probe"""
    src = os.path.join(PROBE_DIR, "digit_check.hip")
    csrc = os.path.join(ROOT, "mental-poker_amd", "csrc")
    emu = os.path.join(ROOT, "tools", "hostemu")
    deps = [src, os.path.join(emu, "rt.hpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(EMU_LIB) or os.path.getmtime(EMU_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-x", "c++", "-include", os.path.join(emu, "rt.hpp"),
                               "-I" + emu, "-I" + csrc, src, "-o", EMU_LIB])
    return EMU_LIB


class Probe:
    def __init__(self, path):
        if not os.path.exists(path):
            raise ImportError("%s is not built (the gfx950 probe is built by __graft_entry__.build())" % path)
        self.lib = lib = ctypes.CDLL(path)
        u, vp = ctypes.c_uint32, ctypes.c_void_p
        lib.dc_rt_name.restype = ctypes.c_char_p
        for c in CURVES:
            getattr(lib, "dc_error_" + c).restype = ctypes.c_char_p
            getattr(lib, "dc_scalar_bits_" + c).restype = u
            getattr(lib, "dc_digits_" + c).argtypes = [ctypes.c_int, u, u, vp, u, vp, vp, vp]
        self.rt_name = lib.dc_rt_name().decode()
        self.dead = None

    def scalar_bits(self, curve):
        return getattr(self.lib, "dc_scalar_bits_" + curve)()

    def digits(self, curve, kind, width, scalars):
        """-> (int32 array [n][nwin], nwin).  A runtime error (a failed launch or copy) ends the probe's use of the device"""
        if self.dead:
            raise RuntimeError("digit_check: not run, an earlier call failed: %s" % self.dead)
        n = len(scalars)
        wire = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in scalars), dtype=np.uint8).copy()
        out, status, nwin = np.full((n, STRIDE), 0x55AA55, np.int32), np.full(n, 77, np.int32), ctypes.c_uint32(0)
        rc = getattr(self.lib, "dc_digits_" + curve)(kind, width, n, wire.ctypes.data_as(ctypes.c_void_p), STRIDE,
                                                     out.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p),
                                                     ctypes.byref(nwin))
        if rc != 0:
            self.dead = getattr(self.lib, "dc_error_" + curve)().decode()
            raise RuntimeError("digit_check: " + self.dead)
        assert not status.any(), "k_load_scalars refused a scalar below q"
        assert not out[:, nwin.value:].any(), "digits beyond the last window"
        return out[:, :nwin.value], nwin.value


# ---- checks ------------------------------------------------------------------------------------------------------------------------------
def check_digits(q, kind, width, k, got):
    """the properties of one scalar's digits that hold whatever the model says -> message or None"""
    nwin = len(got)
    if kind == KIND_FIXED:
        lo, hi = 0, (1 << width) - 1
    elif kind == KIND_STRAUS:
        lo, hi = -15, 16
    else:
        lo, hi = -(1 << (width - 1)), 1 << (width - 1)
    if min(got) < lo or max(got) > hi:
        return "a digit is outside [%d, %d]" % (lo, hi)
    total = sum(d << (w * width) for w, d in enumerate(got))
    if kind != KIND_BUCKET:
        return None if total == k else "the digits add up to %#x" % total
    flip = model_bucket(k, q, width)[0]
    if (-got[nwin - 1] if flip else got[nwin - 1]) < 0:
        return "the top window is negative before the flip"
    want = -(q - k) if flip else k                        # (either way k mod q: the flipped digits are those of k - q)
    if total != want or total % q != k:
        return "the digits add up to %#x, not to %#x" % (total, want)
    return None


def run_digits(probe, curve, kind, width):
    q = order(curve)
    fails, n = [], 0
    if probe.scalar_bits(curve) != q.bit_length():
        fails.append("%s: the engine's scalar field has %d bits, the order %d" % (curve, probe.scalar_bits(curve), q.bit_length()))
    for name, scalars in families(q, kind, width):
        got, nwin = probe.digits(curve, kind, width, scalars)
        if nwin != windows(q, kind, width):
            fails.append("%s kind %d width %d: %d windows, expected %d" % (curve, kind, width, nwin, windows(q, kind, width)))
            continue
        for k, row in zip(scalars, got.tolist()):
            want = model(kind, k, q, width)
            err = "differs from the model %s" % want if row != want else check_digits(q, kind, width, k, row)
            if err and len(fails) < 12:
                fails.append("%s kind %d width %d [%s] k = %#x: digits %s: %s" % (curve, kind, width, name, k, row, err))
        n += len(scalars)
    return fails, n


def top_digit_reach(q, c):
    """the largest top digit (before the flip) any scalar below q has: min(k, q - k) <= (q - 1) / 2, plus the carry of the window below"""
    nwin = windows(q, KIND_BUCKET, c)
    return (((q - 1) // 2) >> (c * (nwin - 1))) + 1


def run_last_bucket(probe):
    """secp256k1 with 8-bit bucket windows: (q - 1) / 2 has 127 in the top window and a carry chain through the windows of 255 below it, so
    the top digit is 128 = 2^(c-1), the last bucket.  No other (curve, width) has a scalar whose top digit gets there"""
    fails = []
    q, c = order("secp256k1"), 8
    k = (q - 1) // 2
    flip, want = model_bucket(k, q, c)
    if flip or want[-1] != 128 or (k >> (c * (len(want) - 1))) != 127:
        fails.append("the model's digits of (q - 1) / 2 on secp256k1, c = 8: %s" % want)
    got, _ = probe.digits("secp256k1", KIND_BUCKET, c, [k, k + 1])
    got = got.tolist()
    if got[0][-1] != 128 or got[0] != want:
        fails.append("secp256k1 c = 8, (q - 1) / 2: the probe's digits %s, the model's %s" % (got[0], want))
    if got[1][-1] != -128 or got[1] != [-d for d in want]:      # (q + 1) / 2 = q - (q - 1) / 2: the same digits, flipped
        fails.append("secp256k1 c = 8, (q + 1) / 2: the probe's digits %s" % got[1])
    n = 2
    for curve in CURVES:
        for cc in BUCKET_BITS:
            reach = top_digit_reach(order(curve), cc)
            if (curve, cc) == ("secp256k1", 8):
                if reach != 128:
                    fails.append("secp256k1 c = 8: the top digit reaches %d" % reach)
            elif reach >= 1 << (cc - 1):
                fails.append("%s c = %d: the top digit reaches %d >= 2^(c-1)" % (curve, cc, reach))
            n += 1
    return fails, n
