"""CPU tests (-m "not gpu") of the device conversions between wire v1 and canonical bytes (kernels_canonical.hpp behind
mp_points_serialize_dev, mp_deck_serialize_dev, mp_proof_serialize_dev, mp_proof_deserialize_dev, mp_decks_deserialize_batch and
mp_proofs_deserialize_batch): the six names in the header, the binding and both builds, and the kernel bodies under the development
emulator (tools/hostemu) on the shared cases of tests/canonical_dev_cases.py.  Calls beyond one launch, proofs from the device prover
and the Python mirror run on the GPU only (tests/test_gpu_canonical_dev.py)."""
import ctypes
import os
import re
import subprocess

import pytest

import canonical_dev_cases as cc
import decompress_pool as dp
from conftest import GOLDEN, ROOT, load_json

CURVES = ["stark", "bn254", "secp256k1", "bls12_377"]
FIXTURES = ["shuffle_stark_m2_n3_s1.json", "shuffle_stark_m3_n4_s11.json", "shuffle_stark_m2_n26_s7.json", "shuffle_stark_m4_n13_s9.json",
            "shuffle_bn254_m2_n4_s3.json", "shuffle_secp256k1_m3_n3_s5.json", "shuffle_bls12_377_m2_n3_s13.json"]
MALFORMED = ["shuffle_stark_m2_n3_s1.json", "shuffle_bls12_377_m2_n3_s13.json", "shuffle_secp256k1_m3_n3_s5.json"]


class _HostMem:
    """the emulator's "device" memory is host memory: ctypes buffers stand in for HBM; fresh ones hold 0x5A"""

    def put(self, b):
        buf = (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")
        return buf, ctypes.addressof(buf)

    def new(self, nbytes):
        buf = (ctypes.c_uint8 * max(nbytes, 1)).from_buffer_copy(b"\x5a" * max(nbytes, 1))
        return buf, ctypes.addressof(buf)

    def get(self, h, nbytes):
        return bytes(h)[:nbytes]


@pytest.fixture(scope="module")
def native(mp):
    mp.build()
    return mp


@pytest.fixture(scope="module")
def emulib(native):
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    return ctypes.CDLL(os.path.join(d, "libmpemu.so"))


@pytest.fixture(scope="module")
def emu(native, emulib):
    """curve -> (engine on the emulator, the emulator library's host serialiser)"""
    lib = native._native.bind(emulib)
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = (native._native.Engine(curve, 0, lib=lib), native.Serializer(curve, lib=lib))
        return made[curve]
    yield get
    for e, _ in made.values():
        e.close()


def test_the_six_names_are_declared_bound_and_exported(native, emulib):
    """include/mpshuffle.h declares them, _native.SYMBOLS lists them, bind() gives each a prototype, and both the emulator build and the
    gfx950 build export them"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpshuffle.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", txt))
    product = native.load()
    fresh = native._native.bind(ctypes.CDLL(os.path.join(ROOT, "tools", "hostemu", "libmpemu.so")))
    for s in cc.SYMBOLS:
        assert s in declared, s
        assert s in native._native.SYMBOLS, s
        assert hasattr(emulib, s) and hasattr(product, s), s
        assert getattr(fresh, s).argtypes and getattr(product, s).argtypes, s
    for s in ("points_serialize_dev", "deck_serialize_dev", "proof_serialize_dev", "proof_deserialize_dev", "decks_deserialize_batch",
              "proofs_deserialize_batch"):
        assert callable(getattr(native.Engine, s)), s
    assert callable(native.DLCards.deserialize_proofs) and callable(native.DLCards.deserialize_decks)
    mirror = open(os.path.join(ROOT, "include", "barnett_smart.hpp")).read()
    for s in cc.SYMBOLS:
        assert s + "(" in mirror, s


@pytest.mark.parametrize("curve", CURVES)
def test_emulated_point_compression(emu, native, curve):
    eng, ser = emu(curve)
    pool = dp.pool(curve)
    cc.run_point_compression(eng, _HostMem(), ser, curve, pool)
    cc.run_point_range_checks(eng, _HostMem(), ser, native.NativeError, curve, pool)


@pytest.mark.parametrize("curve", CURVES)
def test_emulated_deck_framing(emu, curve):
    eng, ser = emu(curve)
    cc.run_deck_framing(eng, _HostMem(), ser, curve, dp.pool(curve))


@pytest.mark.parametrize("name", FIXTURES)
def test_emulated_proof_conversion_on_the_fixtures(emu, native, name):
    """the committed proofs through both directions; those of the small shapes are verified after the round trip"""
    g = load_json(os.path.join(GOLDEN, name))
    curve, m, n = g["curve"], g["m"], g["n"]
    eng, ser = emu(curve)
    verify = None
    if m * n <= 12:
        t = native._native.Table(eng, m, n, bytes.fromhex(g["params"]), bytes.fromhex(g["pk"]))
        verify = lambda wire: t.verify_shuffle_batch(bytes.fromhex(g["deck"]), bytes.fromhex(g["shuffled"]), wire)
    cc.run_proof_round_trip(eng, _HostMem(), ser, curve, m, n, [bytes.fromhex(g["proof"])], verify)


@pytest.mark.parametrize("m,n,B", [(2, 3, 1), (2, 3, 63), (2, 3, 64), (2, 3, 65), (3, 4, 65)])
def test_emulated_proof_conversion_in_batches(emu, native, coracle, m, n, B):
    """B proofs drawn from five different ones of the oracle's prover; the five that come back are verified"""
    eng, ser = emu("stark")
    g, shuffled, proofs = cc.distinct_proofs(coracle, "stark", m, n, 5)
    idx, rows = cc.tiled(proofs, B)
    mem = _HostMem()
    cc.run_proof_round_trip(eng, mem, ser, "stark", m, n, rows)
    if B == 65:
        t = native._native.Table(eng, m, n, g["params"], g["pk"])
        back, st = cc.proofs_deserialize(eng, mem, "stark", m, n, b"".join(ser.proof_serialize(m, n, p) for p in proofs))
        assert st == [0] * 5 and t.verify_shuffle_batch(g["deck"] * 5, b"".join(shuffled), back) == [0] * 5


@pytest.mark.parametrize("name", MALFORMED)
def test_emulated_malformed_proofs(emu, native, name):
    """batches of 65 with one defect per defective lane (every Vec length off by +1, -1, +2^32; a refused point of every family in every
    point group; q and 2^256 - 1 in the first and last scalar of every scalar group; q - 1 accepted), through mp_proof_deserialize_dev
    and through mp_proofs_deserialize_batch with pageable buffers"""
    g = load_json(os.path.join(GOLDEN, name))
    curve, m, n = g["curve"], g["m"], g["n"]
    eng, ser = emu(curve)
    batch = lambda data: eng.proofs_deserialize_batch(m, n, 65, data)
    cc.run_malformed_proofs(eng, _HostMem(), ser, native.NativeError, curve, m, n, bytes.fromhex(g["proof"]), dp.pool(curve),
                            convert_batch=batch)


@pytest.mark.parametrize("pinned", [False, True])
def test_emulated_host_batch_forms(emu, coracle, pinned):
    """mp_proofs_deserialize_batch / mp_decks_deserialize_batch against the _dev forms, accepted and refused entries mixed, with pageable
    buffers and with buffers from mp_host_alloc"""
    eng, ser = emu("stark")
    m, n = 2, 3
    g, shuffled, proofs = cc.distinct_proofs(coracle, "stark", m, n, 3)
    canon = [ser.proof_serialize(m, n, p) for p in proofs]
    bad = bytearray(canon[1])
    bad[0] ^= 1                                                 # the first Vec length
    decks, ok = cc.defective_decks("stark", m * n, dp.pool("stark"))
    out, st = cc.run_host_batch_forms(eng, _HostMem(), "stark", m, n, b"".join([canon[0], bytes(bad), canon[2], canon[1]]), m * n, decks, pinned)
    assert [s == 0 for s in st] == ok


@pytest.mark.parametrize("curve", ["stark", "secp256k1"])
def test_emulated_refusals(emu, native, curve):
    cc.run_refusals(emu(curve)[0], _HostMem(), native.NativeError, curve)


def test_emulated_two_threads_on_one_context(emu, coracle):
    eng, ser = emu("stark")
    g, shuffled, proofs = cc.distinct_proofs(coracle, "stark", 2, 3, 5)
    cc.run_two_threads(eng, _HostMem(), "stark", 2, 3, cc.tiled(proofs, 33)[1])


def test_two_threads_under_thread_sanitizer(tmp_path):
    """tests/cpp/canonical_threads.cpp, a program of its own against the emulator's objects (the STARK units compiled with
    -fsanitize=thread and without OpenMP): one thread serialises proofs of two shapes, one deserialises, on one context; the bytes are the
    single-threaded ones and ThreadSanitizer reports nothing"""
    csrc, emu_dir = os.path.join(ROOT, "mental-poker_amd", "csrc"), os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", emu_dir])      # the other curves' objects (not instrumented, not executed here)
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=thread", "-x", "c++", "-include", os.path.join(emu_dir, "rt.hpp"),
             "-I", emu_dir, "-Wno-unknown-pragmas"]
    objs, procs = [], []
    for unit in ("capi", "curve_stark", "curve_stark_msm"):
        objs.append(str(tmp_path / (unit + ".o")))
        procs.append(subprocess.Popen(flags + ["-c", os.path.join(csrc, unit + ".hip"), "-o", objs[-1]]))
    for p in procs:
        assert p.wait() == 0
    others = [os.path.join(emu_dir, "_obj", u + ".o") for u in ("curve_bn254", "curve_secp256k1", "curve_bls12_377", "curve_bn254_msm",
                                                               "curve_secp256k1_msm", "curve_bls12_377_msm")]
    exe = str(tmp_path / "canonical_threads")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "canonical_threads.cpp")] + objs + others + ["-fopenmp", "-pthread", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 second_deadlock_stack=1", OMP_NUM_THREADS="1"))
    err = out.stderr.decode()
    assert out.returncode == 0, err[-4000:]
    assert "ThreadSanitizer" not in err, err[:6000]
    assert "canonical threads ok" in out.stdout.decode()
