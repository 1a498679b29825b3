"""The device pool (mp_pool_*, include/mpshuffle.h) under ThreadSanitizer: worker threads, the pool's lock, shared fixed-base tables and
the hand-back of error texts.  CPU test, built exactly as tests/test_coalesce_tsan.py builds its driver: the engine's kernel bodies run as
plain loops (tools/hostemu, a development aid that is never shipped), the STARK units compiled WITHOUT OpenMP and with -fsanitize=thread,
a stand-alone executable with its own main.  The emulator has one device, so the pool is {0, 0, 0}: three lanes that share one set of
fixed-base tables.  The scenarios are listed at the top of tests/cpp/pool_threads.cpp; the same driver runs on the HIP library in
tests/test_gpu_pool.py."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "mental-poker_amd", "csrc")
EMU = os.path.join(ROOT, "tools", "hostemu")


def test_pool_under_thread_sanitizer(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])          # the other curves' objects (not instrumented, not executed here)
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=thread", "-x", "c++", "-include", os.path.join(EMU, "rt.hpp"), "-I", EMU,
             "-Wno-unknown-pragmas"]
    objs, procs = [], []
    for unit in ("capi", "curve_stark", "curve_stark_msm"):
        obj = str(tmp_path / (unit + ".o"))
        procs.append(subprocess.Popen(flags + ["-c", os.path.join(CSRC, unit + ".hip"), "-o", obj]))
        objs.append(obj)
    for p in procs:
        assert p.wait() == 0
    others = [os.path.join(EMU, "_obj", u + ".o") for u in ("curve_bn254", "curve_secp256k1", "curve_bls12_377", "curve_bn254_msm",
                                                           "curve_secp256k1_msm", "curve_bls12_377_msm")]
    exe = str(tmp_path / "pool_threads")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pool_threads.cpp")] + objs + others + ["-fopenmp", "-pthread", "-o", exe])
    out = subprocess.run([exe, "tsan"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 second_deadlock_stack=1", OMP_NUM_THREADS="1"))
    err = out.stderr.decode()
    assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
    assert "ThreadSanitizer" not in err, err[:6000]
    assert "pool ok" in out.stdout.decode()
