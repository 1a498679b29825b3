"""Coalescing of the single-proof entry points (mp_set_coalesce, include/mpshuffle.h) under ThreadSanitizer: the library's threading
contract with the request queues in the path.  CPU test: the engine's kernel bodies run as plain loops (tools/hostemu, a development aid
that is never shipped), compiled WITHOUT OpenMP here so that the sanitizer sees every access, as tests/test_threads_tsan.py builds them.
The scenarios (tests/cpp/coalesce_threads.cpp, STARK curve, m = 2, n = 3): 8 threads released by one barrier on one table get the bytes of
the single-threaded uncoalesced run in at most 2 batched calls per queue; a tampered proof, a non-permutation and an off-curve card inside
batches get exactly their own uncoalesced results; keyed calls with 3 keys on a keyless table give the bytes of tables created with those
keys; a lone caller does not wait for requests that never come; coalescing switched on and off while calls are queued changes no result;
a third thread calls setters and the locked getters throughout.  The same driver runs on the HIP library in tests/test_gpu_coalesce.py."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "mental-poker_amd", "csrc")
EMU = os.path.join(ROOT, "tools", "hostemu")


def test_coalesced_single_proofs_under_thread_sanitizer(tmp_path):
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
    exe = str(tmp_path / "coalesce_threads")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coalesce_threads.cpp")] + objs + others + ["-fopenmp", "-pthread", "-o", exe])
    out = subprocess.run([exe, "tsan"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 second_deadlock_stack=1", OMP_NUM_THREADS="1"))
    err = out.stderr.decode()
    assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
    assert "ThreadSanitizer" not in err, err[:6000]
    assert "coalesce ok" in out.stdout.decode()
