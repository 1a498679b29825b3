"""ctypes binding of libmpshuffle.so (include/mpshuffle.h).  Plumbing only: bytes in, bytes out.

The library is the HIP engine; there is no CPU path.  `load()` raises if the shared object is missing
and `Engine(...)` raises `NoDeviceError` if no MI355X is visible.
"""
import ctypes
import os
import subprocess
import weakref

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmpshuffle.so")
ROOT = os.path.dirname(HERE)

CURVE_IDS = {"stark": 0, "bn254": 1, "secp256k1": 2, "bls12_377": 3}
MP_ERR_BAD_ENCODING, MP_ERR_BAD_PERMUTATION, MP_ERR_BAD_ARGUMENT, MP_ERR_NO_DEVICE, MP_ERR_INTERNAL = -1, -2, -3, -4, -5
CHAIN_PIECES_WHOLE, CHAIN_PIECES_BINARY = 0, 1

SYMBOLS = [
    "mp_ctx_create", "mp_ctx_destroy", "mp_last_error", "mp_check_name", "mp_proof_size", "mp_params_size",
    "mp_point_size", "mp_proof_size_curve", "mp_params_size_curve", "mp_set_merged_verify", "mp_set_subgroup_check", "mp_set_bucket_min", "mp_set_bucket_bits", "mp_set_bucket_split", "mp_set_validated", "mp_deck_validate_dev", "mp_set_chain_max_links", "mp_set_chain_group", "mp_set_chain_slice", "mp_chain_group_size", "mp_chain_last_slice", "mp_set_transcript_lanes", "mp_set_group_lanes", "mp_set_work_split", "mp_set_group_verify", "mp_group_size", "mp_set_group_refine", "mp_reverified_count", "mp_set_group_adapt", "mp_set_pipeline", "mp_set_plan_params", "mp_set_plan_thresholds", "mp_set_toom_cook", "mp_host_alloc", "mp_host_free", "mp_set_io_chunk", "mp_io_schedule","mp_shuffle_and_remask_batch_keys", "mp_table_create_params",
    "mp_verify_shuffle_batch_keys", "mp_shuffle_and_remask_batch_keys_dev", "mp_verify_shuffle_batch_keys_dev",
    "mp_keyset_create", "mp_keyset_destroy", "mp_keyset_size", "mp_shuffle_and_remask_batch_keyset_dev", "mp_verify_shuffle_batch_keyset_dev",
    "mp_keyset_create_empty", "mp_keyset_live", "mp_keyset_update", "mp_keyset_update_dev", "mp_keyset_clear",
    "mp_shuffle_and_remask_batch_seeded_keyset_dev", "mp_verify_shuffle_chain_ragged_keyset", "mp_verify_shuffle_chain_ragged_keyset_dev",
    "mp_mask_batch_keyset", "mp_verify_mask_batch_keyset", "mp_verify_mask_batch_keyset_dev", "mp_keyset_seat_ragged_batch",
    "mp_setup", "mp_table_create", "mp_table_create_ex", "mp_table_window_bits", "mp_table_destroy", "mp_shuffle_and_remask", "mp_verify_shuffle",
    "mp_shuffle_and_remask_keyed", "mp_verify_shuffle_keyed", "mp_set_coalesce", "mp_coalesce_stats",
    "mp_shuffle_and_remask_batch", "mp_verify_shuffle_batch", "mp_shuffle_and_remask_batch_dev",
    "mp_verify_shuffle_batch_dev", "mp_verify_shuffle_chain", "mp_verify_shuffle_chain_dev", "mp_sync", "mp_reserve", "mp_set_latency_batch", "mp_remask_batch", "mp_msm", "mp_commit_batch",
    "mp_profile_enable", "mp_profile_report", "mp_work_census", "mp_plan_stats", "mp_sigma_prove_batch",
    "mp_sigma_verify_batch", "mp_blake2s", "mp_reveal_batch", "mp_unmask_batch", "mp_unmask_batch_dev",
    "mp_mask_batch", "mp_verify_mask_batch", "mp_verify_mask_batch_dev", "mp_aggregate_keys_batch",
    "mp_set_sigma_screen", "mp_sigma_screen_stats",
    "mp_reveal_ragged_batch", "mp_unmask_ragged_batch", "mp_unmask_ragged_batch_dev", "mp_aggregate_keys_ragged_batch",
    "mp_verify_shuffle_chain_ragged", "mp_verify_shuffle_chain_ragged_dev", "mp_set_chain_pieces", "mp_chain_ragged_stats",
    "mp_sample_secrets_batch", "mp_sample_secrets_batch_dev", "mp_shuffle_and_remask_batch_seeded", "mp_shuffle_and_remask_batch_seeded_dev",
    "mp_keygen_batch",
    "mp_pool_create", "mp_pool_destroy", "mp_pool_size", "mp_pool_member_ctx", "mp_pool_table_create", "mp_pool_table_destroy",
    "mp_pool_table_member", "mp_pool_set_min_shard", "mp_pool_shuffle_and_remask_batch", "mp_pool_verify_shuffle_batch", "mp_pool_stats",
    "mp_pool_member_stats",
    "mp_serialized_point_size", "mp_serialized_deck_size", "mp_serialized_params_size", "mp_serialized_proof_size",
    "mp_points_serialize", "mp_points_deserialize", "mp_deck_serialize", "mp_deck_deserialize", "mp_params_serialize",
    "mp_params_deserialize", "mp_proof_serialize", "mp_proof_deserialize", "mp_points_deserialize_dev", "mp_deck_deserialize_dev",
    "mp_points_serialize_dev", "mp_deck_serialize_dev", "mp_proof_serialize_dev", "mp_proof_deserialize_dev",
    "mp_decks_deserialize_batch", "mp_proofs_deserialize_batch",
]


class NativeError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("mpshuffle error %d: %s" % (code, text))
        self.code = code


class NoDeviceError(NativeError):
    pass


SOURCES = ["capi.hip"] + [f % c for c in ("stark", "bn254", "secp256k1", "bls12_377") for f in ("curve_%s.hip", "curve_%s_msm.hip")]


def build(verbose=False):
    """compile the HIP engine for gfx950 in-tree -> mental-poker_amd/libmpshuffle.so
    (one translation unit per curve, compiled in parallel, objects cached under csrc/_obj), and beside it the test tools
    tools/quadcheck/quad_check, tools/primcheck/libprimcheck.so, tools/fscheck/libfscheck.so and tools/digitcheck/libdigitcheck.so"""
    from concurrent.futures import ThreadPoolExecutor
    csrc = os.path.join(HERE, "csrc")
    objdir = os.path.join(csrc, "_obj")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    headers.append(os.path.join(ROOT, "include", "mpshuffle.h"))
    hdr_time = max(os.path.getmtime(h) for h in headers)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # max-ilp scheduling: +0.8 % on the MSM kernels in a back-to-back A/B (interleaves the mad chains with the carry handling)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-sched-strategy=max-ilp",
             "-mllvm", "-pragma-unroll-threshold=1000000"]   # the 14-limb products (27 columns x 14) must unroll completely: rolled, their operands are re-read from the stack with dynamic indices

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        spath = os.path.join(csrc, src)
        if os.path.exists(obj) and os.path.getmtime(obj) >= max(hdr_time, os.path.getmtime(spath)):
            return obj, False
        cmd = [hipcc] + flags + ["-c", spath, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj, True

    def compile_check():
        """tools/quadcheck/quad_check: on-device unit test of the four-lane group law (kernels_quad.hpp) against the one-lane one;
        built here so that it travels to the GPU box with the library (tests/test_gpu_parity.py runs it).  A test tool: its failure to
        build is reported, never the library's"""
        src = os.path.join(ROOT, "tools", "quadcheck", "quad_check.hip")
        exe = os.path.join(ROOT, "tools", "quadcheck", "quad_check")
        if not os.path.exists(src) or (os.path.exists(exe) and os.path.getmtime(exe) >= max(hdr_time, os.path.getmtime(src))):
            return
        cmd = [hipcc] + [f for f in flags if f != "-fPIC"] + ["-I", csrc, src, "-o", exe]
        if verbose:
            print(" ".join(cmd), flush=True)
        try:
            subprocess.check_call(cmd)
        except (subprocess.CalledProcessError, OSError) as e:
            print("warning: tools/quadcheck/quad_check did not build (%s); the library is unaffected" % e, flush=True)

    probe_dir = os.path.join(ROOT, "tools", "primcheck")
    probe_src = os.path.join(probe_dir, "prim_check.hip")
    probe_lib = os.path.join(probe_dir, "libprimcheck.so")

    fs_dir = os.path.join(ROOT, "tools", "fscheck")
    fs_src = os.path.join(fs_dir, "fs_check.hip")
    fs_lib = os.path.join(fs_dir, "libfscheck.so")

    dg_dir = os.path.join(ROOT, "tools", "digitcheck")
    dg_src = os.path.join(dg_dir, "digit_check.hip")
    dg_lib = os.path.join(dg_dir, "libdigitcheck.so")

    def compile_probe(curve_id, probe_dir=probe_dir, probe_src=probe_src, stem="prim_check", macro="PRIM_CURVE"):
        """tools/primcheck/prim_check.hip: one field / group operation per lane, for tests/test_gpu_primitives.py; tools/fscheck/fs_check.hip:
        the Fiat-Shamir layer and the screening weights, for tests/test_gpu_fs.py; tools/digitcheck/digit_check.hip: the scalar recodings, for
        tests/test_gpu_digit.py.  One object per curve, with EXACTLY the library's flags
        (the code generation under test is the library's); shared objects of their own, nothing of them goes into libmpshuffle.so"""
        os.makedirs(os.path.join(probe_dir, "_obj"), exist_ok=True)
        obj = os.path.join(probe_dir, "_obj", "%s_%d.o" % (stem, curve_id))
        if os.path.exists(obj) and os.path.getmtime(obj) >= max(hdr_time, os.path.getmtime(probe_src)):
            return obj, False
        cmd = [hipcc] + flags + ["-D%s=%d" % (macro, curve_id), "-I", csrc, "-c", probe_src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj, True

    # The library's translation units are queued first and the library is linked as soon as THEY are done; the probe's objects
    # share the pool and are collected afterwards, so the library never waits for the probe's link (they do compete for cores).
    ex = ThreadPoolExecutor(max_workers=len(SOURCES) + 1 + 3 * len(CURVE_IDS))
    try:
        res_f = [ex.submit(compile_one, s) for s in SOURCES]
        chk = ex.submit(compile_check)
        probe_f = [ex.submit(compile_probe, k) for k in sorted(CURVE_IDS.values())] if os.path.exists(probe_src) else []
        fs_f = [ex.submit(compile_probe, k, fs_dir, fs_src, "fs_check", "FS_CURVE") for k in sorted(CURVE_IDS.values())] if os.path.exists(fs_src) else []
        dg_f = [ex.submit(compile_probe, k, dg_dir, dg_src, "digit_check", "DIGIT_CURVE") for k in sorted(CURVE_IDS.values())] if os.path.exists(dg_src) else []
        res = [f.result() for f in res_f]
        objs = [r[0] for r in res]
        if any(r[1] for r in res) or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(o) for o in objs):
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", LIB_PATH] + objs      # serialize_host.hpp uses std::thread
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        chk.result()
        probe = [f.result() for f in probe_f]      # (a probe that does not compile fails the build: its tests do not skip)
        fs_probe = [f.result() for f in fs_f]
        dg_probe = [f.result() for f in dg_f]
    finally:
        ex.shutdown(wait=True)
    for objs_p, lib_p in ((probe, probe_lib), (fs_probe, fs_lib), (dg_probe, dg_lib)):
        if objs_p and (any(r[1] for r in objs_p) or not os.path.exists(lib_p)
                       or os.path.getmtime(lib_p) < max(os.path.getmtime(r[0]) for r in objs_p)):
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_p] + [r[0] for r in objs_p]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    # multiply-add counts of the compiled field arithmetic (bench.py's int_mul roofline): regenerated with the library
    mc = os.path.join(HERE, "mad_counts.json")
    gen = os.path.join(ROOT, "tools", "gen_mad_counts.py")
    if os.path.exists(gen) and (not os.path.exists(mc) or os.path.getmtime(mc) < max(hdr_time, os.path.getmtime(gen))):
        import importlib.util
        spec = importlib.util.spec_from_file_location("gen_mad_counts", gen)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.main([f for f in flags if f != "-fPIC"])
    return LIB_PATH


def bind(cdll):
    """declare prototypes on an already opened library"""
    c = ctypes
    u8p, u32p, i32p = c.c_void_p, c.c_void_p, c.c_void_p
    cdll.mp_ctx_create.argtypes = [c.c_int, c.c_int, c.POINTER(c.c_void_p)]
    cdll.mp_ctx_destroy.argtypes = [c.c_void_p]
    cdll.mp_ctx_destroy.restype = None
    cdll.mp_last_error.restype = c.c_char_p
    cdll.mp_check_name.argtypes = [c.c_int]
    cdll.mp_check_name.restype = c.c_char_p
    cdll.mp_proof_size.argtypes = [c.c_uint32, c.c_uint32]
    cdll.mp_proof_size.restype = c.c_size_t
    cdll.mp_params_size.argtypes = [c.c_uint32]
    cdll.mp_params_size.restype = c.c_size_t
    cdll.mp_set_merged_verify.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_set_subgroup_check.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_set_bucket_min.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_set_bucket_bits.argtypes = [c.c_void_p, c.c_uint32]
    cdll.mp_set_bucket_split.argtypes = [c.c_void_p, c.c_uint32]
    cdll.mp_set_validated.argtypes = [c.c_void_p, c.c_uint32]
    cdll.mp_deck_validate_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    cdll.mp_set_toom_cook.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_set_chain_max_links.argtypes = [c.c_void_p, c.c_uint32]
    cdll.mp_set_chain_group.argtypes = [c.c_void_p, c.c_uint32]
    cdll.mp_set_chain_slice.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_chain_group_size.argtypes = [c.c_void_p, c.c_size_t, c.c_uint32, c.c_int]
    cdll.mp_chain_group_size.restype = c.c_uint32
    cdll.mp_chain_last_slice.argtypes = [c.c_void_p]
    cdll.mp_chain_last_slice.restype = c.c_size_t
    cdll.mp_set_transcript_lanes.argtypes = [c.c_void_p, c.c_uint32]
    cdll.mp_set_group_lanes.argtypes = [c.c_void_p, c.c_uint32]
    cdll.mp_set_work_split.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_set_group_verify.argtypes = [c.c_void_p, c.c_uint32, c.c_size_t]
    cdll.mp_group_size.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_group_size.restype = c.c_uint32
    cdll.mp_set_group_refine.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32]
    cdll.mp_reverified_count.argtypes = [c.c_void_p]
    cdll.mp_set_group_adapt.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_reverified_count.restype = c.c_uint64
    cdll.mp_set_pipeline.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_set_plan_params.argtypes = [c.c_void_p, c.c_int] + [c.c_uint32] * 5
    cdll.mp_set_plan_thresholds.argtypes = [c.c_void_p] + [c.c_size_t] * 5
    cdll.mp_set_io_chunk.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_io_schedule.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.POINTER(c.c_size_t), c.c_size_t]
    cdll.mp_io_schedule.restype = c.c_size_t
    cdll.mp_host_alloc.argtypes = [c.c_size_t]
    cdll.mp_host_alloc.restype = c.c_void_p
    cdll.mp_host_free.argtypes = [c.c_void_p]
    cdll.mp_host_free.restype = None
    cdll.mp_point_size.argtypes = [c.c_int]
    cdll.mp_point_size.restype = c.c_size_t
    cdll.mp_proof_size_curve.argtypes = [c.c_int, c.c_uint32, c.c_uint32]
    cdll.mp_proof_size_curve.restype = c.c_size_t
    cdll.mp_params_size_curve.argtypes = [c.c_int, c.c_uint32]
    cdll.mp_params_size_curve.restype = c.c_size_t
    cdll.mp_setup.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, u8p, u8p]
    cdll.mp_table_create.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, u8p, u8p, c.POINTER(c.c_void_p)]
    cdll.mp_table_create_ex.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, u8p, u8p, c.c_uint32, c.POINTER(c.c_void_p)]
    cdll.mp_table_window_bits.argtypes = [c.c_void_p]
    cdll.mp_table_window_bits.restype = c.c_uint32
    cdll.mp_table_destroy.argtypes = [c.c_void_p]
    cdll.mp_table_destroy.restype = None
    cdll.mp_shuffle_and_remask.argtypes = [c.c_void_p, u8p, u8p, u32p, u8p, u8p, u8p]
    cdll.mp_verify_shuffle.argtypes = [c.c_void_p, u8p, u8p, u8p, c.c_size_t]
    cdll.mp_shuffle_and_remask_keyed.argtypes = [c.c_void_p, u8p, u8p, u8p, u32p, u8p, u8p, u8p]
    cdll.mp_verify_shuffle_keyed.argtypes = [c.c_void_p, u8p, u8p, u8p, u8p, c.c_size_t]
    cdll.mp_set_coalesce.argtypes = [c.c_void_p, c.c_size_t, c.c_uint32]
    cdll.mp_coalesce_stats.argtypes = [c.c_void_p, c.POINTER(c.c_uint64)]
    cdll.mp_shuffle_and_remask_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_verify_shuffle_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p, i32p]
    cdll.mp_shuffle_and_remask_batch_dev.argtypes = [c.c_void_p, c.c_size_t] + [c.c_void_p] * 7
    cdll.mp_verify_shuffle_batch_dev.argtypes = [c.c_void_p, c.c_size_t] + [c.c_void_p] * 4
    cdll.mp_table_create_params.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, u8p, c.c_uint32, c.POINTER(c.c_void_p)]
    cdll.mp_shuffle_and_remask_batch_keys.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_verify_shuffle_batch_keys.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p, u8p, i32p]
    cdll.mp_shuffle_and_remask_batch_keys_dev.argtypes = [c.c_void_p, c.c_size_t] + [c.c_void_p] * 8
    cdll.mp_verify_shuffle_batch_keys_dev.argtypes = [c.c_void_p, c.c_size_t] + [c.c_void_p] * 5
    cdll.mp_keyset_create.argtypes = [c.c_void_p, c.c_size_t, u8p, c.POINTER(c.c_void_p)]
    cdll.mp_keyset_destroy.argtypes = [c.c_void_p]
    cdll.mp_keyset_destroy.restype = None
    cdll.mp_keyset_size.argtypes = [c.c_void_p]
    cdll.mp_keyset_size.restype = c.c_size_t
    cdll.mp_keyset_create_empty.argtypes = [c.c_void_p, c.c_size_t, c.POINTER(c.c_void_p)]
    cdll.mp_keyset_live.argtypes = [c.c_void_p]
    cdll.mp_keyset_live.restype = c.c_size_t
    cdll.mp_mask_batch_keyset.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_size_t, u32p, u8p, u8p, u8p, u8p, u8p, i32p]
    cdll.mp_verify_mask_batch_keyset.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_size_t, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_verify_mask_batch_keyset_dev.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_size_t] + [c.c_void_p] * 5
    cdll.mp_keyset_seat_ragged_batch.argtypes = [c.c_void_p, c.c_size_t, u32p, u32p, u8p, u8p, u8p, u8p, i32p, i32p, i32p]
    cdll.mp_keyset_update.argtypes = [c.c_void_p, c.c_size_t, u32p, u8p, i32p]
    cdll.mp_keyset_update_dev.argtypes = [c.c_void_p, c.c_size_t, u32p, c.c_void_p, c.c_void_p]
    cdll.mp_keyset_clear.argtypes = [c.c_void_p, c.c_size_t, u32p]
    cdll.mp_shuffle_and_remask_batch_seeded_keyset_dev.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t] + [c.c_void_p] * 8
    cdll.mp_verify_shuffle_chain_ragged_keyset.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, u32p, u32p, u8p, u8p, i32p]
    cdll.mp_verify_shuffle_chain_ragged_keyset_dev.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, u32p] + [c.c_void_p] * 4
    cdll.mp_shuffle_and_remask_batch_keyset_dev.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t] + [c.c_void_p] * 8
    cdll.mp_verify_shuffle_batch_keyset_dev.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t] + [c.c_void_p] * 5
    cdll.mp_verify_shuffle_chain.argtypes = [c.c_void_p, c.c_size_t, c.c_uint32, u8p, u8p, u8p, i32p]
    cdll.mp_verify_shuffle_chain_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_uint32] + [c.c_void_p] * 4
    cdll.mp_verify_shuffle_chain_ragged.argtypes = [c.c_void_p, c.c_size_t, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_verify_shuffle_chain_ragged_dev.argtypes = [c.c_void_p, c.c_size_t, u32p] + [c.c_void_p] * 4
    cdll.mp_set_chain_pieces.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_chain_ragged_stats.argtypes = [c.c_void_p, c.POINTER(c.c_uint64)]
    cdll.mp_sync.argtypes = [c.c_void_p]
    cdll.mp_reserve.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_set_latency_batch.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_remask_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p]
    cdll.mp_msm.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, u8p, u8p, u8p]
    cdll.mp_commit_batch.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, u8p, u8p, u8p]
    cdll.mp_profile_enable.argtypes = [c.c_void_p, c.c_int]
    cdll.mp_profile_report.argtypes = [c.c_void_p, c.c_char_p, c.c_size_t]
    cdll.mp_work_census.argtypes = [c.c_void_p] + [c.POINTER(c.c_uint64)] * 4
    cdll.mp_plan_stats.argtypes = [c.c_void_p, c.POINTER(c.c_uint64)]
    cdll.mp_sigma_prove_batch.argtypes = [c.c_void_p, c.c_size_t, c.c_uint32, u8p, u8p, u8p, u8p, u8p, u8p, i32p]
    cdll.mp_sigma_verify_batch.argtypes = [c.c_void_p, c.c_size_t, c.c_uint32, u8p, u8p, u8p, u8p, i32p]
    cdll.mp_blake2s.argtypes = [u8p, c.c_size_t, u8p]
    cdll.mp_reveal_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, c.c_size_t, u8p, c.c_uint32, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_unmask_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, c.c_size_t, u8p, c.c_uint32, u32p, u8p, u8p, c.c_size_t, u8p, u8p, u32p, i32p, i32p]
    cdll.mp_unmask_batch_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint32] + [c.c_void_p] * 3 + [c.c_size_t] + [c.c_void_p] * 5
    cdll.mp_reveal_ragged_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, c.c_size_t, u8p, u32p, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_unmask_ragged_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, c.c_size_t, u8p, u32p, u32p, u8p, u8p, c.c_size_t, u8p, u8p, u32p, i32p, i32p]
    cdll.mp_unmask_ragged_batch_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, u32p] + [c.c_void_p] * 3 + [c.c_size_t] + [c.c_void_p] * 5
    cdll.mp_aggregate_keys_ragged_batch.argtypes = [c.c_void_p, c.c_size_t, u32p, u8p, u8p, u8p, u8p, i32p, i32p]
    cdll.mp_mask_batch.argtypes = [c.c_void_p, c.c_int, c.c_size_t, u8p, c.c_size_t, u32p, u8p, u8p, u8p, u8p, u8p, i32p]
    cdll.mp_verify_mask_batch.argtypes = [c.c_void_p, c.c_int, c.c_size_t, u8p, c.c_size_t, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_verify_mask_batch_dev.argtypes = [c.c_void_p, c.c_int, c.c_size_t, c.c_void_p, c.c_size_t] + [c.c_void_p] * 5
    cdll.mp_aggregate_keys_batch.argtypes = [c.c_void_p, c.c_size_t, c.c_uint32, u8p, u8p, u8p, u8p, i32p, i32p]
    cdll.mp_set_sigma_screen.argtypes = [c.c_void_p, c.c_uint32, c.c_size_t]
    cdll.mp_sample_secrets_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, c.c_uint32, c.c_uint32, u8p, u32p]
    cdll.mp_sample_secrets_batch_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p]
    cdll.mp_shuffle_and_remask_batch_seeded.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p, u8p, u8p, i32p, u32p, u8p]
    cdll.mp_shuffle_and_remask_batch_seeded_dev.argtypes = [c.c_void_p, c.c_size_t] + [c.c_void_p] * 8
    cdll.mp_keygen_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p, u8p, u8p, i32p]
    cdll.mp_sigma_screen_stats.argtypes = [c.c_void_p, c.POINTER(c.c_uint64)]
    cdll.mp_pool_create.argtypes = [c.c_int, c.c_size_t, c.POINTER(c.c_int), c.POINTER(c.c_void_p)]
    cdll.mp_pool_destroy.argtypes = [c.c_void_p]
    cdll.mp_pool_destroy.restype = None
    cdll.mp_pool_size.argtypes = [c.c_void_p]
    cdll.mp_pool_size.restype = c.c_size_t
    cdll.mp_pool_member_ctx.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_pool_member_ctx.restype = c.c_void_p
    cdll.mp_pool_table_create.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, u8p, u8p, c.c_uint32, c.POINTER(c.c_void_p)]
    cdll.mp_pool_table_destroy.argtypes = [c.c_void_p]
    cdll.mp_pool_table_destroy.restype = None
    cdll.mp_pool_table_member.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_pool_table_member.restype = c.c_void_p
    cdll.mp_pool_set_min_shard.argtypes = [c.c_void_p, c.c_size_t]
    cdll.mp_pool_shuffle_and_remask_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p, u32p, u8p, u8p, u8p, i32p]
    cdll.mp_pool_verify_shuffle_batch.argtypes = [c.c_void_p, c.c_size_t, u8p, u8p, u8p, u8p, i32p]
    cdll.mp_pool_stats.argtypes = [c.c_void_p, c.POINTER(c.c_uint64)]
    cdll.mp_pool_member_stats.argtypes = [c.c_void_p, c.c_size_t, c.POINTER(c.c_uint64)]
    for fn, at in (("mp_serialized_point_size", [c.c_int]), ("mp_serialized_deck_size", [c.c_int, c.c_size_t]),
                   ("mp_serialized_params_size", [c.c_int, c.c_uint32]), ("mp_serialized_proof_size", [c.c_int, c.c_uint32, c.c_uint32])):
        getattr(cdll, fn).argtypes = at
        getattr(cdll, fn).restype = c.c_size_t
    cdll.mp_points_serialize.argtypes = [c.c_int, c.c_size_t, u8p, u8p]
    cdll.mp_points_deserialize.argtypes = [c.c_int, c.c_size_t, u8p, u8p]
    cdll.mp_deck_serialize.argtypes = [c.c_int, c.c_size_t, u8p, u8p]
    cdll.mp_deck_deserialize.argtypes = [c.c_int, u8p, c.c_size_t, c.c_size_t, u8p, c.POINTER(c.c_size_t)]
    cdll.mp_params_serialize.argtypes = [c.c_int, c.c_uint32, c.c_uint32, u8p, u8p]
    cdll.mp_params_deserialize.argtypes = [c.c_int, u8p, c.c_size_t, c.c_size_t, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32), u8p]
    cdll.mp_points_deserialize_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    cdll.mp_deck_deserialize_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    cdll.mp_proof_serialize.argtypes = [c.c_int, c.c_uint32, c.c_uint32, u8p, u8p]
    cdll.mp_proof_deserialize.argtypes = [c.c_int, c.c_uint32, c.c_uint32, u8p, c.c_size_t, u8p]
    cdll.mp_points_serialize_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    cdll.mp_deck_serialize_dev.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    cdll.mp_proof_serialize_dev.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    cdll.mp_proof_deserialize_dev.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    cdll.mp_decks_deserialize_batch.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, u8p, u8p, i32p]
    cdll.mp_proofs_deserialize_batch.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_size_t, u8p, u8p, i32p]
    return cdll


_LIB = None


def load():
    """open libmpshuffle.so (raises if it was not built: there is no fallback)"""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmpshuffle.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                              "the engine has no CPU fallback")
        _LIB = bind(ctypes.CDLL(LIB_PATH))
    return _LIB


def _in(b):
    b = bytes(b)
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


class Serializer:
    """include/mpshuffle.h "canonical serialisation": arkworks-0.3 compressed bytes <-> wire v1.  Host work in libmpshuffle.so;
    needs no GPU and no context."""

    def __init__(self, curve, lib=None):
        self.lib, self.cid, self.curve = (lib if lib is not None else load()), CURVE_IDS[curve], curve
        self.pb = self.lib.mp_point_size(self.cid)
        self.cb = self.lib.mp_serialized_point_size(self.cid)

    def _chk(self, rc):
        if rc != 0:
            raise NativeError(rc, self.lib.mp_last_error().decode())

    def proof_serialized_size(self, m, n):
        return self.lib.mp_serialized_proof_size(self.cid, m, n)

    def points_serialize(self, wire):
        k = len(wire) // self.pb
        if k * self.pb != len(wire):
            raise NativeError(MP_ERR_BAD_ARGUMENT, "whole wire points expected")
        out = (ctypes.c_uint8 * max(k * self.cb, 1))()
        self._chk(self.lib.mp_points_serialize(self.cid, k, _in(wire), out))
        return bytes(out)[:k * self.cb]

    def points_deserialize(self, data):
        k = len(data) // self.cb
        if k * self.cb != len(data):
            raise NativeError(MP_ERR_BAD_ENCODING, "whole compressed points expected")
        out = (ctypes.c_uint8 * max(k * self.pb, 1))()
        self._chk(self.lib.mp_points_deserialize(self.cid, k, _in(data), out))
        return bytes(out)[:k * self.pb]

    def deck_serialize(self, wire):
        k = len(wire) // (2 * self.pb)
        if 2 * k * self.pb != len(wire):
            raise NativeError(MP_ERR_BAD_ARGUMENT, "whole cards expected")
        out = (ctypes.c_uint8 * self.lib.mp_serialized_deck_size(self.cid, k))()
        self._chk(self.lib.mp_deck_serialize(self.cid, k, _in(wire), out))
        return bytes(out)

    def deck_deserialize(self, data):
        cap = max(len(data) // (2 * self.cb), 1)
        out = (ctypes.c_uint8 * (cap * 2 * self.pb))()
        k = ctypes.c_size_t()
        self._chk(self.lib.mp_deck_deserialize(self.cid, _in(data), len(data), cap, out, ctypes.byref(k)))
        return bytes(out)[:k.value * 2 * self.pb]

    def params_serialize(self, m, n, raw):
        if len(raw) != self.pb * (n + 3):
            raise NativeError(MP_ERR_BAD_ARGUMENT, "parameters: wrong length")
        out = (ctypes.c_uint8 * self.lib.mp_serialized_params_size(self.cid, n))()
        self._chk(self.lib.mp_params_serialize(self.cid, m, n, _in(raw), out))
        return bytes(out)

    def params_deserialize(self, data):
        cap = max(len(data) // self.cb, 1)
        out = (ctypes.c_uint8 * (self.pb * (cap + 3)))()
        m, n = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self.lib.mp_params_deserialize(self.cid, _in(data), len(data), cap, ctypes.byref(m), ctypes.byref(n), out))
        return m.value, n.value, bytes(out)[:self.pb * (n.value + 3)]

    def proof_serialize(self, m, n, wire):
        if len(wire) != self.lib.mp_proof_size_curve(self.cid, m, n):
            raise NativeError(MP_ERR_BAD_ARGUMENT, "proof: wrong length")
        out = (ctypes.c_uint8 * self.proof_serialized_size(m, n))()
        self._chk(self.lib.mp_proof_serialize(self.cid, m, n, _in(wire), out))
        return bytes(out)

    def proof_deserialize(self, m, n, data):
        out = (ctypes.c_uint8 * self.lib.mp_proof_size_curve(self.cid, m, n))()
        self._chk(self.lib.mp_proof_deserialize(self.cid, m, n, _in(data), len(data), out))
        return bytes(out)


class Engine:
    """one mp_ctx (GPU + stream + curve)"""

    def __init__(self, curve="stark", device=0, lib=None):
        self.lib = lib if lib is not None else load()
        self.curve = curve
        h = ctypes.c_void_p()
        rc = self.lib.mp_ctx_create(CURVE_IDS[curve], device, ctypes.byref(h))
        if rc != 0:
            text = self.lib.mp_last_error().decode()
            raise (NoDeviceError if rc == MP_ERR_NO_DEVICE else NativeError)(rc, text)
        self.h = h
        self.point_bytes = self.lib.mp_point_size(CURVE_IDS[curve])     # 64; 96 on bls12_377

    @classmethod
    def borrowed(cls, curve, h, lib):
        """the context of a pool member (Pool.engine): the pool owns it, close() only forgets the handle"""
        self = cls.__new__(cls)
        self.lib, self.curve, self.h, self._borrowed = lib, curve, ctypes.c_void_p(h), True
        self.point_bytes = lib.mp_point_size(CURVE_IDS[curve])
        return self

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.mp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise NativeError(rc, self.lib.mp_last_error().decode())
        return rc

    def check_name(self, code):
        return self.lib.mp_check_name(code).decode()

    def proof_size(self, m, n):
        return self.lib.mp_proof_size_curve(CURVE_IDS[self.curve], m, n)

    def blake2s(self, data):
        out = (ctypes.c_uint8 * 32)()
        self._chk(self.lib.mp_blake2s(_in(data), len(data), out))
        return bytes(out)

    def setup(self, m, n, seed):
        out = (ctypes.c_uint8 * self.lib.mp_params_size_curve(CURVE_IDS[self.curve], n))()
        self._chk(self.lib.mp_setup(self.h, m, n, _in(seed), out))
        return bytes(out)

    def table(self, m, n, params, shared_key, fb_bits=8):
        return Table(self, m, n, params, shared_key, fb_bits)

    def sync(self):
        self._chk(self.lib.mp_sync(self.h))

    def points_deserialize_dev(self, count, d_data, d_out_wire, d_status):
        """compressed arkworks points in device memory -> wire v1 in device memory; d_status: one int32 per point"""
        self._chk(self.lib.mp_points_deserialize_dev(self.h, count, d_data, d_out_wire, d_status))

    def deck_deserialize_dev(self, decks, cards, d_data, d_out_wire_decks, d_status):
        """`decks` serialised Vec<MaskedCard> of `cards` cards each (device memory) -> wire decks; d_status: one int32 per deck"""
        self._chk(self.lib.mp_deck_deserialize_dev(self.h, decks, cards, d_data, d_out_wire_decks, d_status))

    def points_serialize_dev(self, count, d_wire, d_out, d_status):
        """wire v1 points in device memory -> compressed arkworks points in device memory; d_status: one int32 per point"""
        self._chk(self.lib.mp_points_serialize_dev(self.h, count, d_wire, d_out, d_status))

    def deck_serialize_dev(self, decks, cards, d_wire_decks, d_out, d_status):
        """`decks` wire decks of `cards` cards each (device memory) -> serialised Vec<MaskedCard>; d_status: one int32 per deck"""
        self._chk(self.lib.mp_deck_serialize_dev(self.h, decks, cards, d_wire_decks, d_out, d_status))

    def proof_serialize_dev(self, m, n, B, d_proofs_wire, d_out, d_status):
        """`B` wire proofs of shape (m, n) (device memory) -> canonical proofs; d_status: one int32 per proof"""
        self._chk(self.lib.mp_proof_serialize_dev(self.h, m, n, B, d_proofs_wire, d_out, d_status))

    def proof_deserialize_dev(self, m, n, B, d_data, d_out_proofs_wire, d_status):
        """`B` canonical proofs of shape (m, n) (device memory) -> wire proofs, validated; d_status: one int32 per proof"""
        self._chk(self.lib.mp_proof_deserialize_dev(self.h, m, n, B, d_data, d_out_proofs_wire, d_status))

    def _deserialize_batch(self, call, units, in_size, out_size, data, pinned):
        """host bytes -> (wire bytes, [status per unit]) through a *_deserialize_batch entry point; pinned: stage the call's buffers in
        page-locked memory from mp_host_alloc"""
        if units < 1 or len(data) != units * in_size:
            raise NativeError(MP_ERR_BAD_ARGUMENT, "deserialize batch: %d bytes for %d units of %d" % (len(data), units, in_size))
        st = (ctypes.c_int32 * units)()
        if not pinned:
            out = (ctypes.c_uint8 * (units * out_size))()
            self._chk(call(_in(data), out, st))
            return bytes(out), list(st)
        sizes = (units * in_size, units * out_size, 4 * units)
        bufs = [self.lib.mp_host_alloc(k) for k in sizes]
        try:
            if not all(bufs):
                raise NativeError(MP_ERR_INTERNAL, "mp_host_alloc failed")
            ctypes.memmove(bufs[0], bytes(data), sizes[0])
            self._chk(call(bufs[0], bufs[1], bufs[2]))
            return ctypes.string_at(bufs[1], sizes[1]), list((ctypes.c_int32 * units).from_buffer_copy(ctypes.string_at(bufs[2], sizes[2])))
        finally:
            for b in bufs:
                if b:
                    self.lib.mp_host_free(ctypes.c_void_p(b))

    def decks_deserialize_batch(self, decks, cards, data, pinned=False):
        """`decks` serialised Vec<MaskedCard> of `cards` cards, back to back in host bytes -> (wire decks, [status per deck]); the
        conversion runs on the device (mp_decks_deserialize_batch)"""
        cid = CURVE_IDS[self.curve]
        return self._deserialize_batch(lambda i, o, s: self.lib.mp_decks_deserialize_batch(self.h, decks, cards, i, o, s), decks,
                                       self.lib.mp_serialized_deck_size(cid, cards), 2 * cards * self.point_bytes, data, pinned)

    def proofs_deserialize_batch(self, m, n, B, data, pinned=False):
        """`B` canonical proofs of shape (m, n), back to back in host bytes -> (wire proofs, [status per proof]); the conversion runs
        on the device (mp_proofs_deserialize_batch)"""
        cid = CURVE_IDS[self.curve]
        return self._deserialize_batch(lambda i, o, s: self.lib.mp_proofs_deserialize_batch(self.h, m, n, B, i, o, s), B,
                                       self.lib.mp_serialized_proof_size(cid, m, n), self.lib.mp_proof_size_curve(cid, m, n), data, pinned)

    def profile_enable(self, on=True):
        self._chk(self.lib.mp_profile_enable(self.h, 1 if on else 0))

    def profile_report(self):
        buf = ctypes.create_string_buffer(1 << 16)
        self._chk(self.lib.mp_profile_report(self.h, buf, len(buf)))
        out = {}
        self.last_profile_items = {}      # name -> threads launched (waves / (equation, window) items for the wave kernels)
        for line in buf.value.decode().splitlines():
            f = line.split()
            out[f[0]] = (int(f[1]), float(f[2]))
            if len(f) > 3:
                self.last_profile_items[f[0]] = int(f[3])
        return out


class KeySet:
    """mp_keyset: fixed-base window tables of the aggregate keys of one Table, in slots that are live or empty
    (include/mpshuffle.h, "key sets" and "key sets whose slots change").  KeySet(table, keys): one live slot per key;
    KeySet(table, capacity=n): n empty slots"""

    def __init__(self, table, keys=None, capacity=None):
        self.table, self.lib = table, table.lib
        h = ctypes.c_void_p()
        if keys is None:
            self.size = int(capacity)
            table.eng._chk(self.lib.mp_keyset_create_empty(table.h, self.size, ctypes.byref(h)))
        else:
            if len(keys) == 0 or len(keys) % table.pb:
                raise ValueError("keys: expected a whole number of %d-byte points" % table.pb)
            self.size = len(keys) // table.pb
            table.eng._chk(self.lib.mp_keyset_create(table.h, self.size, _in(keys), ctypes.byref(h)))
        self.h = h

    @staticmethod
    def _slots(slots):
        return (ctypes.c_uint32 * max(len(slots), 1))(*slots)

    def live(self):
        """the number of live slots (waits for the updates in flight)"""
        return int(self.lib.mp_keyset_live(self.h))

    def seat(self, counts, slots, keys, proofs, fs_init, want_keys=True):
        """mp_keyset_seat_ragged_batch: table k seats counts[k] players (their keys, proofs of key ownership and transcript digests, lane
        by lane) and its aggregate key goes into slot slots[k] without leaving the device
        -> (aggregate keys or None, player status, table status, slot status)"""
        t = self.table
        tables, lanes = len(counts), sum(counts)
        if len(slots) != tables:
            raise ValueError("slots: expected one slot per table")
        t._need("keys", len(keys), lanes * t.pb)
        t._need("proofs", len(proofs), lanes * (t.pb + 32))
        t._need("fs_init", len(fs_init), lanes * 32)
        first = [0]
        for n in counts:
            first.append(first[-1] + n)
        out = (ctypes.c_uint8 * max(tables * t.pb, 1))() if want_keys else None
        ps, ts, ss = (ctypes.c_int32 * max(lanes, 1))(), (ctypes.c_int32 * max(tables, 1))(), (ctypes.c_int32 * max(tables, 1))()
        t.eng._chk(self.lib.mp_keyset_seat_ragged_batch(self.h, tables, (ctypes.c_uint32 * (tables + 1))(*first), self._slots(slots), _in(keys),
                                                        _in(proofs), _in(fs_init), out, ps, ts, ss))
        return (bytes(out)[:tables * t.pb] if want_keys else None), list(ps)[:lanes], list(ts)[:tables], list(ss)[:tables]

    def update(self, slots, keys):
        """slot slots[i] <- wire point i of keys (host bytes) -> status words: 0 = live with that key, MP_ERR_BAD_ENCODING = the key
        was refused and the slot is EMPTY now.  A malformed slots list raises NativeError (MP_ERR_BAD_ARGUMENT): nothing has changed"""
        if len(keys) != len(slots) * self.table.pb:
            raise ValueError("keys: expected %d bytes" % (len(slots) * self.table.pb))
        st = (ctypes.c_int32 * max(len(slots), 1))()
        self.table.eng._chk(self.lib.mp_keyset_update(self.h, len(slots), self._slots(slots), _in(keys), st))
        return list(st)[:len(slots)]

    def update_dev(self, slots, d_keys, d_status):
        """update over device arrays (slots is a host list): queued behind everything the context holds; d_status is final after
        Engine.sync()"""
        self.table.eng._chk(self.lib.mp_keyset_update_dev(self.h, len(slots), self._slots(slots), d_keys, d_status))

    def clear(self, slots):
        """the named slots are empty afterwards"""
        self.table.eng._chk(self.lib.mp_keyset_clear(self.h, len(slots), self._slots(slots)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mp_keyset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Table:
    """one mp_table: Parameters + aggregate key with their fixed-base tables in HBM"""

    def __init__(self, eng, m, n, params, shared_key, fb_bits=8):
        self.eng, self.lib, self.m, self.n, self.N = eng, eng.lib, m, n, m * n
        self.fb_bits = fb_bits
        self.params, self.shared_key = bytes(params), (bytes(shared_key) if shared_key is not None else None)
        self.pb = eng.point_bytes
        self.cb = 2 * eng.point_bytes       # bytes of one card (ciphertext)
        if len(self.params) != self.pb * (n + 3) or (self.shared_key is not None and len(self.shared_key) != self.pb):
            raise NativeError(MP_ERR_BAD_ARGUMENT, "parameters / shared key have the wrong length")
        h = ctypes.c_void_p()
        if self.shared_key is None:         # parameters only: a table for keyed batches (one aggregate key per proof)
            eng._chk(self.lib.mp_table_create_params(eng.h, m, n, _in(self.params), fb_bits, ctypes.byref(h)))
        else:
            eng._chk(self.lib.mp_table_create_ex(eng.h, m, n, _in(self.params), _in(self.shared_key), fb_bits, ctypes.byref(h)))
        self.h = h
        self.fb_bits = self.lib.mp_table_window_bits(h)      # (fb_bits = 0: the engine chose by free HBM, as mp_table_create does)
        self.proof_bytes = eng.proof_size(m, n)

    @classmethod
    def borrowed(cls, eng, h, m, n, params, shared_key):
        """the table of a pool member (PoolTable.member): the pool table owns it, close() only forgets the handle"""
        self = cls.__new__(cls)
        self.eng, self.lib, self.m, self.n, self.N = eng, eng.lib, m, n, m * n
        self.params, self.shared_key = params, shared_key
        self.pb, self.cb = eng.point_bytes, 2 * eng.point_bytes
        self.h, self._borrowed = ctypes.c_void_p(h), True
        self.fb_bits = self.lib.mp_table_window_bits(self.h)
        self.proof_bytes = eng.proof_size(m, n)
        return self

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.mp_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-buffer API
    def shuffle_and_remask_batch(self, decks, factors, perms, seeds):
        """B proofs; decks: B*N*128 bytes, factors: B*N*32, perms: list of B*N ints, seeds: B*32 -> (decks, proofs, status)"""
        B = len(seeds) // 32
        N = self.N
        self._need("prover seeds", len(seeds), B * 32)
        self._need("decks", len(decks), B * N * self.cb)
        self._need("masking factors", len(factors), B * N * 32)
        self._need("permutations", len(perms), B * N)
        out_d = (ctypes.c_uint8 * (B * N * self.cb))()
        out_p = (ctypes.c_uint8 * (B * self.proof_bytes))()
        st = (ctypes.c_int32 * B)()
        pm = (ctypes.c_uint32 * (B * N))(*perms)
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch(self.h, B, _in(decks), _in(factors), pm, _in(seeds), out_d, out_p, st))
        return bytes(out_d), bytes(out_p), list(st)

    # ---- keyed batches: one aggregate key per proof (keys: B wire points)
    def shuffle_and_remask_batch_keys(self, keys, decks, factors, perms, seeds):
        B = len(seeds) // 32
        N = self.N
        self._need("prover seeds", len(seeds), B * 32)
        self._need("keys", len(keys), B * self.pb)
        self._need("decks", len(decks), B * N * self.cb)
        self._need("masking factors", len(factors), B * N * 32)
        self._need("permutations", len(perms), B * N)
        out_d = (ctypes.c_uint8 * (B * N * self.cb))()
        out_p = (ctypes.c_uint8 * (B * self.proof_bytes))()
        st = (ctypes.c_int32 * B)()
        pm = (ctypes.c_uint32 * (B * N))(*perms)
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch_keys(self.h, B, _in(keys), _in(decks), _in(factors), pm, _in(seeds), out_d, out_p, st))
        return bytes(out_d), bytes(out_p), list(st)

    def verify_shuffle_batch_keys(self, keys, decks, shuffled, proofs):
        N = self.N
        B = len(decks) // (N * self.cb)
        self._need("decks", len(decks), B * N * self.cb)
        self._need("keys", len(keys), B * self.pb)
        self._need("shuffled decks", len(shuffled), len(decks))
        self._need("proofs", len(proofs), B * self.proof_bytes)
        st = (ctypes.c_int32 * B)()
        self.eng._chk(self.lib.mp_verify_shuffle_batch_keys(self.h, B, _in(keys), _in(decks), _in(shuffled), _in(proofs), st))
        return list(st)

    # ---- chain verification: `tables` chains of `links` shuffles; decks: (links + 1) * tables decks (deck j of table t at j * tables + t)
    def verify_shuffle_chain(self, tables, links, decks, proofs, keys=None):
        self._need("decks", len(decks), (links + 1) * tables * self.N * self.cb)
        self._need("proofs", len(proofs), links * tables * self.proof_bytes)
        if keys is not None:
            self._need("keys", len(keys), links * tables * self.pb)
        st = (ctypes.c_int32 * (links * tables))()
        self.eng._chk(self.lib.mp_verify_shuffle_chain(self.h, tables, links, _in(keys) if keys is not None else None, _in(decks),
                                                       _in(proofs), st))
        return list(st)

    def verify_shuffle_chain_ragged(self, links, decks, proofs, keys=None):
        """chains of different lengths: links[t] shuffles for table t, table-major -- table t owns the decks off(t) + t .. off(t) + t +
        links[t] and the proofs, keys and status words off(t) .. off(t) + links[t] - 1, off(t) = sum(links[:t]) -> status words"""
        tables, total = len(links), sum(links)
        self._need("decks", len(decks), (total + tables) * self.N * self.cb)
        self._need("proofs", len(proofs), total * self.proof_bytes)
        if keys is not None:
            self._need("keys", len(keys), total * self.pb)
        st = (ctypes.c_int32 * max(total, 1))()
        lk = (ctypes.c_uint32 * max(tables, 1))(*links)
        self.eng._chk(self.lib.mp_verify_shuffle_chain_ragged(self.h, tables, lk, _in(keys) if keys is not None else None, _in(decks),
                                                              _in(proofs), st))
        return list(st)[:total]

    def verify_shuffle_chain_ragged_dev(self, links, d_keys, d_decks, d_proofs, d_status):
        """verify_shuffle_chain_ragged over device arrays in the same table-major layout (16-byte aligned; d_keys None = the table's own
        key); `links` is a host list.  d_status is final after Engine.sync()"""
        lk = (ctypes.c_uint32 * max(len(links), 1))(*links)
        self.eng._chk(self.lib.mp_verify_shuffle_chain_ragged_dev(self.h, len(links), lk, d_keys, d_decks, d_proofs, d_status))

    def verify_shuffle_chain_dev(self, tables, links, d_keys, d_decks, d_proofs, d_status):
        self.eng._chk(self.lib.mp_verify_shuffle_chain_dev(self.h, tables, links, d_keys, d_decks, d_proofs, d_status))

    # ---- key sets: window tables of many aggregate keys, built once; proofs name their key by index (device arrays of uint32)
    def keyset(self, keys):
        """keys: n wire points back to back (host bytes) -> KeySet (close() it before the table)"""
        return KeySet(self, keys)

    def keyset_empty(self, capacity):
        """a KeySet of `capacity` empty slots, to be filled by KeySet.update / update_dev"""
        return KeySet(self, capacity=capacity)

    def shuffle_and_remask_batch_keyset_dev(self, ks, B, d_key_index, d_decks, d_factors, d_perms, d_seeds, d_out_decks, d_out_proofs, d_status):
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch_keyset_dev(self.h, ks.h, B, d_key_index, d_decks, d_factors, d_perms, d_seeds,
                                                                      d_out_decks, d_out_proofs, d_status))

    def verify_shuffle_batch_keyset_dev(self, ks, B, d_key_index, d_decks, d_shuffled, d_proofs, d_status):
        self.eng._chk(self.lib.mp_verify_shuffle_batch_keyset_dev(self.h, ks.h, B, d_key_index, d_decks, d_shuffled, d_proofs, d_status))

    def shuffle_and_remask_batch_seeded_keyset_dev(self, ks, B, d_key_index, d_decks, d_seeds, d_out_decks, d_out_proofs, d_status,
                                                   d_out_perms=None, d_out_factors=None):
        """shuffle_and_remask_batch_seeded_dev with key d_key_index[b] of the key set for proof b"""
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch_seeded_keyset_dev(self.h, ks.h, B, d_key_index, d_decks, d_seeds, d_out_decks,
                                                                             d_out_proofs, d_status, d_out_perms, d_out_factors))

    def verify_shuffle_chain_ragged_keyset(self, ks, links, key_index, decks, proofs):
        """verify_shuffle_chain_ragged with ONE key-set index per table (key_index[t]) instead of a key per link -> status words; every
        link of a table whose index names no key reads MP_ERR_BAD_ARGUMENT"""
        tables, total = len(links), sum(links)
        if len(key_index) != tables:
            raise ValueError("key_index: expected one index per table")
        self._need("decks", len(decks), (total + tables) * self.N * self.cb)
        self._need("proofs", len(proofs), total * self.proof_bytes)
        st = (ctypes.c_int32 * max(total, 1))()
        lk = (ctypes.c_uint32 * max(tables, 1))(*links)
        ki = (ctypes.c_uint32 * max(tables, 1))(*key_index)
        self.eng._chk(self.lib.mp_verify_shuffle_chain_ragged_keyset(self.h, ks.h, tables, lk, ki, _in(decks), _in(proofs), st))
        return list(st)[:total]

    def verify_shuffle_chain_ragged_keyset_dev(self, ks, links, d_key_index, d_decks, d_proofs, d_status):
        """the same over device arrays (16-byte aligned; d_key_index: one uint32 per table); `links` is a host list"""
        lk = (ctypes.c_uint32 * max(len(links), 1))(*links)
        self.eng._chk(self.lib.mp_verify_shuffle_chain_ragged_keyset_dev(self.h, ks.h, len(links), lk, d_key_index, d_decks, d_proofs, d_status))

    def shuffle_and_remask_batch_keys_dev(self, B, d_keys, d_decks, d_factors, d_perms, d_seeds, d_out_decks, d_out_proofs, d_status):
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch_keys_dev(self.h, B, d_keys, d_decks, d_factors, d_perms, d_seeds,
                                                                    d_out_decks, d_out_proofs, d_status))

    def verify_shuffle_batch_keys_dev(self, B, d_keys, d_decks, d_shuffled, d_proofs, d_status):
        self.eng._chk(self.lib.mp_verify_shuffle_batch_keys_dev(self.h, B, d_keys, d_decks, d_shuffled, d_proofs, d_status))

    def verify_shuffle_batch(self, decks, shuffled, proofs):
        N = self.N
        B = len(decks) // (N * self.cb)
        self._need("decks", len(decks), B * N * self.cb)
        self._need("shuffled decks", len(shuffled), len(decks))
        self._need("proofs", len(proofs), B * self.proof_bytes)
        st = (ctypes.c_int32 * B)()
        self.eng._chk(self.lib.mp_verify_shuffle_batch(self.h, B, _in(decks), _in(shuffled), _in(proofs), st))
        return list(st)

    def _need(self, what, got, want):
        if got != want:
            raise NativeError(MP_ERR_BAD_ARGUMENT, "%s: %d bytes/entries given, %d expected" % (what, got, want))

    def shuffle_and_remask(self, deck, factors, perm, seed):
        self._need("deck", len(deck), self.N * self.cb)
        self._need("masking factors", len(factors), self.N * 32)
        self._need("permutation", len(perm), self.N)
        self._need("prover seed", len(seed), 32)
        out_d = (ctypes.c_uint8 * (self.N * self.cb))()
        out_p = (ctypes.c_uint8 * self.proof_bytes)()
        pm = (ctypes.c_uint32 * self.N)(*perm)
        rc = self.lib.mp_shuffle_and_remask(self.h, _in(deck), _in(factors), pm, _in(seed), out_d, out_p)
        self.eng._chk(rc)
        return bytes(out_d), bytes(out_p)

    def verify_shuffle(self, deck, shuffled, proof):
        self._need("deck", len(deck), self.N * self.cb)
        self._need("shuffled deck", len(shuffled), self.N * self.cb)
        self._need("proof", len(proof), self.proof_bytes)
        rc = self.lib.mp_verify_shuffle(self.h, _in(deck), _in(shuffled), _in(proof), len(proof))
        return self.eng._chk(rc)

    # ---- single proofs with the aggregate key given per call (keyless tables included); coalesced when set_coalesce is on
    def shuffle_and_remask_keyed(self, shared_key, deck, factors, perm, seed):
        self._need("shared key", len(shared_key), self.pb)
        self._need("deck", len(deck), self.N * self.cb)
        self._need("masking factors", len(factors), self.N * 32)
        self._need("permutation", len(perm), self.N)
        self._need("prover seed", len(seed), 32)
        out_d = (ctypes.c_uint8 * (self.N * self.cb))()
        out_p = (ctypes.c_uint8 * self.proof_bytes)()
        pm = (ctypes.c_uint32 * self.N)(*perm)
        rc = self.lib.mp_shuffle_and_remask_keyed(self.h, _in(shared_key), _in(deck), _in(factors), pm, _in(seed), out_d, out_p)
        self.eng._chk(rc)
        return bytes(out_d), bytes(out_p)

    def verify_shuffle_keyed(self, shared_key, deck, shuffled, proof):
        self._need("shared key", len(shared_key), self.pb)
        self._need("deck", len(deck), self.N * self.cb)
        self._need("shuffled deck", len(shuffled), self.N * self.cb)
        self._need("proof", len(proof), self.proof_bytes)
        rc = self.lib.mp_verify_shuffle_keyed(self.h, _in(shared_key), _in(deck), _in(shuffled), _in(proof), len(proof))
        return self.eng._chk(rc)

    def set_coalesce(self, max_batch, max_wait_us=0):
        """gather the concurrent single-proof calls of this table (shuffle_and_remask, verify_shuffle and their _keyed forms) into batched
        calls of up to max_batch requests; a batch waits at most max_wait_us for more once the context is free; max_batch = 0: off"""
        self.eng._chk(self.lib.mp_set_coalesce(self.h, int(max_batch), int(max_wait_us)))

    def coalesce_stats(self):
        """counters since set_coalesce"""
        v = (ctypes.c_uint64 * 8)()
        self.eng._chk(self.lib.mp_coalesce_stats(self.h, v))
        keys = ["served", "batches", "largest", "closed_full", "closed_time", "rerun", "wait_us"]
        return dict(zip(keys, [int(x) for x in v[:7]]))

    def remask_batch(self, cards, factors):
        count = len(cards) // self.cb
        out = (ctypes.c_uint8 * (count * self.cb))()
        self.eng._chk(self.lib.mp_remask_batch(self.h, count, _in(cards), _in(factors), out))
        return bytes(out)

    def msm(self, n_msm, k, scalars, points):
        out = (ctypes.c_uint8 * (n_msm * self.pb))()
        self.eng._chk(self.lib.mp_msm(self.h, n_msm, k, _in(scalars), _in(points), out))
        return bytes(out)

    def commit_batch(self, count, length, values, r):
        out = (ctypes.c_uint8 * (count * self.pb))()
        self.eng._chk(self.lib.mp_commit_batch(self.h, count, length, _in(values), _in(r), out))
        return bytes(out)

    # ---- device-pointer API (ints = HBM addresses, e.g. torch tensor .data_ptr())
    def set_latency_batch(self, B):
        self.eng._chk(self.lib.mp_set_latency_batch(self.h, B))

    def reserve(self, B):
        self.eng._chk(self.lib.mp_reserve(self.h, B))

    def shuffle_and_remask_batch_dev(self, B, d_decks, d_factors, d_perms, d_seeds, d_out_decks, d_out_proofs, d_status):
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch_dev(self.h, B, d_decks, d_factors, d_perms, d_seeds, d_out_decks, d_out_proofs, d_status))

    def verify_shuffle_batch_dev(self, B, d_decks, d_shuffled, d_proofs, d_status):
        self.eng._chk(self.lib.mp_verify_shuffle_batch_dev(self.h, B, d_decks, d_shuffled, d_proofs, d_status))

    def sigma_prove_batch(self, nbases, bases, publics, witness, fs_init, seeds):
        B = len(witness) // 32
        out = (ctypes.c_uint8 * (B * (nbases * self.pb + 32)))()
        st = (ctypes.c_int32 * B)()
        self.eng._chk(self.lib.mp_sigma_prove_batch(self.h, B, nbases, _in(bases), _in(publics), _in(witness), _in(fs_init),
                                                    _in(seeds), out, st))
        return bytes(out), list(st)

    def sigma_verify_batch(self, nbases, bases, publics, proofs, fs_init):
        B = len(proofs) // (nbases * self.pb + 32)
        st = (ctypes.c_int32 * B)()
        self.eng._chk(self.lib.mp_sigma_verify_batch(self.h, B, nbases, _in(bases), _in(publics), _in(proofs), _in(fs_init), st))
        return list(st)

    # ---- opening cards: K keys, C cards, T tokens per card; signer: C * T indices into the keys, lane order c * T + j
    NO_INDEX = 0xFFFFFFFF

    def reveal_batch(self, keys, secret_keys, cards, T, signer, seeds):
        """a player's side: token = sk[signer] * c0 with its Chaum-Pedersen proof, per (card, token) -> (tokens, proofs, status)"""
        K, C = len(keys) // self.pb, len(cards) // self.cb
        B = C * T
        self._need("keys", len(keys), K * self.pb)
        self._need("secret keys", len(secret_keys), K * 32)
        self._need("cards", len(cards), C * self.cb)
        self._need("signer", len(signer), B)
        self._need("prover seeds", len(seeds), B * 32)
        tok = (ctypes.c_uint8 * max(B * self.pb, 1))()
        prf = (ctypes.c_uint8 * max(B * (2 * self.pb + 32), 1))()
        st = (ctypes.c_int32 * max(B, 1))()
        sg = (ctypes.c_uint32 * max(B, 1))(*signer)
        self.eng._chk(self.lib.mp_reveal_batch(self.h, K, _in(keys), _in(secret_keys), C, _in(cards), T, sg, _in(seeds), tok, prf, st))
        return bytes(tok)[:B * self.pb], bytes(prf)[:B * (2 * self.pb + 32)], list(st)[:B]

    def unmask_batch(self, keys, cards, T, signer, tokens, proofs, plain_cards=b""):
        """whoever opens: verify every token, plaintext = c1 - sum of the card's tokens, index of the plaintext in plain_cards
        -> (plaintexts, indices, token_status, card_status)"""
        K, C = len(keys) // self.pb, len(cards) // self.cb
        B = C * T
        n_plain = len(plain_cards) // self.pb
        self._need("keys", len(keys), K * self.pb)
        self._need("cards", len(cards), C * self.cb)
        self._need("signer", len(signer), B)
        self._need("tokens", len(tokens), B * self.pb)
        self._need("proofs", len(proofs), B * (2 * self.pb + 32))
        self._need("card list", len(plain_cards), n_plain * self.pb)
        out = (ctypes.c_uint8 * max(C * self.pb, 1))()
        idx = (ctypes.c_uint32 * max(C, 1))()
        ts = (ctypes.c_int32 * max(B, 1))()
        cs = (ctypes.c_int32 * max(C, 1))()
        sg = (ctypes.c_uint32 * max(B, 1))(*signer)
        self.eng._chk(self.lib.mp_unmask_batch(self.h, K, _in(keys), C, _in(cards), T, sg, _in(tokens), _in(proofs), n_plain,
                                               _in(plain_cards) if n_plain else None, out, idx, ts, cs))
        return bytes(out)[:C * self.pb], list(idx)[:C], list(ts)[:B], list(cs)[:C]

    def unmask_batch_dev(self, K, d_keys, C, d_cards, T, d_signer, d_tokens, d_proofs, n_plain, d_plain_cards, d_out_plain, d_out_index,
                         d_token_status, d_card_status):
        """the same with device pointers (d_cards may be the prover's d_out_decks); outputs are final after Engine.sync()"""
        self.eng._chk(self.lib.mp_unmask_batch_dev(self.h, K, d_keys, C, d_cards, T, d_signer, d_tokens, d_proofs, n_plain, d_plain_cards,
                                                   d_out_plain, d_out_index, d_token_status, d_card_status))

    # ---- the same for cards with different numbers of tokens: counts[c] tokens for card c, everything per token in lane order
    @staticmethod
    def ragged_first(counts):
        """the offsets array of the ragged calls: item c owns the lanes first[c] .. first[c+1] - 1"""
        first = (ctypes.c_uint32 * (len(counts) + 1))()
        for i, n in enumerate(counts):
            first[i + 1] = first[i] + n
        return first

    def reveal_ragged_batch(self, keys, secret_keys, cards, counts, signer, seeds):
        """reveal_batch with counts[c] tokens for card c -> (tokens, proofs, status)"""
        K, C = len(keys) // self.pb, len(cards) // self.cb
        B = sum(counts)
        self._need("keys", len(keys), K * self.pb)
        self._need("secret keys", len(secret_keys), K * 32)
        self._need("cards", len(cards), C * self.cb)
        self._need("counts", len(counts), C)
        self._need("signer", len(signer), B)
        self._need("prover seeds", len(seeds), B * 32)
        tok = (ctypes.c_uint8 * max(B * self.pb, 1))()
        prf = (ctypes.c_uint8 * max(B * (2 * self.pb + 32), 1))()
        st = (ctypes.c_int32 * max(B, 1))()
        sg = (ctypes.c_uint32 * max(B, 1))(*signer)
        self.eng._chk(self.lib.mp_reveal_ragged_batch(self.h, K, _in(keys), _in(secret_keys), C, _in(cards), self.ragged_first(counts), sg,
                                                      _in(seeds), tok, prf, st))
        return bytes(tok)[:B * self.pb], bytes(prf)[:B * (2 * self.pb + 32)], list(st)[:B]

    def unmask_ragged_batch(self, keys, cards, counts, signer, tokens, proofs, plain_cards=b""):
        """unmask_batch with counts[c] tokens for card c -> (plaintexts, indices, token_status, card_status)"""
        K, C = len(keys) // self.pb, len(cards) // self.cb
        B = sum(counts)
        n_plain = len(plain_cards) // self.pb
        self._need("keys", len(keys), K * self.pb)
        self._need("cards", len(cards), C * self.cb)
        self._need("counts", len(counts), C)
        self._need("signer", len(signer), B)
        self._need("tokens", len(tokens), B * self.pb)
        self._need("proofs", len(proofs), B * (2 * self.pb + 32))
        self._need("card list", len(plain_cards), n_plain * self.pb)
        out = (ctypes.c_uint8 * max(C * self.pb, 1))()
        idx = (ctypes.c_uint32 * max(C, 1))()
        ts = (ctypes.c_int32 * max(B, 1))()
        cs = (ctypes.c_int32 * max(C, 1))()
        sg = (ctypes.c_uint32 * max(B, 1))(*signer)
        self.eng._chk(self.lib.mp_unmask_ragged_batch(self.h, K, _in(keys), C, _in(cards), self.ragged_first(counts), sg, _in(tokens),
                                                      _in(proofs), n_plain, _in(plain_cards) if n_plain else None, out, idx, ts, cs))
        return bytes(out)[:C * self.pb], list(idx)[:C], list(ts)[:B], list(cs)[:C]

    def unmask_ragged_batch_dev(self, K, d_keys, counts, d_cards, d_signer, d_tokens, d_proofs, n_plain, d_plain_cards, d_out_plain,
                                d_out_index, d_token_status, d_card_status):
        """the same with device pointers; `counts` stays a host list (the offsets are validated on the host and uploaded by the
        library before the call returns); outputs are final after Engine.sync()"""
        self.eng._chk(self.lib.mp_unmask_ragged_batch_dev(self.h, K, d_keys, len(counts), d_cards, self.ragged_first(counts), d_signer,
                                                          d_tokens, d_proofs, n_plain, d_plain_cards, d_out_plain, d_out_index,
                                                          d_token_status, d_card_status))

    def aggregate_keys_ragged_batch(self, counts, keys, proofs, fs_init):
        """seating tables of different sizes: counts[k] players at table k, lanes in table order
        -> (aggregate keys, player status, table status)"""
        tables, B = len(counts), sum(counts)
        self._need("keys", len(keys), B * self.pb)
        self._need("proofs", len(proofs), B * (self.pb + 32))
        self._need("fs_init", len(fs_init), B * 32)
        out = (ctypes.c_uint8 * max(tables * self.pb, 1))()
        ps = (ctypes.c_int32 * max(B, 1))()
        ts = (ctypes.c_int32 * max(tables, 1))()
        self.eng._chk(self.lib.mp_aggregate_keys_ragged_batch(self.h, tables, self.ragged_first(counts), _in(keys), _in(proofs),
                                                              _in(fs_init), out, ps, ts))
        return bytes(out)[:tables * self.pb], list(ps)[:B], list(ts)[:tables]

    # ---- dealing and seating: K aggregate keys, C cards with a key index each; kind: DEAL_MASK (inputs = plaintext cards, one point
    #      each) or DEAL_REMASK (inputs = masked cards)
    DEAL_MASK, DEAL_REMASK = 0, 1

    def _deal_shape(self, kind, keys, key_index, inputs):
        K, C = len(keys) // self.pb, len(key_index)
        self._need("keys", len(keys), K * self.pb)
        self._need("inputs", len(inputs), C * (self.cb if kind == self.DEAL_REMASK else self.pb))
        return K, C, (ctypes.c_uint32 * max(C, 1))(*key_index)

    def mask_batch(self, kind, keys, key_index, inputs, factors, seeds):
        """whoever deals: masked = in + (r G, r pk[key_index]) with its Chaum-Pedersen proof, per card -> (masked cards, proofs, status)"""
        K, C, ki = self._deal_shape(kind, keys, key_index, inputs)
        psz = 2 * self.pb + 32
        self._need("masking factors", len(factors), C * 32)
        self._need("prover seeds", len(seeds), C * 32)
        out = (ctypes.c_uint8 * max(C * self.cb, 1))()
        prf = (ctypes.c_uint8 * max(C * psz, 1))()
        st = (ctypes.c_int32 * max(C, 1))()
        self.eng._chk(self.lib.mp_mask_batch(self.h, kind, K, _in(keys), C, ki, _in(inputs), _in(factors), _in(seeds), out, prf, st))
        return bytes(out)[:C * self.cb], bytes(prf)[:C * psz], list(st)[:C]

    def verify_mask_batch(self, kind, keys, key_index, inputs, masked, proofs):
        """every player: one status word per card (0, 6 "Chaum-Pedersen" or < 0)"""
        K, C, ki = self._deal_shape(kind, keys, key_index, inputs)
        self._need("masked cards", len(masked), C * self.cb)
        self._need("proofs", len(proofs), C * (2 * self.pb + 32))
        st = (ctypes.c_int32 * max(C, 1))()
        self.eng._chk(self.lib.mp_verify_mask_batch(self.h, kind, K, _in(keys), C, ki, _in(inputs), _in(masked), _in(proofs), st))
        return list(st)[:C]

    def mask_batch_keyset(self, ks, kind, key_index, inputs, factors, seeds):
        """mask_batch with the keys named as slots of a key set (key_index[c]) -> (masked cards, proofs, status)"""
        C = len(key_index)
        isz, psz = (self.cb if kind == self.DEAL_REMASK else self.pb), 2 * self.pb + 32
        self._need("inputs", len(inputs), C * isz)
        self._need("masking factors", len(factors), C * 32)
        self._need("prover seeds", len(seeds), C * 32)
        ki = (ctypes.c_uint32 * max(C, 1))(*key_index)
        out, prf, st = (ctypes.c_uint8 * max(C * self.cb, 1))(), (ctypes.c_uint8 * max(C * psz, 1))(), (ctypes.c_int32 * max(C, 1))()
        self.eng._chk(self.lib.mp_mask_batch_keyset(self.h, ks.h, kind, C, ki, _in(inputs), _in(factors), _in(seeds), out, prf, st))
        return bytes(out)[:C * self.cb], bytes(prf)[:C * psz], list(st)[:C]

    def verify_mask_batch_keyset(self, ks, kind, key_index, inputs, masked, proofs):
        """verify_mask_batch with the keys named as slots of a key set -> one status word per card"""
        C = len(key_index)
        self._need("inputs", len(inputs), C * (self.cb if kind == self.DEAL_REMASK else self.pb))
        self._need("masked cards", len(masked), C * self.cb)
        self._need("proofs", len(proofs), C * (2 * self.pb + 32))
        ki = (ctypes.c_uint32 * max(C, 1))(*key_index)
        st = (ctypes.c_int32 * max(C, 1))()
        self.eng._chk(self.lib.mp_verify_mask_batch_keyset(self.h, ks.h, kind, C, ki, _in(inputs), _in(masked), _in(proofs), st))
        return list(st)[:C]

    def verify_mask_batch_keyset_dev(self, ks, kind, C, d_key_index, d_inputs, d_masked, d_proofs, d_status):
        """the same with device pointers; d_status is final after Engine.sync()"""
        self.eng._chk(self.lib.mp_verify_mask_batch_keyset_dev(self.h, ks.h, kind, C, d_key_index, d_inputs, d_masked, d_proofs, d_status))

    def verify_mask_batch_dev(self, kind, K, d_keys, C, d_key_index, d_inputs, d_masked, d_proofs, d_status):
        """the same with device pointers (d_inputs may be a prover's d_out_decks); d_status is final after Engine.sync()"""
        self.eng._chk(self.lib.mp_verify_mask_batch_dev(self.h, kind, K, d_keys, C, d_key_index, d_inputs, d_masked, d_proofs, d_status))

    def aggregate_keys_batch(self, tables, P, keys, proofs, fs_init):
        """seating: lane = table * P + seat -> (aggregate keys, player status, table status)"""
        B = tables * P
        self._need("keys", len(keys), B * self.pb)
        self._need("proofs", len(proofs), B * (self.pb + 32))
        self._need("fs_init", len(fs_init), B * 32)
        out = (ctypes.c_uint8 * max(tables * self.pb, 1))()
        ps = (ctypes.c_int32 * max(B, 1))()
        ts = (ctypes.c_int32 * max(tables, 1))()
        self.eng._chk(self.lib.mp_aggregate_keys_batch(self.h, tables, P, _in(keys), _in(proofs), _in(fs_init), out, ps, ts))
        return bytes(out)[:tables * self.pb], list(ps)[:B], list(ts)[:tables]

    # ---- secrets from seeds ("mpshuffle secret stream v1", include/mpshuffle.h): one 32-byte seed per lane
    def sample_secrets_batch(self, seeds, S, P):
        """L seeds -> (L * S wire scalars as bytes, list of L * P permutation entries)"""
        L = len(seeds) // 32
        self._need("seeds", len(seeds), L * 32)
        sc = (ctypes.c_uint8 * max(L * S * 32, 1))()
        pm = (ctypes.c_uint32 * max(L * P, 1))()
        self.eng._chk(self.lib.mp_sample_secrets_batch(self.h, L, _in(seeds), S, P, sc if S else None, pm if P else None))
        return bytes(sc)[:L * S * 32], list(pm)[:L * P]

    def sample_secrets_batch_dev(self, L, d_seeds, S, P, d_out_scalars, d_out_perms):
        """the same with device pointers; the outputs are final after Engine.sync()"""
        self.eng._chk(self.lib.mp_sample_secrets_batch_dev(self.h, L, d_seeds, S, P, d_out_scalars, d_out_perms))

    def shuffle_and_remask_batch_seeded(self, decks, seeds, keys=None, witness=False):
        """B proofs whose masking factors and permutations are drawn on the device from seeds[b] (also the prover seed); keys: None = the
        table's key, else B wire points -> (decks, proofs, status), with witness=True also (permutation entries, masking factors)"""
        B, N = len(seeds) // 32, self.N
        self._need("seeds", len(seeds), B * 32)
        self._need("decks", len(decks), B * N * self.cb)
        if keys is not None:
            self._need("keys", len(keys), B * self.pb)
        out_d = (ctypes.c_uint8 * max(B * N * self.cb, 1))()
        out_p = (ctypes.c_uint8 * max(B * self.proof_bytes, 1))()
        st = (ctypes.c_int32 * max(B, 1))()
        pm = (ctypes.c_uint32 * max(B * N, 1))() if witness else None
        rho = (ctypes.c_uint8 * max(B * N * 32, 1))() if witness else None
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch_seeded(self.h, B, _in(keys) if keys is not None else None, _in(decks), _in(seeds),
                                                                  out_d, out_p, st, pm, rho))
        res = bytes(out_d)[:B * N * self.cb], bytes(out_p)[:B * self.proof_bytes], list(st)[:B]
        return res + (list(pm)[:B * N], bytes(rho)[:B * N * 32]) if witness else res

    def shuffle_and_remask_batch_seeded_dev(self, B, d_keys, d_decks, d_seeds, d_out_decks, d_out_proofs, d_status, d_out_perms=None,
                                            d_out_factors=None):
        """the same with device pointers (d_keys / d_out_perms / d_out_factors may be None); final after Engine.sync()"""
        self.eng._chk(self.lib.mp_shuffle_and_remask_batch_seeded_dev(self.h, B, d_keys, d_decks, d_seeds, d_out_decks, d_out_proofs, d_status,
                                                                      d_out_perms, d_out_factors))

    def keygen_batch(self, seeds, fs_init=None):
        """K players: sk = the stream's single scalar, pk = sk G; with fs_init (K * 32 bytes) also the proofs of key ownership under the
        prover seeds `seeds` -> (public keys, secret keys, proofs or None, status)"""
        K = len(seeds) // 32
        self._need("seeds", len(seeds), K * 32)
        if fs_init is not None:
            self._need("fs_init", len(fs_init), K * 32)
        psz = self.pb + 32
        pk = (ctypes.c_uint8 * max(K * self.pb, 1))()
        sk = (ctypes.c_uint8 * max(K * 32, 1))()
        prf = (ctypes.c_uint8 * max(K * psz, 1))() if fs_init is not None else None
        st = (ctypes.c_int32 * max(K, 1))()
        self.eng._chk(self.lib.mp_keygen_batch(self.h, K, _in(seeds), _in(fs_init) if fs_init is not None else None, pk, sk, prf, st))
        return bytes(pk)[:K * self.pb], bytes(sk)[:K * 32], bytes(prf)[:K * psz] if prf is not None else None, list(st)[:K]

    def set_io_chunk(self, proofs):
        """proofs per pipelined chunk of the host-buffer entry points (0 = default 65536)"""
        self.eng._chk(self.lib.mp_set_io_chunk(self.h, proofs))

    def io_schedule(self, B, verify=False):
        """the chunk sizes, in order, that a host-buffer prove (verify=False) or verify call of B proofs takes under the current set_io_chunk"""
        k = self.lib.mp_io_schedule(self.h, B, 1 if verify else 0, None, 0)
        out = (ctypes.c_size_t * max(k, 1))()
        k2 = self.lib.mp_io_schedule(self.h, B, 1 if verify else 0, out, k)
        if k2 != k:
            raise NativeError(MP_ERR_INTERNAL, "mp_io_schedule: the schedule changed between two calls")
        return list(out)[:k]

    def set_merged_verify(self, on=True):
        """verification strategy: merged screening pass first (default) or always equation by equation"""
        self.eng._chk(self.lib.mp_set_merged_verify(self.h, 1 if on else 0))

    def set_bucket_min(self, terms):
        """variable-base MSMs of at least `terms` terms run on the bucket-method kernel (default 2048; 0 = never)"""
        self.eng._chk(self.lib.mp_set_bucket_min(self.h, terms))

    def set_bucket_bits(self, bits):
        """window width of the bucket method: 8 .. 13, or 0 = by the size of the MSM (default: 11 from 40 000 terms on, 12 from 100 000, 13 from 200 000)"""
        self.eng._chk(self.lib.mp_set_bucket_bits(self.h, bits))

    VALIDATED_DECKS, VALIDATED_SHUFFLED, VALIDATED_PROOFS = 1, 2, 4

    def set_validated(self, what):
        """inputs the caller has validated once already (OR of VALIDATED_*): their subgroup test is not repeated in every call"""
        self.eng._chk(self.lib.mp_set_validated(self.h, what))

    def deck_validate_dev(self, decks, d_wire_decks, d_status):
        """wire-v1 decks in device memory -> one int32 per deck (0 / MP_ERR_BAD_ENCODING): range, curve equation, prime-order subgroup"""
        self.eng._chk(self.lib.mp_deck_validate_dev(self.h, decks, d_wire_decks, d_status))

    def set_bucket_split(self, min_bits):
        """windows of at least `min_bits` bits run sort / additions / reduction as three kernels (default 12; 10 .. 15 = never)"""
        self.eng._chk(self.lib.mp_set_bucket_split(self.h, min_bits))

    def set_chain_max_links(self, links):
        """chain verification: at most `links` links per chain equation (0 = as many as fit)"""
        self.eng._chk(self.lib.mp_set_chain_max_links(self.h, links))

    def set_chain_slice(self, tables_per_pass):
        """chain verification in passes of this many tables (0 = one pass if its workspace fits the free memory)"""
        self.eng._chk(self.lib.mp_set_chain_slice(self.h, tables_per_pass))

    def set_chain_pieces(self, mode):
        """how the ragged chain calls cut their chains: CHAIN_PIECES_WHOLE (one piece per table, a pass per distinct length) or
        CHAIN_PIECES_BINARY (pieces of 2^k links, at most 12 passes; a call in which that would save no pass, such as chains of one
        length, keeps its chains whole); same status words"""
        self.eng._chk(self.lib.mp_set_chain_pieces(self.h, mode))

    def chain_ragged_stats(self):
        """the last ragged chain call: [passes, pieces, tables, links, bytes gathered on the device, bytes staged on the host (the constant 0: there is no
        such copy), pieces of the widest pass, the cut that was made]"""
        out = (ctypes.c_uint64 * 8)()
        self.eng._chk(self.lib.mp_chain_ragged_stats(self.h, out))
        return list(out)

    def chain_group_size(self, tables, links, keyed=False):
        """tables per chain equation a pass of `tables` tables x `links` links takes under the current settings"""
        return int(self.lib.mp_chain_group_size(self.h, tables, links, 1 if keyed else 0))

    def chain_last_slice(self):
        """tables per pass of the last chain verification call on this table"""
        return int(self.lib.mp_chain_last_slice(self.h))

    def set_chain_group(self, tables_per_equation):
        """chain verification: tables per chain equation (0 = by size, 1 = every table on its own)"""
        self.eng._chk(self.lib.mp_set_chain_group(self.h, tables_per_equation))

    def set_transcript_lanes(self, lanes):
        """lanes per Fiat-Shamir transcript hash: 1, 4, or 0 = by batch size (4 up to 32 768 proofs)"""
        self.eng._chk(self.lib.mp_set_transcript_lanes(self.h, lanes))

    def set_group_lanes(self, lanes):
        """lanes per group operation of the MSM dependency chains: 1, 4, or 0 = by batch size (4 for a few dozen proofs)"""
        self.eng._chk(self.lib.mp_set_group_lanes(self.h, lanes))

    def set_work_split(self, split):
        """every batch takes work split `split` (0 throughput, 1 latency, 2 medium, 3 finest, 4 wide, 5 small); -1 = by batch size"""
        self.eng._chk(self.lib.mp_set_work_split(self.h, split))

    def group_size(self, B):
        """proofs per group of the screening pass for a batch of B (0: per-proof screen)"""
        return self.lib.mp_group_size(self.h, B)

    def set_group_verify(self, points_per_group=243712, min_batch=6144):
        """screening pass of large batches: one equation of ~points_per_group points per group of proofs on the bucket kernels (a proof
        brings 4N + 11m + 8 points; 0 = off; up to 65 535: at most that many and one wave per window, as in rounds 4-5; the default:
        equations of up to 1 024 52-card proofs on the split pipeline for batches of 32 768 proofs and more)"""
        self.eng._chk(self.lib.mp_set_group_verify(self.h, points_per_group, min_batch))

    def set_group_refine(self, points_per_subgroup=0, min_subgroups=0):
        """what a failing group costs: its members go through equations of sub-groups of ~points_per_subgroup points (0 = an eighth of
        the group equation's) when there are at least min_subgroups of them (0 = 128), else straight to the per-equation pass"""
        self.eng._chk(self.lib.mp_set_group_refine(self.h, points_per_subgroup, min_subgroups))

    def set_group_adapt(self, on=True):
        """groups that shrink under sustained rejection (default on): more than a fifth of a call's groups failing halves the next call's
        group size, fewer than 4 % restore it step by step; False pins the default size"""
        self.eng._chk(self.lib.mp_set_group_adapt(self.h, 1 if on else 0))

    def reverified_count(self):
        """proofs that have taken a per-equation pass on this table because a screen could not clear them"""
        return int(self.lib.mp_reverified_count(self.h))

    def set_pipeline(self, depth=1):
        """depth >= 1: device-resident verify calls run on the context's second lane beside the next prove call and do not wait for
        their screening verdict (include/mpshuffle.h: mp_set_pipeline); their inputs must stay untouched until `depth` further verify
        calls or a sync have returned; 0 = off"""
        self.eng._chk(self.lib.mp_set_pipeline(self.h, int(depth)))

    def set_plan_params(self, split, fixed_terms, var_terms, table_group, norm_chunk, window_lanes=1):
        """sizes of work split `split`: terms per fixed-base / variable-base sub-job, bases per table lane, points per inversion,
        lanes per variable-base sub-job (window split)"""
        self.eng._chk(self.lib.mp_set_plan_params(self.h, split, fixed_terms, var_terms, table_group, norm_chunk, window_lanes))

    def set_plan_thresholds(self, finest, small, latency, medium, wide):
        """largest batch that takes the finest / small / latency / medium / wide split"""
        self.eng._chk(self.lib.mp_set_plan_thresholds(self.h, finest, small, latency, medium, wide))

    def set_toom_cook(self, on=True):
        """3 <= m <= 8: Toom-Cook (default) or Karatsuba evaluation of the multi-exponentiation diagonals"""
        self.eng._chk(self.lib.mp_set_toom_cook(self.h, 1 if on else 0))

    SIGMA_SCREEN_AUTO = 0xFFFFFFFF      # MP_SIGMA_SCREEN_AUTO

    def set_sigma_screen(self, lanes_per_group=SIGMA_SCREEN_AUTO, min_lanes=1024):
        """screening of the sigma verifiers (unmask_batch[_dev], verify_mask_batch[_dev], aggregate_keys_batch, sigma_verify_batch): the
        checks of `lanes_per_group` consecutive lanes as one weighted equation on the bucket kernels, the lanes of a failing group re-verified
        one by one -- same status words, same outputs.  0 = off (the default), SIGMA_SCREEN_AUTO = sized by points; calls with fewer than
        min_lanes lanes keep the per-proof path.  With it on, the *_dev forms wait once for a 4-byte flag.  Resets sigma_screen_stats."""
        self.eng._chk(self.lib.mp_set_sigma_screen(self.h, lanes_per_group, min_lanes))

    def sigma_screen_stats(self):
        """since the last set_sigma_screen: [lanes screened, group equations evaluated, groups that failed, lanes re-verified per proof]"""
        v = (ctypes.c_uint64 * 4)()
        self.eng._chk(self.lib.mp_sigma_screen_stats(self.h, v))
        return [int(x) for x in v]

    def set_subgroup_check(self, on=True):
        """curves with a cofactor: test every wire point for membership in the prime-order subgroup (default on)"""
        self.eng._chk(self.lib.mp_set_subgroup_check(self.h, 1 if on else 0))

    def plan_stats(self):
        v = (ctypes.c_uint64 * 16)()
        self.eng._chk(self.lib.mp_plan_stats(self.h, v))
        keys = ["fixed_terms", "var_terms", "fixed_jobs", "var_jobs", "table_bases", "combine_terms"]
        out = {"prove": dict(zip(keys, v[0:6])), "verify": dict(zip(keys, v[6:12]))}
        out.update(var_windows=v[12], fixed_windows=v[13], N=v[14] & 0xFFFFFFFF, toom_points_m=v[14] >> 32)
        # MSMs on the bucket-method kernel (prove + verify together): terms and jobs; 8-bit windows
        out.update(bucket_terms=v[15] & 0xFFFFFFFF, bucket_jobs=v[15] >> 32)
        return out

    def work_census(self):
        v = [ctypes.c_uint64() for _ in range(4)]
        self.eng._chk(self.lib.mp_work_census(self.h, *[ctypes.byref(x) for x in v]))
        return dict(prove_terms=v[0].value, verify_terms=v[1].value, prove_point_ops=v[2].value, verify_point_ops=v[3].value)


class Pool:
    """one mp_pool: contexts behind one handle (include/mpshuffle.h, "device pool").  devices[i] is the device of member i; a device named
    several times gives lanes that run side by side on it; an int k means devices 0 .. k-1"""

    def __init__(self, curve="stark", devices=(0,), lib=None):
        self.lib = lib if lib is not None else load()
        self.curve = curve
        self.devices = list(range(devices)) if isinstance(devices, int) else [int(d) for d in devices]
        n = len(self.devices)
        h = ctypes.c_void_p()
        rc = self.lib.mp_pool_create(CURVE_IDS[curve], n, (ctypes.c_int * max(n, 1))(*self.devices), ctypes.byref(h))
        if rc != 0:
            text = self.lib.mp_last_error().decode()
            raise (NoDeviceError if rc == MP_ERR_NO_DEVICE else NativeError)(rc, text)
        self.h = h
        self.point_bytes = self.lib.mp_point_size(CURVE_IDS[curve])
        self._tables = weakref.WeakSet()      # the pool's tables must go before it: close() closes those still open

    def __len__(self):
        return self.lib.mp_pool_size(self.h)

    def engine(self, i=0):
        """member i's context as a non-owning Engine"""
        h = self.lib.mp_pool_member_ctx(self.h, i)
        if not h:
            raise NativeError(MP_ERR_BAD_ARGUMENT, "pool has no member %d" % i)
        return Engine.borrowed(self.curve, h, self.lib)

    def table(self, m, n, params, shared_key=None, fb_bits=8):
        """shared_key None: a keyless pool table (one aggregate key per proof)"""
        return PoolTable(self, m, n, params, shared_key, fb_bits)

    def close(self):
        if getattr(self, "h", None):
            for t in list(self._tables):
                t.close()
            self.lib.mp_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoolTable:
    """one mp_pool_table: a Table per pool member; the members of one device share its fixed-base tables.  The batch calls cut their
    proofs into contiguous blocks over the members and return the bytes and status words of the same call on one Table"""

    def __init__(self, pool, m, n, params, shared_key=None, fb_bits=8):
        self.pool, self.lib, self.m, self.n, self.N = pool, pool.lib, m, n, m * n
        self.params, self.shared_key = bytes(params), (bytes(shared_key) if shared_key is not None else None)
        self.pb, self.cb = pool.point_bytes, 2 * pool.point_bytes
        if len(self.params) != self.pb * (n + 3) or (self.shared_key is not None and len(self.shared_key) != self.pb):
            raise NativeError(MP_ERR_BAD_ARGUMENT, "parameters / shared key have the wrong length")
        h = ctypes.c_void_p()
        self._chk(self.lib.mp_pool_table_create(pool.h, m, n, _in(self.params), _in(self.shared_key) if self.shared_key is not None else None,
                                                fb_bits, ctypes.byref(h)))
        self.h = h
        pool._tables.add(self)
        self.proof_bytes = self.lib.mp_proof_size_curve(CURVE_IDS[pool.curve], m, n)

    def _chk(self, rc):
        if rc < 0:
            raise NativeError(rc, self.lib.mp_last_error().decode())
        return rc

    _need = Table._need

    def close(self):
        if getattr(self, "h", None):
            self.lib.mp_pool_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def member(self, i):
        """member i's table as a non-owning Table: settings, direct calls, device-resident callers that shard themselves"""
        h = self.lib.mp_pool_table_member(self.h, i)
        if not h:
            raise NativeError(MP_ERR_BAD_ARGUMENT, "pool table has no member %d" % i)
        return Table.borrowed(self.pool.engine(i), h, self.m, self.n, self.params, self.shared_key)

    def set_min_shard(self, proofs):
        """proofs a block must hold before a call takes another member (default 1)"""
        self._chk(self.lib.mp_pool_set_min_shard(self.h, int(proofs)))

    def stats(self):
        """[pool calls, proofs, members used by the last call, fixed-base table builds (= distinct devices), members, 0, 0, 0]"""
        v = (ctypes.c_uint64 * 8)()
        self._chk(self.lib.mp_pool_stats(self.h, v))
        return [int(x) for x in v]

    def member_stats(self, i):
        v = (ctypes.c_uint64 * 4)()
        self._chk(self.lib.mp_pool_member_stats(self.h, i, v))
        return dict(zip(["device", "calls", "proofs", "busy_us"], [int(x) for x in v]))

    def shuffle_and_remask_batch(self, decks, factors, perms, seeds, keys=None):
        """B proofs as Table.shuffle_and_remask_batch (keys: B wire points, one aggregate key per proof) -> (decks, proofs, status)"""
        B = len(seeds) // 32
        N = self.N
        self._need("prover seeds", len(seeds), B * 32)
        if keys is not None:
            self._need("keys", len(keys), B * self.pb)
        self._need("decks", len(decks), B * N * self.cb)
        self._need("masking factors", len(factors), B * N * 32)
        self._need("permutations", len(perms), B * N)
        out_d = (ctypes.c_uint8 * max(B * N * self.cb, 1))()
        out_p = (ctypes.c_uint8 * max(B * self.proof_bytes, 1))()
        st = (ctypes.c_int32 * max(B, 1))()
        pm = (ctypes.c_uint32 * max(B * N, 1))(*perms)
        self._chk(self.lib.mp_pool_shuffle_and_remask_batch(self.h, B, _in(keys) if keys is not None else None, _in(decks), _in(factors), pm,
                                                            _in(seeds), out_d, out_p, st))
        return bytes(out_d)[:B * N * self.cb], bytes(out_p)[:B * self.proof_bytes], list(st)[:B]

    def verify_shuffle_batch(self, decks, shuffled, proofs, keys=None):
        N = self.N
        B = len(decks) // (N * self.cb)
        self._need("decks", len(decks), B * N * self.cb)
        if keys is not None:
            self._need("keys", len(keys), B * self.pb)
        self._need("shuffled decks", len(shuffled), len(decks))
        self._need("proofs", len(proofs), B * self.proof_bytes)
        st = (ctypes.c_int32 * max(B, 1))()
        self._chk(self.lib.mp_pool_verify_shuffle_batch(self.h, B, _in(keys) if keys is not None else None, _in(decks), _in(shuffled),
                                                        _in(proofs), st))
        return list(st)[:B]
