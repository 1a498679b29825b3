"""CPU tests (-m "not gpu") of the chunked host-buffer calls (tests/host_pipeline_cases.py) with the kernel bodies under the
development emulator (tools/hostemu): mp_io_schedule against the model of the three schedules on the whole sweep; the tiny-size prover
and verifier cases (C <= 9, shape (2, 3)) on STARK -- even cut, ramp, keyed, seeded, bad witnesses and defects at every chunk edge under
the three verification strategies, the pipeline setting and the shared staging buffers -- and one prover / verifier pair on BLS12-377,
whose 96-byte points change every offset; each with pageable buffers and with buffers from mp_host_alloc.

The emulator's copies are synchronous (tools/hostemu/rt.hpp: h2d / d2h are a memcpy, stream_wait does nothing), so what these tests
check are the OFFSETS and the SCHEDULES; an ordering mistake -- a missing wait between the streams -- can only show on the GPU, where
tests/test_gpu_host_pipeline.py runs the same cases and the large ones."""
import ctypes
import os
import subprocess

import pytest

import host_pipeline_cases as hp
from conftest import ROOT


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


def _run(emu, curve, want, fn, *args, **kw):
    eng = emu(curve)
    try:
        fails, checks = fn(eng, *args, **kw)
    finally:
        eng.close()
    assert not fails, "\n".join(fails[:40])
    assert checks == want


STARK = ("stark", 2, 3)
TINY = [(4, 11), (8, 16), (8, 20), (8, 27), (9, 19)]       # even cut; the ramp; C / 8 and 3C / 8 rounding down
_cb = lambda v: "C%d-B%d" % v


def test_schedule_model_is_the_librarys(emu, coracle):
    _run(emu, "stark", hp.schedule_count(), hp.run_schedule, coracle)


@pytest.mark.parametrize("cb", TINY, ids=_cb)
def test_prover_returns_every_row_under_every_schedule(emu, coracle, cb):
    import torch
    _run(emu, "stark", hp.prover_count(*cb), hp.run_prover, coracle, torch, "cpu", *STARK, *cb)


def test_prover_and_verifier_on_96_byte_points(emu, coracle):
    import torch
    _run(emu, "bls12_377", hp.prover_count(8, 20), hp.run_prover, coracle, torch, "cpu", "bls12_377", 2, 3, 8, 20)


def test_keyed_batches_across_chunks(emu, coracle):
    import torch
    _run(emu, "stark", hp.prover_count(8, 27, keyed=True), hp.run_prover, coracle, torch, "cpu", *STARK, 8, 27, keyed=True)


def test_seeded_witnesses_across_chunks(emu, coracle):
    import torch
    _run(emu, "stark", hp.prover_count(8, 27, seeded=True), hp.run_prover, coracle, torch, "cpu", *STARK, 8, 27, seeded=True)


def test_bad_witnesses_at_every_chunk_edge(emu, coracle):
    import torch
    _run(emu, "stark", hp.bad_witness_count(8, 27), hp.run_bad_witness, coracle, torch, "cpu", *STARK, 8, 27)


@pytest.mark.parametrize("cb", TINY, ids=_cb)
def test_verifier_defects_at_every_chunk_edge(emu, coracle, cb):
    import torch
    modes = hp.MODES if cb == (8, 20) else hp.MODES[:2]       # (20, 8): 1 8 6 5 -- the chunk of 1 takes no group, the others do
    _run(emu, "stark", hp.verifier_count(*cb, modes=modes), hp.run_verifier, coracle, torch, "cpu", *STARK, *cb, modes=modes)


def test_pipeline_setting_leaves_the_host_calls_alone(emu, coracle):
    import torch
    _run(emu, "stark", hp.pipeline_count(20), hp.run_pipeline_setting, coracle, torch, "cpu", *STARK, 8, 20)


def test_staging_buffers_shared_with_chain_slices(emu, coracle):
    import torch
    _run(emu, "stark", hp.staging_count(), hp.run_shared_staging, coracle, torch, "cpu", *STARK)
