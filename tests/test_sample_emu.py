"""CPU tests (-m "not gpu") of the secrets drawn from seeds -- mp_sample_secrets_batch[_dev], mp_shuffle_and_remask_batch_seeded[_dev],
mp_keygen_batch -- with the kernel bodies under the development emulator (tools/hostemu): the cases of tests/sample_cases.py.  The
stream is checked in full on all four curves; the provers behind it are the emulator's CPU loops, so the seeded prover runs its small
shapes here ((2, 3) with 1 and 65 proofs, (2, 4) on bn254 with 65) and the rest -- 257 proofs, the 52-card deck -- on the GPU
(tests/test_gpu_sample.py), and key generation runs every K on the STARK curve and K = 65 on the others."""
import ctypes
import os
import re
import subprocess
import threading

import pytest

import sample_cases as sc
from conftest import ROOT

NEW_SYMBOLS = ["mp_sample_secrets_batch", "mp_sample_secrets_batch_dev", "mp_shuffle_and_remask_batch_seeded",
               "mp_shuffle_and_remask_batch_seeded_dev", "mp_keygen_batch"]


@pytest.fixture(scope="module")
def emulib(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    return mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))


@pytest.fixture(scope="module")
def emu(mp, emulib):
    return lambda curve: mp._native.Engine(curve, 0, lib=emulib)


def _run(fn, *args, **kw):
    fails, checks = fn(*args, **kw)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


def test_c_abi_symbols_are_exported_bound_and_declared(mp, emulib):
    header = open(os.path.join(ROOT, "include", "mpshuffle.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(emulib, name).argtypes, name                                  # bound with a prototype
        assert name in mp._native.SYMBOLS, name
        assert re.search(r"^int %s\(mp_table\* t, " % name, header, re.M), name      # declared
        assert getattr(mp._native.load(), name) is not None, name                    # exported by the gfx950 build as well
    assert b"mpshuffle secret stream v1" == sc.TAG and sc.TAG.decode() in header
    assert mp.protocol.SECRET_STREAM_TAG == sc.TAG


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("curve", sc.CURVES)
def test_stream_word_for_word(emu, coracle, mp, curve, shape):
    _run(sc.run_stream, emu(curve), coracle, curve, shape, mp)


def test_long_streams_stark(emu, coracle):
    _run(sc.run_long, emu("stark"), coracle)


@pytest.mark.parametrize("keyed", [False, True], ids=["table key", "key per proof"])
@pytest.mark.parametrize("curve,mn,B", [("stark", (2, 3), 1), ("stark", (2, 3), 65), ("bn254", (2, 4), 65)])
def test_seeded_prove_equals_unseeded_prove(emu, coracle, curve, mn, B, keyed):
    _run(sc.run_seeded, emu(curve), coracle, curve, mn, B, keyed, python_oracle=B == 1)


@pytest.mark.parametrize("keyed", [False, True], ids=["table key", "key per proof"])
def test_device_pointer_form_equals_host_form(emu, coracle, keyed):
    import torch
    _run(sc.run_seeded_dev, emu("stark"), coracle, "stark", (2, 3), 65, keyed, torch, "cpu")


@pytest.mark.parametrize("curve,K", [("stark", K) for K in sc.KEYGEN] + [(c, 65) for c in sc.CURVES if c != "stark"])
def test_keygen_matches_the_oracle_and_seats(emu, coracle, curve, K):
    _run(sc.run_keygen, emu(curve), coracle, curve, K)


def test_refusals(emu, coracle):
    _run(sc.run_refusals, emu("stark"), coracle, "stark")


def test_two_host_threads_sample_on_one_table(emu, coracle):
    _run(sc.run_threads, emu("stark"), coracle, "stark", threading)
