"""CPU tests (-m "not gpu") of the ragged calls -- mp_reveal_ragged_batch, mp_unmask_ragged_batch[_dev], mp_aggregate_keys_ragged_batch,
mp_verify_shuffle_chain_ragged -- with the kernel bodies under the development emulator (tools/hostemu): the cases of
tests/ragged_cases.py in full on the STARK curve, the shapes that cross a wave or a workgroup on BLS12-377 as well (the 14-limb field, and
the only curve with a subgroup test)."""
import ctypes
import os
import subprocess

import pytest

import ragged_cases as rc
from conftest import ROOT


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


def _run(fn, *args):
    fails, checks = fn(*args)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


_ids = [c[0] for c in rc.CASES]
_BLS = [c for c in rc.CASES if c[0] in ("an item straddles lanes 63 | 64", "counts 2..10 mixed, the last item of one lane")]


def test_every_case_hits_the_edge_it_names():
    assert rc.workgroup_size() == rc.WORKGROUP
    assert not rc.edge_failures()


@pytest.mark.parametrize("case", rc.CASES, ids=_ids)
def test_opening_matches_the_oracle_and_the_regrouped_uniform_calls_stark(emu, coracle, case):
    _run(rc.run_open_case, emu("stark"), coracle, "stark", case)


@pytest.mark.parametrize("case", _BLS, ids=[c[0] for c in _BLS])
def test_opening_matches_the_oracle_and_the_regrouped_uniform_calls_bls12_377(emu, coracle, case):
    _run(rc.run_open_case, emu("bls12_377"), coracle, "bls12_377", case)


@pytest.mark.parametrize("case", rc.CASES, ids=_ids)
def test_seating_matches_the_oracle_and_the_regrouped_uniform_calls_stark(emu, coracle, case):
    _run(rc.run_seating_case, emu("stark"), coracle, "stark", case)


@pytest.mark.parametrize("case", _BLS, ids=[c[0] for c in _BLS])
def test_seating_matches_the_oracle_and_the_regrouped_uniform_calls_bls12_377(emu, coracle, case):
    _run(rc.run_seating_case, emu("bls12_377"), coracle, "bls12_377", case)


@pytest.mark.parametrize("shape", rc.EQUAL, ids=lambda s: "%dx%d" % s)
def test_equal_counts_give_the_bytes_of_the_uniform_calls(emu, coracle, shape):
    _run(rc.run_open_equal, emu("stark"), coracle, "stark", shape)
    _run(rc.run_seating_equal, emu("stark"), coracle, "stark", shape)


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
def test_defects_stay_with_their_lanes_and_items(emu, coracle, curve):
    _run(rc.run_open_defects, emu(curve), coracle, curve)
    _run(rc.run_seating_defects, emu(curve), coracle, curve)


def test_screened_calls_give_the_same_words_and_bytes(emu, coracle):
    _run(rc.run_screen, emu("stark"), coracle, "stark")


def test_argument_errors_leave_the_outputs_alone(emu, coracle):
    _run(rc.run_argument_errors, emu("stark"), coracle, "stark")


def test_device_pointer_form_gives_the_same_outputs(emu, coracle):
    import torch
    _run(rc.run_open_dev, emu("stark"), coracle, "stark", torch, "cpu")


def test_tiny_batch_matches_the_python_oracle(emu, coracle):
    _run(rc.run_open_python_oracle, emu("stark"), coracle, "stark")


@pytest.mark.parametrize("keyed", [False, True], ids=["own key", "keys per link"])
def test_chains_of_different_lengths(emu, coracle, keyed):
    _run(rc.run_chains, emu("stark"), coracle, keyed)


def test_cpp_mirror_ragged_members(emu, tmp_path):
    """the ragged overloads of include/barnett_smart.hpp, compiled with g++ and run against the emulator library"""
    d = os.path.join(ROOT, "tools", "hostemu")
    exe = tmp_path / "mirror_ragged"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mirror_ragged.cpp"),
                           "-L", d, "-lmpemu", "-Wl,-rpath," + d, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mirror_ragged ok" in out.stdout, out.stdout + out.stderr
