"""CPU tests (-m "not gpu") of chains of different lengths verified in passes of equal pieces -- mp_verify_shuffle_chain_ragged[_dev],
mp_set_chain_pieces, mp_chain_ragged_stats -- with the kernel bodies under the development emulator (tools/hostemu): the cases of
tests/chain_piece_cases.py except the 52-card rows, which only the GPU test runs.  The emulator's copies are synchronous: what the _dev
cases can show here is the addressing, not the ordering of the gather, the passes, the scatter and mp_sync."""
import ctypes
import os
import subprocess

import pytest

import chain_piece_cases as cp
from conftest import ROOT


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


def _run(fn, *args, **kw):
    fails, checks = fn(*args, **kw)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0


@pytest.mark.parametrize("keyed", [False, True], ids=["own key", "keys per link"])
def test_honest_chains_in_both_modes_from_host_and_device_buffers(emu, coracle, keyed):
    """the first case: fails without mp_verify_shuffle_chain_ragged_dev, mp_set_chain_pieces and mp_chain_ragged_stats"""
    import torch
    _run(cp.run_honest, emu("stark"), coracle, keyed, torch, "cpu")


def test_the_cases_reach_their_edges_and_the_model_restates_the_source():
    assert not cp.edge_failures()


@pytest.mark.parametrize("name", cp.DEFECTS)
def test_defects_at_piece_boundaries_fail_their_links_alone(emu, coracle, name):
    import torch
    _run(cp.run_defect, emu("stark"), coracle, name, True, torch, "cpu", settings=name == cp.DEFECTS[0])


def test_defects_on_a_table_with_its_own_key(emu, coracle):
    _run(cp.run_defect, emu("stark"), coracle, cp.DEFECTS[1], False)


@pytest.mark.parametrize("keyed", [False, True], ids=["own key", "keys per link"])
def test_equal_lengths_give_the_words_of_the_uniform_call(emu, coracle, keyed):
    _run(cp.run_equal, emu("stark"), coracle, keyed)


def test_rows_of_96_byte_points(emu, coracle):
    _run(cp.run_width, emu("bls12_377"), coracle, "bls12_377", cp.MN, cp.BLS_LINKS)


def test_refused_calls_touch_nothing(emu, coracle):
    import torch
    _run(cp.run_refusals, emu("stark"), coracle, torch, "cpu")


def test_cpp_mirror_device_form_and_setter(emu, tmp_path):
    """verify_shuffle_chains_dev and set_chain_pieces of include/barnett_smart.hpp, compiled with g++ and run against the emulator
    library (its device pointers are host pointers)"""
    d = os.path.join(ROOT, "tools", "hostemu")
    exe = tmp_path / "mirror_chain_pieces"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mirror_chain_pieces.cpp"),
                           "-L", d, "-lmpemu", "-Wl,-rpath," + d, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mirror_chain_pieces ok" in out.stdout, out.stdout + out.stderr
