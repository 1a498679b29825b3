"""CPU tests (-m "not gpu") of dealing and seating -- mp_mask_batch, mp_verify_mask_batch, mp_verify_mask_batch_dev,
mp_aggregate_keys_batch -- with the kernel bodies under the development emulator (tools/hostemu): the cases of tests/deal_cases.py in
full on the STARK curve, the honest shapes on BLS12-377 (the 14-limb field, and the only curve with a subgroup test)."""
import ctypes
import os
import subprocess
import threading

import pytest

import deal_cases as dc
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


@pytest.mark.parametrize("shape", dc.shapes("stark"), ids=lambda s: "%dx%d" % s)
def test_mask_and_verify_match_the_oracle_stark(emu, coracle, shape):
    _run(dc.run_honest, emu("stark"), coracle, "stark", [shape])


@pytest.mark.parametrize("shape", dc.shapes("bls12_377"), ids=lambda s: "%dx%d" % s)
def test_mask_and_verify_match_the_oracle_bls12_377(emu, coracle, shape):
    _run(dc.run_honest, emu("bls12_377"), coracle, "bls12_377", [shape])


@pytest.mark.parametrize("seats", dc.SEATS, ids=lambda s: "%dx%d" % s)
def test_aggregate_keys_match_the_oracle_stark(emu, coracle, seats):
    _run(dc.run_seating, emu("stark"), coracle, "stark", [seats])


@pytest.mark.parametrize("seats", dc.SEATS, ids=lambda s: "%dx%d" % s)
def test_aggregate_keys_match_the_oracle_bls12_377(emu, coracle, seats):
    _run(dc.run_seating, emu("bls12_377"), coracle, "bls12_377", [seats])


def test_tiny_batch_matches_the_python_oracle(emu, coracle):
    _run(dc.run_python_oracle, emu("stark"), coracle, "stark")


def test_one_defect_per_lane_and_call_level_refusals(emu, coracle):
    _run(dc.run_defects, emu("stark"), coracle, "stark")


def test_points_outside_the_subgroup_bls12_377(emu, coracle):
    _run(dc.run_subgroup, emu("bls12_377"), coracle)


def test_agreement_with_the_composed_calls(emu, coracle):
    _run(dc.run_agreement, emu("stark"), coracle, "stark")


def test_device_pointer_form_gives_the_same_words(emu, coracle):
    import torch
    _run(dc.run_dev, emu("stark"), coracle, "stark", torch, "cpu")


def test_two_host_threads_verify_on_one_table(emu, coracle):
    _run(dc.run_threads, emu("stark"), coracle, "stark", threading)
