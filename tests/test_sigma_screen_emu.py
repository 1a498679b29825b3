"""CPU tests (-m "not gpu") of the screening pass of the sigma verifiers (mp_set_sigma_screen) with the kernel bodies under the
development emulator (tools/hostemu): the case functions of open_cases.py and deal_cases.py, unmodified, on tables that screen in groups
of 64 lanes -- on the STARK curve, the honest shapes and the subgroup cases on BLS12-377 as well --, and the cases of
sigma_screen_cases.py: screened against unscreened, localisation, cancelling forgeries, the cofactor rule, usage."""
import ctypes
import os
import subprocess

import pytest

import deal_cases as dc
import open_cases as oc
import sigma_screen_cases as sc
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


def _screened(emu, curve, honest, fn, coracle, *args):
    eng = sc.Screened(emu(curve))
    _run(fn, eng, coracle, curve, *args)
    fails = sc.honest_log_failures(eng.log) if honest else sc.screened_log_failures(eng.log)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_opening_honest_shapes_under_screening(emu, coracle, curve, shape):
    _screened(emu, curve, True, oc.run_honest, coracle, [shape])


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_dealing_honest_shapes_under_screening(emu, coracle, curve, shape):
    _screened(emu, curve, True, dc.run_honest, coracle, [shape])


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
@pytest.mark.parametrize("seats", [s for s in dc.SEATS if s != (7, 9)], ids=lambda s: "%dx%d" % s)
def test_seating_honest_shapes_under_screening(emu, coracle, curve, seats):
    _screened(emu, curve, True, dc.run_seating, coracle, [seats])


def test_seating_with_defects_under_screening(emu, coracle):
    _screened(emu, "stark", False, dc.run_seating, coracle, [(7, 9)])


def test_opening_defects_under_screening(emu, coracle):
    _screened(emu, "stark", False, oc.run_defects, coracle)


def test_opening_agreement_under_screening(emu, coracle):
    _screened(emu, "stark", False, oc.run_agreement, coracle)


def test_opening_device_pointer_form_under_screening(emu, coracle):
    import torch
    _screened(emu, "stark", False, oc.run_dev, coracle, torch, "cpu")


def test_dealing_defects_under_screening(emu, coracle):
    _screened(emu, "stark", False, dc.run_defects, coracle)


def test_dealing_device_pointer_form_under_screening(emu, coracle):
    import torch
    _screened(emu, "stark", False, dc.run_dev, coracle, torch, "cpu")


def test_opening_points_outside_the_subgroup_under_screening(emu, coracle):
    _screened(emu, "bls12_377", False, oc.run_subgroup, coracle)


def test_dealing_points_outside_the_subgroup_under_screening(emu, coracle):
    _screened(emu, "bls12_377", False, dc.run_subgroup, coracle)


def test_screened_equals_unscreened(emu, coracle):
    _run(sc.run_equal, emu("stark"), coracle, "stark")


def test_a_defect_fails_its_group_alone(emu, coracle):
    _run(sc.run_localisation, emu("stark"), coracle, "stark")


def test_cancelling_forgeries_are_refused(emu, coracle):
    _run(sc.run_cancelling, emu("stark"), coracle, "stark")


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
def test_cofactor_rule(emu, coracle, curve):
    _run(sc.run_cofactor, emu(curve), coracle, curve)


def test_usage(emu, coracle):
    _run(sc.run_usage, emu("stark"), coracle, "stark")
