"""CPU tests (-m "not gpu") of key sets whose slots change -- mp_keyset_create_empty, mp_keyset_update[_dev], mp_keyset_clear,
mp_keyset_live, the two _keyset_dev shuffle calls over live and empty slots, the seeded prover, the ragged chain verifier and the dealing calls by index, seating into a set -- with the kernel bodies under the development emulator
(tools/hostemu): the cases of tests/keyset_cases.py except the ordering case, which needs a GPU's streams (the emulator's copies and
launches are synchronous), and the build slice at its real size.  The slice case runs against a second emulator library whose slice is
lowered to 4 keys (make -C tools/hostemu KS_SLICE=4)."""
import ctypes
import os
import re
import subprocess

import pytest

import keyset_cases as kc
from conftest import ROOT

HOSTEMU = os.path.join(ROOT, "tools", "hostemu")
LOWERED_SLICE = 4


@pytest.fixture(scope="module")
def emu(mp):
    mp.build()
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTEMU])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(HOSTEMU, "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


@pytest.fixture(scope="module")
def emu_slice(mp):
    mp.build()
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTEMU, "KS_SLICE=%d" % LOWERED_SLICE])
    lib = mp._native.bind(ctypes.CDLL(os.path.join(HOSTEMU, "libmpemu_ksslice%d.so" % LOWERED_SLICE)))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


def _run(want, fn, *args):
    import torch
    fails, checks = fn(*args, torch, "cpu")
    assert not fails, "\n".join(fails[:40])
    assert checks == want


def _form(k):
    return ("host", "dev")[k % 2]


def test_the_new_symbols_are_declared_exported_and_bound(mp, emu):
    """the header's key-set symbols, in the shared object's binding list and in the emulator library"""
    new = ["mp_keyset_clear", "mp_keyset_create_empty", "mp_keyset_live", "mp_keyset_update", "mp_keyset_update_dev",
           "mp_shuffle_and_remask_batch_seeded_keyset_dev", "mp_verify_shuffle_chain_ragged_keyset",
           "mp_verify_shuffle_chain_ragged_keyset_dev", "mp_mask_batch_keyset", "mp_verify_mask_batch_keyset",
           "mp_verify_mask_batch_keyset_dev", "mp_keyset_seat_ragged_batch"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpshuffle.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", txt))
    lib = mp.load()
    eng = emu("stark")
    for s in new:
        assert s in declared, s
        assert s in mp._native.SYMBOLS, s
        assert hasattr(lib, s), s
        assert hasattr(eng.lib, s), s
    members = ((mp._native.KeySet, ("update", "update_dev", "clear", "live", "seat")),
               (mp._native.Table, ("keyset", "keyset_empty", "shuffle_and_remask_batch_seeded_keyset_dev", "verify_shuffle_chain_ragged_keyset",
                                   "verify_shuffle_chain_ragged_keyset_dev", "mask_batch_keyset", "verify_mask_batch_keyset", "verify_mask_batch_keyset_dev")),
               (mp.DLCards, ("key_set",)))
    for cls, names in members:
        for n in names:
            assert callable(getattr(cls, n)), n


@pytest.mark.parametrize("curve", kc.CURVES)
def test_every_index_of_an_empty_set_is_refused_and_live_neighbours_serve(emu, coracle, curve):
    _run(kc.empty_count(), kc.run_empty, emu(curve), coracle, curve)


@pytest.mark.parametrize("count", kc.UPDATE_COUNTS)
def test_filled_slots_serve_the_oracles_bytes_under_their_keys(emu, coracle, count):
    _run(kc.fill_count(count), kc.run_fill, count, _form(count), emu("stark"), coracle, "stark")


@pytest.mark.parametrize("curve", kc.CURVES[1:])
def test_filled_slots_on_the_other_curves(emu, coracle, curve):
    _run(kc.fill_count(2), kc.run_fill, 2, "dev", emu(curve), coracle, curve)


@pytest.mark.parametrize("created", [True, False], ids=["mp_keyset_create", "mp_keyset_create_empty"])
@pytest.mark.parametrize("curve", kc.CURVES)
def test_a_replaced_slot_serves_the_new_key_and_its_neighbours_their_own(emu, coracle, curve, created):
    """fails on the parent for want of any way to make slot s mean another key; a build that keeps the old table or the old wire key
    proves under the old key"""
    _run(kc.replace_count(created), kc.run_replace, created, _form(created), emu(curve), coracle, curve)


@pytest.mark.parametrize("at", kc.REFUSED_AT)
@pytest.mark.parametrize("name", kc.defects("stark"))
def test_a_refused_key_empties_its_slot_and_no_other(emu, coracle, name, at):
    _run(kc.refused_count(), kc.run_refused, name, at, _form(at), emu("stark"), coracle, "stark")


@pytest.mark.parametrize("curve,name,at", [(c, n, kc.REFUSED_AT[(i + j) % 3]) for j, c in enumerate(kc.CURVES[1:])
                                           for i, n in enumerate(kc.defects(c))]
                         + [("bls12_377", "outside the subgroup", a) for a in kc.REFUSED_AT[1:]])
def test_refused_keys_on_the_other_curves(emu, coracle, curve, name, at):
    _run(kc.refused_count(), kc.run_refused, name, at, "dev", emu(curve), coracle, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_near_misses_enter_the_set(emu, coracle, curve):
    _run(kc.near_miss_count(), kc.run_near_miss, "host", emu(curve), coracle, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_malformed_slots_arrays_change_nothing(emu, coracle, curve):
    _run(kc.bad_slots_count(), kc.run_bad_slots, emu(curve), coracle, curve)


@pytest.mark.parametrize("curve", kc.CURVES)
def test_cleared_slots_are_empty_and_their_neighbours_untouched(emu, coracle, curve):
    _run(kc.clear_count(), kc.run_clear, "dev", emu(curve), coracle, curve)


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
def test_one_key_past_a_build_slice(emu_slice, coracle, curve):
    _run(kc.slice_count(), kc.run_slice, LOWERED_SLICE, "dev", emu_slice(curve), coracle, curve)


def test_chains_verified_by_one_index_per_table(emu, coracle):
    _run(kc.chains_count(kc.CHAIN_MODES, (0, 1, 2)), kc.run_chains, kc.CHAIN_MODES, (0, 1, 2), emu("stark"), coracle, "stark")


@pytest.mark.parametrize("curve", kc.CURVES[1:])
def test_one_chain_case_on_the_other_curves(emu, coracle, curve):
    """binary pieces; three honest tables around one past the set and one on an empty slot"""
    _run(kc.chains_count((1,), (2,)), kc.run_chains, (1,), (2,), emu(curve), coracle, curve)


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
def test_the_seeded_prover_by_index(emu, coracle, curve):
    _run(kc.seeded_count(), kc.run_seeded, emu(curve), coracle, curve)


def test_cpp_mirror_key_set_members(emu, tmp_path):
    """key_set, key_set_update, key_set_clear, key_set_live and verify_shuffle_chains by index of include/barnett_smart.hpp, compiled with
    g++ and run against the emulator library"""
    exe = tmp_path / "mirror_keyset"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mirror_keyset.cpp"),
                           "-L", HOSTEMU, "-lmpemu", "-Wl,-rpath," + HOSTEMU, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mirror_keyset ok" in out.stdout, out.stdout + out.stderr


def _run_deal(want, fn, *args):
    fails, checks = fn(*args)
    assert not fails, "\n".join(fails[:40])
    assert checks == want


@pytest.mark.parametrize("shape", kc.DEAL_SHAPES, ids=lambda s: "C=%d" % s[0])
def test_dealing_by_index_gives_the_oracles_bytes_and_those_of_the_keyed_calls(emu, coracle, shape):
    import torch
    _run_deal(kc.deal_count([shape]), kc.run_deal, [shape], emu("stark"), coracle, "stark", torch, "cpu")


@pytest.mark.parametrize("curve", kc.CURVES[1:])
def test_one_deal_case_on_the_other_curves(emu, coracle, curve):
    import torch
    _run_deal(kc.deal_count([(65, 7)]), kc.run_deal, [(65, 7)], emu(curve), coracle, curve, torch, "cpu")


def test_the_verifier_by_index_takes_one_defect_per_lane_screened_or_not(emu, coracle):
    _run_deal(kc.deal_defects_count("stark"), kc.run_deal_defects, emu("stark"), coracle, "stark")


@pytest.mark.parametrize("curve", ["stark", "bls12_377"])
def test_seating_straight_into_a_set(emu, coracle, curve):
    import torch
    _run_deal(kc.seat_count(), kc.run_seat, emu(curve), coracle, curve, torch, "cpu")
