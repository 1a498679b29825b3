"""CPU tests (-m "not gpu") of the split bucket pipeline at chunk, mode and bucket-range edges (tests/bucket_split_cases.py) with the
kernel bodies under the development emulator (tools/hostemu).  At the engine's chunk of 24 576 terms a multi-chunk case takes the
emulator tens of seconds, so the multi-chunk cases run against a second emulator library built with a chunk of 1 024 terms
(make CHUNK=1024: MP_EXP_BK_CHUNK) -- every family on STARK, BLS12-377 and secp256k1 --, and the ordinary libmpemu.so runs
what has one run per bucket: family A up to one full chunk (K = 24 575 and 24 576 included), D and E.  Every call checks the number
of k_bucket_sort workgroups against the chunk it was built for, so a library with another chunk size fails every multi-chunk case.
tests/test_gpu_bucket_split.py runs all of it at 24 576 on gfx950.

The construction check needs no engine: every case of both chunk sizes against the digit model, with the edge each case reaches
printed (pytest -s)."""
import ctypes
import os
import subprocess

import pytest

import bucket_split_cases as bsc
from conftest import ROOT


def _emu(mp, chunk):
    mp.build()
    d = os.path.join(ROOT, "tools", "hostemu")
    subprocess.check_call(["make", "-s", "-j8", "-C", d] + (["CHUNK=%d" % chunk] if chunk else []))
    lib = mp._native.bind(ctypes.CDLL(os.path.join(d, "libmpemu_chunk%d.so" % chunk if chunk else "libmpemu.so")))
    return lambda curve: mp._native.Engine(curve, 0, lib=lib)


@pytest.fixture(scope="module")
def emu_small(mp):
    return _emu(mp, bsc.CHUNK_EMU)


@pytest.fixture(scope="module")
def emu(mp):
    return _emu(mp, 0)


def _run(fn, *args, **kw):
    fails, checks = fn(*args, **kw)
    assert not fails, "\n".join(fails[:40])
    assert checks > 0
    return checks


def test_geometry_is_the_engines():
    assert bsc.geometry_is_the_engines() == []
    g = bsc.Geo(14, bsc.CHUNK_GPU)
    assert (g.NBK, g.T, g.NBP, g.units, g.Q, g.packed) == (8192, 56, 256, 32, 2048, True)
    g = bsc.Geo(10, bsc.CHUNK_GPU)
    assert (g.NBK, g.T, g.NBP, g.units, g.Q, g.packed) == (512, 416, 256, 2, 128, False)
    assert [g.chunks(K) for K in (1, 24575, 24576, 24577, 49152, 49153, 49216)] == [1, 1, 1, 2, 2, 3, 3]


@pytest.mark.parametrize("chunk", [bsc.CHUNK_EMU, bsc.CHUNK_GPU])
@pytest.mark.parametrize("curve", list(bsc.WIDTHS))
def test_constructions_reach_their_edges(curve, chunk):
    fails, checks, lines = bsc.self_check(chunk, curves=(curve,))
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:40])
    assert checks == len(lines) > 0


@pytest.mark.parametrize("fam", bsc.FAMILIES)
@pytest.mark.parametrize("curve", list(bsc.WIDTHS))
def test_split_pipeline_edges_chunk_1024(emu_small, coracle, curve, fam):
    eng = emu_small(curve)
    try:
        _run(bsc.run_family, eng, coracle, curve, fam, bsc.CHUNK_EMU)
    finally:
        eng.close()


@pytest.mark.parametrize("fam", ["A", "D", "E"])
def test_split_pipeline_edges_one_run_per_bucket(emu, coracle, fam):
    eng = emu("stark")
    try:
        _run(bsc.run_family, eng, coracle, "stark", fam, bsc.CHUNK_GPU, single_chunk=True)
    finally:
        eng.close()
