"""-m gpu: the split bucket pipeline (k_bucket_sort / k_bucket_acc / k_bucket_list / k_bucket_reduce / k_bucket_final) at chunk, mode
and bucket-range edges on the GPU -- the cases of tests/bucket_split_cases.py at the engine's chunk of 24 576 terms, which
tests/test_bucket_split_emu.py runs through the emulator at 1 024: lengths either side of a chunk boundary, a bucket exactly at the
list-mode threshold and one term past it, list-mode walks over empty buckets and short chunks, more runs than units, bucket layouts
that single out units, lanes and quarters, exceptional points inside a run, calls of several items in both modes, and small calls
after large ones -- through mp_msm, the result point byte for byte against the oracle's, every call checked to have run on the split
pipeline.  STARK: windows of 10, 12, 13 and 14 bits; BLS12-377 (14 limbs): 11 and 13; secp256k1 (256-bit order): 12."""
import pytest

import bucket_split_cases as bsc

pytestmark = pytest.mark.gpu

CASES = [(curve, fam) for curve in bsc.WIDTHS for fam in bsc.FAMILIES]


@pytest.mark.parametrize("curve,fam", CASES, ids=["%s-%s" % cf for cf in CASES])
def test_split_pipeline_edges(mp, coracle, curve, fam):
    eng = mp._native.Engine(curve, 0)
    try:
        fails, checks = bsc.run_family(eng, coracle, curve, fam, bsc.CHUNK_GPU)
    finally:
        eng.close()
    print("%s family %s: %d checks" % (curve, fam, checks))
    assert not fails, "\n".join(fails[:40])
    assert checks > 0
