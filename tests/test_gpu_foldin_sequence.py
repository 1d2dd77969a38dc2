"""The four fold-in setups one after the other on one handle (mfx_rec_fold_in_setup implicit, mfx_rec_fold_in_block_setup,
mfx_rec_fold_in_block_setup_als, mfx_rec_fold_in_setup explicit): they share their start (the device, the unpacked H, the
"not set up" mark), and each must leave nothing behind that the next one sees.  After each setup the solved rows pass the
check that the setup's own test applies to a fresh handle -- the bits of the single operator (tests/test_gpu_foldin.py) or
of the chained block halves (tests/test_gpu_foldin_block.py, tests/test_gpu_foldin_alsb.py) -- and rows, lists and scores
equal those of a fresh handle given that setup alone.

40 x 70 factors at k = 12 (one MFMA chunk, three item tiles, blocks of 5 + 5 + 2), 33 query rows of 1 to 5 entries: one
slot more than the 32 of a wave."""
import numpy as np
import pytest

from test_gpu_foldin import factors, same, segments
from test_gpu_foldin_block import LAM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mfx():
    import mfx as m
    assert m.device_count() >= 1, m.lib().mfx_last_error()
    return m


def test_the_setups_in_sequence_equal_each_alone(mfx):
    rows, cols, k, n_top, alpha, d, sweeps = 40, 70, 12, 5, 2.0, 5, 2
    sizes = np.random.default_rng(15).integers(1, 6, 33).tolist()
    assert min(sizes) >= 1 and max(sizes) <= 5
    ptr, idx, val = segments(15, cols, sizes)
    W, H = factors(15, cols, k, rows=rows)

    def chained(half):
        Y = None
        for _ in range(sweeps):
            Y = half(Y)
        return Y

    steps = [
        ("implicit", lambda r: r.fold_in_setup(mfx.MFX_FOLD_IMPLICIT, LAM, alpha),
         mfx.ials_half(ptr, idx, val, H, k, LAM, alpha)),
        ("implicit blocks", lambda r: r.fold_in_block_setup(LAM, alpha, block=d, sweeps=sweeps),
         chained(lambda Y: mfx.ials_block_half(ptr, idx, val, H, k, LAM, alpha, d, Y_in=Y))),
        ("explicit blocks", lambda r: r.fold_in_block_setup_als(LAM, block=d, sweeps=sweeps),
         chained(lambda Y: mfx.als_block_half(ptr, idx, val, H, k, LAM, d, Y_in=Y))),
        ("explicit", lambda r: r.fold_in_setup(mfx.MFX_FOLD_ALS, LAM),
         mfx.als_half(ptr, idx, val, H, k, LAM, variant=1)),
    ]
    assert len({w.tobytes() for _, _, w in steps}) == 4  # (the four setups do solve different rows)
    with mfx.Recommender(W, H, 1) as r:
        for name, setup, want in steps:
            setup(r)
            items, scores, got = r.fold_in((ptr, idx, val), n_top)
            assert same(got, want), name
            with mfx.Recommender(W, H, 1) as fresh:
                setup(fresh)
                fi, fs, fw = fresh.fold_in((ptr, idx, val), n_top)
            assert items.shape == (33, n_top) and np.array_equal(items, fi), name
            assert same(scores, fs) and same(got, fw), name
