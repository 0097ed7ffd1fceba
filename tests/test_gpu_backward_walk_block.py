"""The block of the backward walk on the GPU (pytest -m gpu): smc_sample_paths and smc_rb_sample_paths share one walk and one
block on the handle (hist.d_path, DESIGN.md "History on a handle"), which grows when a call needs more and is kept otherwise.
M = 5, then M = 70 (the block grows), then M = 5 again (in the larger block): the first and the third call agree bit for bit,
and every call equals the host twin."""
import numpy as np
import pytest

import test_gpu_backward_paths as BP
import test_gpu_rb_paths as RP

pytestmark = pytest.mark.gpu

N, SEG, NTH, T = 130, 256, 3, 4


def test_sample_paths_across_a_regrown_block(L):
    rows = BP.rows_for(BP.LG, NTH)
    h = BP.run_recorded(L, 1, rows, N, SEG, T)
    res = [BP.compare_with_host(L, h, 1, rows, M)[2:] for M in (5, 70, 5)]
    assert np.array_equal(res[0][0], res[2][0]) and BP.same(res[0][1], res[2][1])
    assert np.all(res[1][0] >= 0)
    h.close()


def test_rb_sample_paths_across_a_regrown_block(L):
    rows = RP.rows_for(NTH)
    h, y = RP.run_recorded(L, rows, N, SEG, T)
    res = [RP.compare_with_host(L, h, rows, y, M)[2] for M in (5, 70, 5)]
    assert np.array_equal(res[0]["idx"], res[2]["idx"])
    for k in RP.KEYS:
        assert RP.same(res[0][k], res[2][k]), k
    assert np.all(res[1]["idx"] >= 0)
    h.close()
