"""The host twins of the backward walk (smc_host_smooth, smc_host_sample_paths, smc_host_rb_sample_paths) against their own
bits as recorded before they came to share their helpers (tests/golden/backward_twins.npz, make_golden.py backward_twins).
The other host tests compare the twins with long-double references within a tolerance and would not see another order of
summation or selection; the device tests compare with the twins.  Inputs come from the file as well.  No GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden as G  # noqa: E402

RECORDS = [("%s_n%d" % (fam, n), "%s_n%d" % (fam, n)) for fam, spec in G.BACKWARD_FAMILIES.items() for n in spec[3]]
RECORDS += [(fam + "_dead", fam + "_n65") for fam in G.BACKWARD_FAMILIES]
OUTPUTS = {True: ("idx", "vol", "tmean", "tvar", "tdraw", "out"), False: ("ws", "mean", "var", "idx", "xs")}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "backward_twins.npz")) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


@pytest.mark.parametrize("name,source", RECORDS, ids=[r[0] for r in RECORDS])
def test_twins_reproduce_their_recorded_bits(L, golden, name, source):
    fam = name.split("_")[0]
    x, w = golden[source + "/x"], golden[source + "/w"]
    if name.endswith("_dead"):
        w = w.copy()
        w[G.BACKWARD_DEAD_T] = 0.0
    got = G.backward_twin_outputs(L, fam, x, w, golden["y"])
    assert set(got) == set(OUTPUTS[fam == "rb"])
    for k, v in got.items():
        ref = golden[name + "/" + k]
        assert v.dtype == ref.dtype and v.shape == ref.shape, k
        assert np.array_equal(bits(v), bits(ref)), (name, k)           # (the uint64 view: NaNs count)


@pytest.mark.parametrize("fam", list(G.BACKWARD_FAMILIES))
def test_fixture_holds_complete_and_refused_paths(golden, fam):
    idx = [golden[name + "/idx"] for name, _ in RECORDS if name.split("_")[0] == fam]
    assert sum(int(np.sum(np.all(i >= 0, axis=0))) for i in idx) > 0
    assert sum(int(np.sum(i == -1)) for i in idx) > 0
