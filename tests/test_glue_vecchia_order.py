"""The ordering shim of glue/cocons_hip_glue.c EXECUTED against the R C-API stand-in, the way tests/test_glue_vecchia_knn.py
drives the neighbour-search shims: on the GPU `_cocons_hip_vecchia_order` returns what the Python layer returns, to the bit
(its registration and refusals: tests/test_order_abi.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import order_reference as OR  # noqa: E402
from test_glue_exec import RStub  # noqa: E402


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["uniform 65", "uniform 641", "lattice / 39"])
def test_the_r_wrapper_equals_python(name):
    import cocons_amd as ca
    R = RStub()
    locs, want, _ = OR.reference(name)
    got = R.value(R.call("_cocons_hip_vecchia_order", R.real(np.array(locs)), R.integer([0])))
    got = np.asarray(got).ravel()
    print("order-report glue | the order through the R wrapper | %s | positions that differ %d"
          % (name, int(np.count_nonzero(got != want))))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, ca.vecchia_order_device(locs))
