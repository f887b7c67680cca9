"""CPU: the HOST half of tests/test_gpu_xyzz_edges.py -- the same records at the corners of the stored-point contract through the
XYZZ laws as g++ compiles them (portable loops, limb-bound checker armed), against the formula model of tests/xyzz_edge_cases.py.
What this proves without a GPU: every record respects the contract (no 64-bit column overflows, no biased subtraction underflows
anywhere inside a law), the model is right on every branch, and every output is a stored point again.  The GPU test then requires
the device build -- one-lane, four-lane and two-lane forms -- to return the same limbs / residues."""
import pytest

import test_gpu_devtest as g
import test_gpu_xyzz_edges as e


@pytest.fixture(scope="module")
def host_libs(built):
    return g.load_libs(False)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_madd_edges_host(host_libs, cid):
    e.check_madd(host_libs, cid, e.N_RECORDS)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_add_edges_host(host_libs, cid):
    e.check_add(host_libs, cid, e.N_RECORDS)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_dbl_edges_host(host_libs, cid):
    e.check_dbl(host_libs, cid, e.N_RECORDS)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_trajectories_host(host_libs, cid):
    e.check_trajectories(host_libs, cid, e.N_TRAJECTORIES, e.N_ROUNDS)
