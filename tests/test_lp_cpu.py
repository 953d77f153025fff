"""Label propagation without a GPU: the numpy restatement of the contract (tests/lp_reference.py) on hand-checked cases, and the build
products of the feature (header, exported symbols, Python entry point, the lp app)."""
import ctypes
import os
import re

import numpy as np
import pytest

import lp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_hand_cases(name):
    V, edges, init, max_it, want, iterations, history = R.HAND_CASES[name]
    src, dst = zip(*edges)
    rowptr, adj = R.csr_from_edges(V, src, dst)
    labels, its, hist = R.label_propagation(rowptr, adj, init, max_it)
    assert labels.dtype == np.int32
    assert labels.tolist() == want
    assert its == iterations and hist == history


def test_restatement_tie_goes_to_largest_label_whatever_the_order():
    rowptr = np.array([0, 4, 4, 4, 4, 4], dtype=np.int64)
    for adj in ([1, 2, 3, 4], [4, 3, 2, 1], [2, 4, 1, 3]):
        labels = R.lp_step(rowptr, np.array(adj), np.array([0, -3, 9, -3, 9], dtype=np.int32))
        assert labels[0] == 9


def test_restatement_zero_iterations_returns_the_start():
    rowptr, adj = R.csr_from_edges(3, [0, 1], [1, 2])
    labels, its, hist = R.label_propagation(rowptr, adj, [4, 5, 6], 0)
    assert labels.tolist() == [4, 5, 6] and its == 0 and hist == []


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_header_declares_lp(built):
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    assert re.search(r"\bint vgl_hip_lp_run\s*\(", text) and re.search(r"\bint vgl_hip_lp_prepare\s*\(", text)
    assert "vgl_hip_lp_stats" in text and "VGL_LP_AUTO" in text


def test_library_exports_lp(built):
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "vgl_hip_lp_run") and hasattr(L, "vgl_hip_lp_prepare")
    assert "vgl_hip_lp_run" in lib.EXPORTED_SYMBOLS and "vgl_hip_lp_prepare" in lib.EXPORTED_SYMBOLS
    assert [f for f, _ in lib.LpStats._fields_] == ["iterations", "converged", "frontier_steps", "changed_last", "rows_processed",
                                                     "edges_examined", "algorithmic_bytes"]


def test_python_entry_point(built):
    from vectorgraphlibrary_amd import api
    assert callable(api.label_propagation) and callable(api.Graph.prepare_label_propagation)
    assert (api.LP_ALL_ACTIVE, api.LP_FRONTIER, api.LP_AUTO) == (0, 1, 2)


def test_lp_app_built(built):
    assert os.access(os.path.join(ROOT, "apps", "bin", "lp_hip"), os.X_OK)
