"""Chunked workgroup rows (csrc/vgl_chunks.h) on the GPU, through the four algorithms that cut a long row into pieces: multi_source_bfs (the flat
mapping on the team), minimum_spanning_forest (the flat mapping), core_numbers and betweenness_centrality (the 2-D grid).  Rows that end on, one
before and one past a chunk boundary, and the one row length at which the clamp on the number of chunks starts to act.  Every result is compared with
the reference and under the comparison of the algorithm's own test file; every run must have launched its chunked kernel."""
import numpy as np
import pytest
import torch

import kcore_reference
import msbfs_reference
import msf_reference
import test_bc_gpu as BC
import test_kcore_gpu as KC
import test_msbfs_gpu as MS
import test_msf_gpu as MSF

pytestmark = pytest.mark.gpu
CHUNK = 16                                             # VGL_<ALG>_CHUNK of every shrunk set
MSBFS_SHRUNK = {"VGL_MSBFS_SHORT": "4", "VGL_MSBFS_WAVE": "16", "VGL_MSBFS_CHUNK": "16"}       # test_every_row_class_with_shrunk_thresholds
# bc's chunked class is its fourth (hub: longer than VGL_BC_WG, 64 in its shrunk set); at VGL_BC_WG = VGL_BC_WAVE the same rows are chunked as in the others
BC_SHRUNK = dict(BC.SHRUNK, VGL_BC_WG=BC.SHRUNK["VGL_BC_WAVE"])
# centre degrees: wave bound + 1 (9 for kcore and msf, 17 for msbfs and bc), c - 1, c, c + 1, 2c - 1, 2c, 2c + 1, 3c, 3c + 1; those at or below
# an algorithm's wave bound are rows of its other classes there
DEGREES = (9, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK, 3 * CHUNK + 1)


def stars(degrees):
    """disjoint stars stored both ways: (V, src, dst, centres, first leaves, last leaves); star j is its centre followed by its leaves"""
    src, dst, centres, first, last = [], [], [], [], []
    V = 0
    for d in degrees:
        leaves = np.arange(V + 1, V + 1 + d, dtype=np.int64)
        src += [np.full(d, V, dtype=np.int64), leaves]
        dst += [leaves, np.full(d, V, dtype=np.int64)]
        centres.append(V)
        first.append(V + 1)
        last.append(V + d)
        V += d + 1
    return V, np.concatenate(src), np.concatenate(dst), centres, first, last


def set_env(monkeypatch, switches):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)


def chunked(degrees, wave):
    return [d for d in degrees if d > wave]


def test_degrees_cover_the_boundaries():
    assert chunked(DEGREES, 8) == [9, 15, 16, 17, 31, 32, 33, 48, 49] and chunked(DEGREES, 16) == [17, 31, 32, 33, 48, 49]
    assert int(MSBFS_SHRUNK["VGL_MSBFS_CHUNK"]) == int(KC.SHRUNK["VGL_KCORE_CHUNK"]) == int(MSF.SHRUNK["VGL_MSF_CHUNK"]) == int(BC_SHRUNK["VGL_BC_CHUNK"]) == CHUNK
    assert int(KC.SHRUNK["VGL_KCORE_WAVE"]) == int(MSF.SHRUNK["VGL_MSF_WAVE"]) == 8 and int(MSBFS_SHRUNK["VGL_MSBFS_WAVE"]) == int(BC_SHRUNK["VGL_BC_WG"]) == 16


@pytest.fixture(scope="module")
def boundary():
    return stars(DEGREES)


def test_msbfs_rows_on_chunk_boundaries(boundary, ctx, monkeypatch):
    """sources on the centre, the first and the last leaf of every star: a push from a centre must reach every entry of its row, and a pull into a
    centre finds its one source bit in the first or the last entry of the row"""
    A = MS.api()
    V, src, dst, centres, first, last = boundary
    set_env(monkeypatch, MSBFS_SHRUNK)
    sources = centres + first + last
    ref = msbfs_reference.multi_source_bfs(V, src, dst, sources, want_levels=True)
    g = A.Graph.from_coo(ctx, V, *MS.coo(ctx, src, dst))
    for mode in ("push", "pull"):
        monkeypatch.setenv("VGL_MSBFS_MODE", mode)
        ctx.timing(True)
        MS.assert_equals_reference(g, V, src, dst, sources, "stars, " + mode, ref=ref)
        n = MS.launches(ctx)
        ctx.timing(False)
        assert n["msbfs_%s_wg" % mode] > 0, n
    g.close()


def test_kcore_rows_on_chunk_boundaries(boundary, ctx, monkeypatch):
    A = KC.api()
    V, src, dst, _, _, _ = boundary
    set_env(monkeypatch, KC.SHRUNK)
    ref = kcore_reference.core_numbers(V, src, dst)
    g = A.Graph.from_coo(ctx, V, *KC.coo(ctx, src, dst))
    ctx.timing(True)
    st = KC.assert_equals_reference(g, ref, "stars")
    n = KC.launches(ctx)
    ctx.timing(False)
    assert n["kcore_wg"] > 0, n
    assert st["edges_examined"] == 2 * sum(DEGREES), st["edges_examined"]          # every row is walked once, whole: no piece twice, none dropped
    g.close()


def test_msf_rows_on_chunk_boundaries(boundary, ctx, monkeypatch):
    """the lightest edge of every centre is its last entry"""
    A = MSF.api()
    V, src, dst, centres, _, last = boundary
    set_env(monkeypatch, MSF.SHRUNK)
    centre, leaf = np.minimum(src, dst), np.maximum(src, dst)
    w = (1 + np.asarray(last)[np.searchsorted(centres, centre)] - leaf).astype(np.float32)      # the same both ways: 1 at the last leaf, the degree at the first
    assert np.array_equal(w[np.isin(leaf, last)], np.ones(2 * len(last), dtype=np.float32)) and w.max() == max(DEGREES)
    ref = msf_reference.minimum_spanning_forest(V, src, dst, w)
    g = A.Graph.from_coo(ctx, V, MSF.dev(ctx, src, np.int32), MSF.dev(ctx, dst, np.int32), want_perm=True)
    ctx.timing(True)
    MSF.assert_equals_reference(g, MSF.csr_weights(ctx, g, MSF.dev(ctx, w, np.float32)), ref, "stars")
    n = MSF.launches(ctx)
    ctx.timing(False)
    assert n["msf_min_wg"] > 0, n
    g.close()


def test_bc_rows_on_chunk_boundaries(boundary, ctx, monkeypatch):
    A = BC.api()
    V, src, dst, centres, first, last = boundary
    set_env(monkeypatch, BC_SHRUNK)
    g = A.Graph.from_coo(ctx, V, *BC.coo(ctx, src, dst))
    ctx.timing(True)
    BC.assert_equals_reference(g, V, src, dst, centres + first + last, "stars")
    fwd, bwd = BC.sweep_launches(ctx, "forward"), BC.sweep_launches(ctx, "backward")
    ctx.timing(False)
    assert fwd["hub"] > 0 and bwd["hub"] > 0, (fwd, bwd)
    g.close()


CLAMP_LEAVES = 16 * 32768 + 1                          # the shortest row whose chunk the clamp raises (to 17: 30841 chunks)


@pytest.fixture(scope="module")
def clamp_star():
    return stars([CLAMP_LEAVES])


def test_msbfs_at_the_chunk_clamp(clamp_star, ctx, monkeypatch):
    A = MS.api()
    V, src, dst, _, _, _ = clamp_star
    k = CLAMP_LEAVES
    set_env(monkeypatch, MSBFS_SHRUNK)
    g = A.Graph.from_coo(ctx, V, *MS.coo(ctx, src, dst))
    leaf_h = float(np.float64(1.0) / np.float64(1.0) + np.float64(k - 1) / np.float64(2.0))
    for mode in ("push", "pull"):
        monkeypatch.setenv("VGL_MSBFS_MODE", mode)
        ctx.timing(True)
        got, st = A.multi_source_bfs(g, [0, 1, 2, k])
        n = MS.launches(ctx)
        ctx.timing(False)
        print(mode, st, n)
        assert n["msbfs_%s_wg" % mode] > 0, n
        assert got["reached"].tolist() == [k + 1] * 4 and got["dist_sum"].tolist() == [k] + [1 + 2 * (k - 1)] * 3
        assert got["ecc"].tolist() == [1, 2, 2, 2] and got["harmonic"].tolist() == [float(k)] + [leaf_h] * 3
        assert st["levels_total"] == 3 and st["reached_total"] == 4 * (k + 1)
        if mode == "push":                                                  # the centre and three leaves; the centre and all leaves; all leaves
            assert st["edges_push"] == (k + 3) + 2 * k + k
    g.close()


def test_kcore_at_the_chunk_clamp(clamp_star, ctx, monkeypatch):
    A = KC.api()
    V, src, dst, _, _, _ = clamp_star
    set_env(monkeypatch, KC.SHRUNK)
    g = A.Graph.from_coo(ctx, V, *KC.coo(ctx, src, dst))
    ctx.timing(True)
    top, st = A.core_numbers(g)
    n = KC.launches(ctx)
    ctx.timing(False)
    print({k: v for k, v in st.items() if not torch.is_tensor(v)}, n)
    assert n["kcore_wg"] > 0, n
    assert top == 1 and bool((st["core"] == 1).all())
    assert st["edges_examined"] == 2 * CLAMP_LEAVES and st["max_degree"] == CLAMP_LEAVES
    g.close()
