"""GPU test of the operator primitives one by one: apps/primitives_contract.cpp checks compute, reduce, generate_new_frontier, the three advance
kernels, VGL_SRC_ID_ADD and copy_if_indexes against host evaluations (families A .. G in its head comment).  Here it runs on the ragged inputs of
tests/primitives_graphs.py -- sizes that are no multiple of any tile, empty rows, rows longer than a chunk, stretches of nearly empty rows -- whose
branch coverage tests/test_primitives_graphs_cpu.py proves without a GPU, and the program's own coverage facts must confirm that the branches ran."""
import os
import re
import subprocess

import pytest

import primitives_graphs as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "apps", "bin", "primitives_contract_hip")
FACTS = ("unstaged_sparse_tiles", "rows_longer_than_chunk", "row_blocks_over_one_chunk", "combined_add_wavefronts", "mixed_add_wavefronts",
         "v_mod_8_nonzero", "v_mod_256_nonzero", "v_mod_2048_nonzero")


def run_program(args):
    out = subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text
    assert re.search(r"^error count: 0$", out.stdout, re.M), text
    assert "FAILED" not in out.stdout, text
    facts = {k: int(v) for k, v in re.findall(r"^coverage: (\w+) = (-?\d+)$", out.stdout, re.M)}
    assert set(facts) == set(FACTS), text
    return facts


@pytest.mark.parametrize("fmt", ["csr", "vcsr"])
@pytest.mark.parametrize("name", list(P.GRAPHS))
def test_primitives_on_ragged_graphs(name, fmt, tmp_path, oracle, ctx):
    V, src, dst = P.GRAPHS[name]()
    path = str(tmp_path / (name + ".el_container"))
    oracle.write_el_container(path, V, src, dst)
    facts = run_program(["-import", path, "-format", fmt])
    if name != "ragged":
        return
    assert all(facts[k] > 0 for k in FACTS), facts                     # no branch was skipped
    if fmt == "csr":                                                   # the ids are the input's: the static facts are those numpy derives
        want = {}
        for rowptr, _ in P.both_directions(V, src, dst):
            for k, v in P.coverage(rowptr, V).items():
                want[k] = want.get(k, 0) + v
        for k in ("rows_longer_than_chunk", "row_blocks_over_one_chunk", "combined_add_wavefronts", "mixed_add_wavefronts"):
            assert facts[k] == want[k], (k, facts, want)
        assert facts["unstaged_sparse_tiles"] >= want["unstaged_sparse_tiles"]      # (the program adds up every sparse advance it checks)


@pytest.mark.parametrize("fmt", ["csr", "vcsr"])
def test_primitives_on_rmat(fmt, ctx):
    """the common shape: V = 2^12, edge factor 16"""
    run_program(["-s", 12, "-e", 16, "-type", "rmat", "-format", fmt])
