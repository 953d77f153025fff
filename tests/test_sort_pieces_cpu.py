"""The piece planner of the piecewise key sorts (csrc/vgl_pieces.h, host only): a stand-alone program built with the host compiler
against a restatement of the rule.  The rule: rows are taken in order; a piece is closed before a row when it holds keys already and
the row would lift it above the cap, so a row above the cap is a piece of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MAX = (1 << 63) - 1


def plan(keys, cap):
    bounds, acc, largest = [0], 0, 0
    for i, k in enumerate(keys):
        if acc > 0 and acc + k > cap:
            bounds.append(i)
            largest = max(largest, acc)
            acc = 0
        acc += k
    bounds.append(len(keys))
    return [max(largest, acc)] + bounds


def cases():
    rng = np.random.default_rng(20261020)
    random_rows = [int(x) for x in np.minimum(rng.geometric(0.02, 100000) - 1, rng.integers(0, 4000, 100000))]
    big = 1 << 40
    out = [
        ("no rows", [], 8),
        ("all rows empty", [0] * 7, 8),
        ("cap 1", [0, 1, 3, 0, 0, 2, 1, 1, 0], 1),
        ("a row that fits exactly", [3, 5, 1, 7, 8, 0, 8], 8),
        ("a row one over the cap", [3, 6, 1, 7, 9, 0, 8, 1], 8),
        ("one row above the cap between small rows", [1, 2, 1, 100, 1, 2, 1], 8),
        ("no cap, counts near 2^40", [big - 1, big, big + 1, 0, big] * 3, INT64_MAX),
        ("cap just under the sum of two counts near 2^40", [big, big - 1, big, big, 1], 2 * big - 1),
    ]
    return out + [("random rows, cap %d" % cap, random_rows, cap) for cap in (1, 1000, 1 << 20)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pieces") / "sort_pieces")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "sort_pieces_main.cpp")], check=True, timeout=300)
    return exe


def test_pieces_match_the_rule(program):
    all_cases = cases()
    text = "".join("%d %d %s\n" % (cap, len(keys), " ".join(map(str, keys))) for _, keys, cap in all_cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    assert len(out) == len(all_cases)
    for (name, keys, cap), line in zip(all_cases, out):
        got, want = [int(x) for x in line.split()], plan(keys, cap)
        assert got == want, name
        bounds = want[1:]
        assert bounds[0] == 0 and bounds[-1] == len(keys), name
        assert not keys or all(a < b for a, b in zip(bounds, bounds[1:])), name      # no empty piece


def test_restatement_on_the_named_cases():
    # the restatement itself, by hand: largest piece, then the bounds
    assert plan([], 8) == [0, 0, 0]
    assert plan([0] * 7, 8) == [0, 0, 7]
    assert plan([0, 1, 3, 0, 0, 2, 1, 1, 0], 1) == [3, 0, 2, 3, 6, 7, 9]
    assert plan([3, 5, 1], 8) == [8, 0, 2, 3]                      # 3 + 5 == cap stays in the piece
    assert plan([3, 6, 1], 8) == [7, 0, 1, 3]                      # 3 + 6 is one over
    assert plan([1, 2, 1, 100, 1, 2, 1], 8) == [100, 0, 3, 4, 7]
