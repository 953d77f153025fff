"""Chunked workgroup rows (csrc/vgl_chunks.h, host and device): a stand-alone program built with the host compiler against a restatement.
The rule: chunk = max(switch, ceil(max(longest, 1) / 32768)), nchunks = max(1, ceil(max(longest, 1) / chunk)); piece k of a row is
[row_lo + k * chunk, min(row_end, row_lo + (k + 1) * chunk)) and is empty when it starts at or past row_end; item it of the flat forms
is (row it // nchunks, piece it % nchunks)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CHUNKS = 32768
FIRST_ENTRY = 1000              # where the program lays the first row

# (switch's chunk, longest row)
CASES = [(16, 0), (16, 1), (16, 15), (16, 16), (16, 17), (16, 16 * 32768), (16, 16 * 32768 + 1), (16384, 1 << 40), (1 << 28, 5)]


def ceil_div(a, b):
    return -(-a // b)


def chunks_of(env, longest):
    longest = max(longest, 1)
    chunk = max(env, ceil_div(longest, MAX_CHUNKS))
    return chunk, max(1, ceil_div(longest, chunk))


def pieces_of(chunk, nchunks, lo, end):
    return [(k, lo + k * chunk, min(end, lo + (k + 1) * chunk)) for k in range(nchunks) if lo + k * chunk < end]


def row_lengths(chunk, longest):
    return [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, longest]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("chunks") / "rc_chunks")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "rc_chunks_main.cpp")], check=True, timeout=300)
    return exe


def test_chunks_match_the_rule(program):
    text = ""
    for env, longest in CASES:
        lens = row_lengths(chunks_of(env, longest)[0], longest)
        text += "%d %d %d %s\n" % (env, longest, len(lens), " ".join(map(str, lens)))
    out = subprocess.run([program], input=text, capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    at = 0
    for env, longest in CASES:
        name = "switch %d, longest row %d" % (env, longest)
        chunk, nchunks = [int(x) for x in out[at].split()]
        at += 1
        assert (chunk, nchunks) == chunks_of(env, longest), name
        assert nchunks <= MAX_CHUNKS and chunk >= env and nchunks * chunk >= longest, name
        row_lo = FIRST_ENTRY
        for length in row_lengths(chunk, longest):
            got = [int(x) for x in out[at].split()]
            at += 1
            row_end = row_lo + length
            assert got[:2] == [row_lo, row_end] and got[-1] == 1, (name, length)              # the last figure: split inverts row * nchunks + k
            got_pieces = list(zip(got[2:-1:3], got[3:-1:3], got[4:-1:3]))
            assert len(got) == 3 + 3 * len(got_pieces), (name, length)
            # a row within the longest is tiled once, in order, by pieces of 1 .. chunk entries; a longer row by its first nchunks pieces
            covered = min(length, nchunks * chunk)
            edge = row_lo
            for i, (k, lo, hi) in enumerate(got_pieces):
                assert k == i and lo == edge and lo < hi <= lo + chunk, (name, length, k)
                edge = hi
            assert edge == row_lo + covered, (name, length)
            assert got_pieces == pieces_of(chunk, nchunks, row_lo, row_end), (name, length)
            row_lo = row_end
    assert at == len(out)


def test_restatement_on_the_named_cases():
    # the restatement itself, by hand
    assert chunks_of(16, 0) == (16, 1)
    assert chunks_of(16, 1) == (16, 1)
    assert chunks_of(16, 15) == (16, 1)
    assert chunks_of(16, 16) == (16, 1)
    assert chunks_of(16, 17) == (16, 2)
    assert chunks_of(16, 16 * 32768) == (16, 32768)                 # the last row length the switch's chunk serves
    assert chunks_of(16, 16 * 32768 + 1) == (17, 30841)             # 17 * 30840 = 524280 < 524289 <= 17 * 30841
    assert chunks_of(16384, 1 << 40) == (1 << 25, 32768)
    assert chunks_of(1 << 28, 5) == (1 << 28, 1)
    assert pieces_of(16, 2, 1000, 1000) == []
    assert pieces_of(16, 2, 1000, 1015) == [(0, 1000, 1015)]
    assert pieces_of(16, 2, 1000, 1016) == [(0, 1000, 1016)]        # a row of exactly one chunk has no second piece
    assert pieces_of(16, 2, 1000, 1017) == [(0, 1000, 1016), (1, 1016, 1017)]
    assert pieces_of(16, 3, 1000, 1032) == [(0, 1000, 1016), (1, 1016, 1032)]
