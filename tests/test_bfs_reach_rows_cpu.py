"""The shapes of tests/bfs_reach_rows_reference.py are what tests/test_bfs_reach_rows_gpu.py needs them to be, asserted without a GPU: where
reach_rows falls, which sources lie beyond the rows the bounded scan launches, and -- with the rule of tests/bfs_schedule_reference.py -- that
every traversal from a source with entries reaches the scan of `levels` and turns bottom-up after it, with the list kernel on and off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_reach_rows_reference as RR  # noqa: E402
import bfs_schedule_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def shapes():
    return {name: RR.shape(name) for name in RR.LAYOUT}


def test_reach_rows_fall_where_the_cases_need_them(shapes):
    rr = {name: s.reach_rows for name, s in shapes.items()}
    assert rr == {name: core for name, (core, _) in RR.LAYOUT.items()}
    assert rr["mid_byte"] % 8 != 0 and rr["mid_byte"] > RR.TILE
    assert rr["mid_word"] % 8 == 0 and rr["mid_word"] % 64 != 0
    assert rr["mid_tile"] % 64 == 0 and rr["mid_tile"] % RR.TILE != 0
    assert rr["first_tile"] < RR.TILE and RR.scan_tiles(rr["first_tile"], shapes["first_tile"].V) == 1 < -(-shapes["first_tile"].V // RR.TILE) - 1
    assert rr["whole"] == shapes["whole"].V and shapes["whole"].V % 64 != 0
    for name, s in shapes.items():
        in_deg = np.bincount(s.dst, minlength=s.V)
        assert (in_deg[:s.reach_rows] > 0).all() and (in_deg[s.reach_rows:] == 0).all(), name
        if name != "whole":
            assert s.V % 64 != 0 and RR.scan_tiles(s.reach_rows, s.V) < -(-s.V // RR.TILE), name


def test_sources_are_of_their_kind(shapes):
    for name, s in shapes.items():
        out_deg, in_deg = np.bincount(s.src, minlength=s.V), np.bincount(s.dst, minlength=s.V)
        scanned = RR.scan_tiles(s.reach_rows, s.V) * RR.TILE
        assert s.sources["inside"] < s.reach_rows and in_deg[s.sources["inside"]] > 0
        if name == "whole":
            assert set(s.sources) == {"inside"}
            continue
        for kind in ("near", "far", "far2"):
            v = s.sources[kind]
            assert v >= s.reach_rows and out_deg[v] > 0 and in_deg[v] == 0, (name, kind)
        assert s.sources["near"] < scanned <= s.sources["far"] < s.sources["far2"], name
        assert s.sources["far"] // 8 == s.sources["far2"] // 8, name           # one byte of the bitmaps holds both
        v = s.sources["isolated"]
        assert v >= scanned and out_deg[v] == 0 and in_deg[v] == 0, name


@pytest.mark.parametrize("name", list(RR.LAYOUT))
def test_every_source_with_entries_reaches_the_scan_and_turns_bottom_up(shapes, name):
    s = shapes[name]
    for kind, v in s.sources.items():
        levels, records = R.schedule(s.V, s.src, s.dst, v)
        if kind == "isolated":
            assert len(records) == 1 and records[0].M == 0 and (levels >= 0).sum() == 1
            continue
        for env in RR.SCAN_ENV:
            assert RR.scans_then_bottom_up(s.V, s.dst, records, env), (name, kind, env, R.directions(records))
        # with the list kernel off the level before that one is scanned for too, and stays top-down: the count after that scan is taken off
        # bm_front, where a stale bit of the source would be counted
        assert records[0].direction == R.TOP_DOWN and records[1].direction == R.TOP_DOWN and records[2].direction == R.BOTTOM_UP, (name, kind)
        assert records[0].M > 0 and records[1].M > RR.small_m(s.V, {}) > 0, (name, kind)


def test_many_tiles_shape_reaches_the_scan(oracle):
    """the large shape: more tiles below reach_rows than the scan has workgroups, so that some workgroups take two tiles per trip"""
    s = RR.many_tiles()
    tiles = RR.scan_tiles(s.reach_rows, s.V)
    assert RR.SCAN_BLOCKS + 64 < tiles < -(-s.V // RR.TILE) and tiles * RR.TILE <= s.V and s.V % 64 != 0
    assert s.reach_rows % RR.TILE != 0 and s.sources["near"] >= s.reach_rows and s.sources["near"] < tiles * RR.TILE <= s.sources["far"]
    in_deg = np.bincount(s.dst, minlength=s.V)
    assert (in_deg[s.reach_rows:] == 0).all() and in_deg[s.sources["inside"]] > 0
    rowptr, adj, _ = oracle.coo_to_csr(s.V, s.src, s.dst)
    for kind in ("inside", "near", "far"):
        levels = oracle.bfs_top_down(rowptr, adj, s.sources[kind])[0]
        records = RR.records_of_levels(s.V, s.src, s.dst, levels)
        for env in RR.SCAN_ENV:
            assert RR.scans_then_bottom_up(s.V, s.dst, records, env), (kind, env, R.directions(records))
        assert records[0].direction == R.TOP_DOWN and records[1].direction == R.TOP_DOWN and records[0].M > 0, kind
