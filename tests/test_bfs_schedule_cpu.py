"""The restatement of the direction-optimising BFS schedule (tests/bfs_schedule_reference.py) checked on the CPU before tests/test_bfs_schedule_gpu.py
compares the HIP traversal with it: its levels and top-down totals are those of oracle.bfs_top_down, the two inequalities of the direction rule hold
at their exact boundaries, and every shaped input still has the schedule it was built for -- a generator change that loses a path of the driver
fails here, not silently on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_schedule_reference as R  # noqa: E402

TD_EMIT_EDGES = 65536       # vgl_bfs_td_emit_edges for V < 2^24: heavier top-down levels leave their frontier in `levels` only
SMALL_F = 2048              # VGL_SMALL_F: the longest list the list kernel hands over as ids


@pytest.fixture(scope="module")
def shapes():
    out = {}
    for name, make in R.SHAPES.items():
        V, src, dst, source = make()
        levels, records = R.schedule(V, src, dst, source)
        out[name] = (V, src, dst, source, levels, records)
    return out


def check_against_oracle(O, V, src, dst, source):
    rowptr, adj, _ = O.coo_to_csr(V, src, dst)
    want, st = O.bfs_top_down(rowptr, adj, source)
    levels, records = R.schedule(V, src, dst, source)
    assert np.array_equal(levels, want)
    td_levels, td_records = R.schedule(V, src, dst, source, direction_optimising=False)
    assert np.array_equal(td_levels, want)
    assert all(r.direction == R.TOP_DOWN for r in td_records)
    e = R.expected(td_records)
    assert (e["levels"], e["td_edges"], e["frontier_total"], e["discovered"]) == \
        (st["levels"], st["edges_examined"], st["frontier_total"], st["discovered"])
    assert e["td_steps"] == e["levels"] and e["bu_steps"] == 0 and e["bu_found"] == 0 and e["td_frontier"] == e["frontier_total"]
    # either mode expands the same frontiers
    assert [(r.level, r.F, r.M, r.found, r.unvisited_in_entries) for r in records] == \
        [(r.level, r.F, r.M, r.found, r.unvisited_in_entries) for r in td_records]
    return records


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_levels_and_top_down_totals_on_shapes(oracle, name):
    V, src, dst, source = R.SHAPES[name]()
    assert V % 64 != 0 and V < 40000 and len(src) < 1200000
    check_against_oracle(oracle, V, src, dst, source)


def test_levels_and_top_down_totals_on_endings_union(oracle):
    V, src, dst, sources = R.endings_union()
    for source in sources.values():
        check_against_oracle(oracle, V, src, dst, source)


@pytest.mark.parametrize("kind,scale,ef,seed", [("rmat", 10, 8, 2), ("ru", 12, 16, 5)])       # tests/golden/{rmat_s10_e8_seed2,ru_s12_e16_seed5}.npz
def test_levels_and_top_down_totals_on_golden_generators(oracle, kind, scale, ef, seed):
    src, dst = (oracle.gen_rmat if kind == "rmat" else oracle.gen_uniform)(scale, ef, seed)
    V = 1 << scale
    out_deg = np.bincount(src, minlength=V)
    some_bottom_up = False
    for source in (int(np.argmax(out_deg)), int(np.nonzero(out_deg)[0][0]), int(np.argmin(out_deg))):
        records = check_against_oracle(oracle, V, src, dst, source)
        some_bottom_up |= any(r.direction == R.BOTTOM_UP for r in records)
    assert some_bottom_up


def test_levels_and_top_down_totals_on_study_graphs(oracle):
    for seed in range(20):
        V, src, dst, rng = R.study_graph(seed, log_v_end=14)
        assert V <= 1 << 13
        out_deg = np.bincount(src, minlength=V)
        for source in {int(rng.integers(0, V)), int(np.argmax(out_deg)), 0}:
            check_against_oracle(oracle, V, src, dst, source)


def test_unvisited_in_entries_is_what_the_name_says(shapes):
    V, src, dst, source, levels, records = shapes["hub_layer"]
    in_deg = np.bincount(dst, minlength=V)
    for r in records:
        unvisited = (levels < 0) | (levels > r.level)
        assert r.unvisited_in_entries == int(in_deg[unvisited].sum())
        assert r.found == int((levels == r.level + 1).sum()) and r.F == int((levels == r.level).sum())


# ---- the rule at its boundaries ----
def test_bottom_up_boundary():
    V, factor, visited, prev_f = 1000, 3, 100, 10
    threshold = ((V - visited) * factor + V) // 15
    assert threshold == 246 and ((V - visited) * factor + V) % 15 != 0          # the division truncates
    assert R.turn_bottom_up(11, threshold, prev_f, visited, V, factor)
    assert not R.turn_bottom_up(11, threshold - 1, prev_f, visited, V, factor)
    assert not R.turn_bottom_up(10, threshold, prev_f, visited, V, factor)      # F == prevF is not growing
    assert not R.turn_bottom_up(10, 10 ** 9, prev_f, visited, V, factor)
    assert not R.turn_bottom_up(9, 10 ** 9, prev_f, visited, V, factor)
    # every vertex visited: V / 15 edges are still needed
    assert R.turn_bottom_up(2, V // 15, 1, V, V, factor) and not R.turn_bottom_up(2, V // 15 - 1, 1, V, V, factor)


def test_top_down_boundary():
    V, factor, visited = 1000, 3, 100
    threshold = ((V - visited) * factor + V) // (factor * 18)
    assert threshold == 68 and ((V - visited) * factor + V) % (factor * 18) != 0
    assert R.turn_top_down(threshold - 1, threshold - 1, visited, V, factor)     # F == prevF can turn top-down
    assert R.turn_top_down(threshold - 1, 10 ** 6, visited, V, factor)
    assert not R.turn_top_down(threshold, 10 ** 6, visited, V, factor)           # F equal to the threshold stays
    assert not R.turn_top_down(threshold - 1, threshold - 2, visited, V, factor)  # growing stays, however small
    assert R.do_factor(1000, 3999) == 1 and R.do_factor(1000, 4000) == 2 and R.do_factor(1000, 0) == 1 and R.do_factor(7, 10 ** 6) == 71428


def test_schedule_applies_the_rule_with_the_frontier_counted_as_visited():
    """tiny graphs worked by hand (factor 1 in all of them)"""
    # a star, V 31, 30 entries: F 1 > 0, visited 1, M 30 >= (30 + 31) // 15 = 4: bottom-up at level 1; level 2 grows, so it stays
    _, records = R.schedule(31, np.zeros(30, np.int64), np.arange(1, 31), 0)
    assert R.directions(records) == "B2"
    # V 100, 0 -> 1, 1 -> 2 .. 51: level 2 has M 50 >= (98 + 100) // 15 = 13 but F 1 == prevF: top-down; level 3 grows but has no entries
    _, records = R.schedule(100, np.concatenate([[0], np.ones(50, np.int64)]), np.arange(1, 52), 0)
    assert R.directions(records) == "t3" and records[1].M == 50
    # 0 -> 1 .. 5 (M 5).  V 46: visited 1 gives (45 + 46) // 15 = 6 > 5: top-down
    _, records = R.schedule(46, np.zeros(5, np.int64), np.arange(1, 6), 0)
    assert records[0].direction == R.TOP_DOWN
    # V 45: visited 1 gives 89 // 15 = 5 <= 5: bottom-up; a `visited` that left the frontier out would give 90 // 15 = 6: top-down
    _, records = R.schedule(45, np.zeros(5, np.int64), np.arange(1, 6), 0)
    assert records[0].direction == R.BOTTOM_UP


# ---- every shape has the schedule it was built for ----
def test_two_bursts(shapes):
    V, src, dst, source, levels, records = shapes["two_bursts"]
    ph = R.phases(records)
    assert len(ph) >= 2
    back = R.switches_back(records)
    assert len(back) == len(ph) and all(r.F < 64 for r in back)
    for p in ph[:2]:
        assert len(p) >= 2 and p[0].F != p[1].F and abs(p[0].F - p[1].F) > 1          # a filter bound fits between them
    assert sum(r.direction == R.TOP_DOWN and r.F == 1 for r in records) >= 45        # the path between the clusters


def test_hub_source(shapes):
    V, src, dst, source, levels, records = shapes["hub_source"]
    assert 19000 < V < 21000
    assert records[0].direction == R.BOTTOM_UP and records[0].F == 1
    assert R.expected(records)["td_steps"] == 0 and records[-1].found == 0


def test_hub_layer(shapes):
    V, src, dst, source, levels, records = shapes["hub_layer"]
    assert records[0].direction == R.TOP_DOWN
    assert records[1].level == 2 and records[1].direction == R.BOTTOM_UP and records[1].F <= SMALL_F
    assert records[-1].direction == R.TOP_DOWN


@pytest.mark.parametrize("name,heavy_edges", [("heavy_not_growing", TD_EMIT_EDGES), ("heavy_not_growing_shrunk", 8192)])
def test_heavy_not_growing(shapes, name, heavy_edges):
    V, src, dst, source, levels, records = shapes[name]
    assert all(r.direction == R.TOP_DOWN for r in records)
    factor = R.do_factor(V, len(src))
    visited, heavy = 0, 0
    for r in records:
        visited += r.F
        if r.M > heavy_edges:
            heavy += 1
            assert r.M >= ((V - visited) * factor + V) // R.ALPHA, "only `not growing` keeps this level top-down"
    assert heavy >= 5


def test_late_from_start(shapes):
    V, src, dst, source, levels, records = shapes["late_from_start"]
    assert V == 32771
    nz = R.in_nz_rows(V, dst)
    assert nz + 1 <= V // 64                                    # late() of the driver holds whatever has been visited
    bu = [r for r in records if r.direction == R.BOTTOM_UP]
    assert len(bu) == 1 and bu[0].found > 0
    assert records[0].direction == R.TOP_DOWN and records[-1].direction == R.TOP_DOWN


def test_deep_path(shapes):
    V, src, dst, source, levels, records = shapes["deep_path"]
    assert len(records) == 3000 and all(r.F == 1 and r.direction == R.TOP_DOWN for r in records)
    assert int((levels < 0).sum()) == 500


def test_boundary_shapes_sit_on_the_boundaries(shapes):
    """the graph forms of test_bottom_up_boundary / test_top_down_boundary: one entry or one vertex decides the direction of a level"""
    def visited_at(records, k):
        return sum(r.F for r in records[:k + 1])

    V, src, _, _, _, at = shapes["bottom_up_at_threshold"]
    _, src2, _, _, _, below = shapes["bottom_up_below_threshold"]
    assert R.do_factor(V, len(src)) == R.do_factor(V, len(src2)) == 1
    threshold = (V - visited_at(at, 1) + V) // R.ALPHA
    assert at[1].F == below[1].F > at[0].F and visited_at(at, 1) == visited_at(below, 1)
    assert at[1].M == threshold and at[1].direction == R.BOTTOM_UP
    assert below[1].M == threshold - 1 and below[1].direction == R.TOP_DOWN
    assert (V - visited_at(at, 1) + V) // (R.ALPHA + 1) < threshold - 1 and R.expected(at) != R.expected(below)

    V, _, _, _, _, at = shapes["top_down_at_threshold"]
    _, _, _, _, _, below = shapes["top_down_below_threshold"]
    assert at[1].direction == below[1].direction == R.BOTTOM_UP
    assert at[2].F == (V - visited_at(at, 2) + V) // R.BETA and at[2].F < at[1].F and at[2].direction == R.BOTTOM_UP
    assert below[2].F == (V - visited_at(below, 2) + V) // R.BETA - 1 and below[2].direction == R.TOP_DOWN

    _, _, _, _, _, eq = shapes["equal_frontiers"]
    assert R.directions(eq) == "B2 t2" and eq[2].F == eq[1].F and eq[2].found > 0


def test_endings_union_ends_in_every_way():
    V, src, dst, sources = R.endings_union()
    assert V % 64 != 0
    small_m = min(8192, V // 15 - 1)                          # the list kernel's edge bound in direction-optimising mode
    rec = {name: R.schedule(V, src, dst, s)[1] for name, s in sources.items()}
    r = rec["list_kernel_finishes"]
    assert all(x.F <= SMALL_F and x.M <= small_m and x.direction == R.TOP_DOWN for x in r)
    r = rec["bitmap_expand_finds_nothing"]
    assert r[-2].direction == R.BOTTOM_UP and r[-1].direction == R.TOP_DOWN and r[-1].found == 0 and r[-1].M > 0
    r = rec["empty_count_after_top_down"]
    assert all(x.direction == R.TOP_DOWN for x in r) and r[-1].found == 0 and small_m < r[-1].M <= TD_EMIT_EDGES
    r = rec["bottom_up_finds_nothing"]
    assert all(x.direction == R.BOTTOM_UP for x in r) and r[-1].found == 0
    r = rec["source_without_entries"]
    assert len(r) == 1 and r[0].M == 0
    # ... and what the last top-down level that counts its discoveries leaves behind would turn that source's empty next level bottom-up
    left = rec["bitmap_expand_finds_nothing"][3]
    assert left.direction == R.BOTTOM_UP and R.turn_bottom_up(left.F, left.M, 1, 1 + left.F, V, R.do_factor(V, len(src)))
