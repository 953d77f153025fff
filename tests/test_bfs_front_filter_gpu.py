"""The folded-frontier filter of the bottom-up BFS step (VGL_BFS_FILTER_F: -1 / unset = default bound on the frontier size, 0 = never, a very
large value = every bottom-up level).  On a level whose frontier has at most that many vertices the fused traversal folds the frontier bitmap onto
2^17 bits (vgl_k_front_fold, timed as `bfs_front_fold`) and probes with vgl_k_bu_probe_filtered / vgl_k_bu_probe_wide_filtered, which ask an LDS
copy of the fold before they load a frontier word.  The filter has no false negatives, so on every graph below the levels are those of
oracle.bfs_top_down and the WHOLE statistics record (the STATS keys of tests/test_bfs_packed_heads_gpu.py, `bu_edges` = the probes of a sequential
scan included) equals that of the same traversal with VGL_BFS_FILTER_F=0.

Whether a source turns bottom-up, and with what frontier, is worked out on the CPU from the oracle's levels with that file's `turns_bottom_up`
rule and asserted before anything runs on the GPU; that the filtered kernel did run is read off the launch count of `bfs_front_fold` (at least one
where the rule's frontier is small, none with VGL_BFS_FILTER_F=0)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bfs_packed_heads_gpu import ALPHA, STATS, heads, host_csr, turns_bottom_up  # noqa: E402

pytestmark = pytest.mark.gpu

FOLD_WORDS = 2048
FOLD_BITS = FOLD_WORDS * 64          # 2^17
DEFAULT_F = 65536
EVERY = str(1 << 40)
SETTINGS = ("0", None, EVERY)        # never, the default rule, every bottom-up level


class filter_f:
    """VGL_BFS_FILTER_F for the traversals inside the block (read per traversal)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("VGL_BFS_FILTER_F")
        if self.value is None:
            os.environ.pop("VGL_BFS_FILTER_F", None)
        else:
            os.environ["VGL_BFS_FILTER_F"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("VGL_BFS_FILTER_F", None)
        else:
            os.environ["VGL_BFS_FILTER_F"] = self.old


def first_bottom_up_frontier(rowptr, levels):
    """size of the frontier of the first level that the switch rule (turns_bottom_up of test_bfs_packed_heads_gpu.py) turns bottom-up, or None"""
    V = len(rowptr) - 1
    E = int(rowptr[-1])
    factor = max(E // V // 2, 1)
    deg = np.diff(rowptr)
    prev_f, visited = 0, 0
    for lv in range(int(levels.max()) + 1):
        members = levels == lv
        f, m = int(members.sum()), int(deg[members].sum())
        visited += f
        if f > prev_f and m >= ((V - visited) * factor + V) // ALPHA:
            return f
        prev_f = f
    return None


def run_settings(ctx, g, source, ref, small_first):
    """the traversal from `source` under the three settings: levels of the oracle, one statistics record, and the fold launched when it must be"""
    from vectorgraphlibrary_amd import api
    records = {}
    for setting in SETTINGS:
        with filter_f(setting):
            ctx.timing(True)
            lv, st = api.bfs(g, source, api.BFS_DIRECTION_OPT, raw=True)
            folds = ctx.timing_get("bfs_front_fold")[0]
            ctx.timing(False)
        assert (lv.cpu().numpy() == ref).all(), (setting, source)
        assert st["bu_steps"] > 0, (setting, source)
        records[setting] = {k: st[k] for k in STATS}
        if setting == "0":
            assert folds == 0, source
        elif setting == EVERY:
            assert folds == st["bu_steps"], source
        elif small_first:
            assert 1 <= folds <= st["bu_steps"], source
    assert records[None] == records["0"], source
    assert records[EVERY] == records["0"], source
    return records["0"]


# ---- the fold on its own ----
def numpy_fold(front, words):
    padded = np.zeros(((words + FOLD_WORDS - 1) // FOLD_WORDS) * FOLD_WORDS, np.uint64)
    padded[:words] = front[:words]
    return np.bitwise_or.reduce(padded.reshape(-1, FOLD_WORDS), axis=0)


@pytest.mark.parametrize("words", [1, 2047, 2048, 2049, 4097 + 3])
def test_fold_alone(ctx, words):
    rng = np.random.default_rng(words)
    sparse = np.zeros(words, np.uint64)
    hits = rng.integers(0, words, max(1, words // 16))
    sparse[hits] |= np.uint64(1) << rng.integers(0, 64, len(hits)).astype(np.uint64)
    last = np.zeros(words, np.uint64)
    last[words - 1] = np.uint64(1) << np.uint64(63)
    dense = rng.integers(0, 1 << 63, words).astype(np.uint64)
    for name, pattern in (("sparse", sparse), ("zero", np.zeros(words, np.uint64)), ("last word", last), ("dense", dense)):
        buf = np.full(words + 3 * FOLD_WORDS, ~np.uint64(0))          # what lies past `words` must count as 0
        buf[:words] = pattern
        front = torch.from_numpy(buf.view(np.int64)).to(ctx.device)
        fold = ctx.bfs_front_fold(front, words).cpu().numpy().view(np.uint64)
        assert fold.shape == (FOLD_WORDS,)
        assert (fold == numpy_fold(pattern, words)).all(), (name, words)


# ---- the hand-built graph: aliases of the frontier in the filter, deferred rows, the last bitmap word ----
HV = (1 << 18) + 70                  # neither a multiple of 64 nor of 2^17
H_SRC = 5000
H_LOW = [h for h in range(3, 603, 3) if h != 69]        # 199 hubs at low ids (69 + 2^18 is the last vertex, a hub of its own below)
H_BIG = 200000                       # a hub at a large id: the member that only the deferred scan of a long row reaches
H_LAST = HV - 1                      # a hub in the last (partial) word of the frontier bitmap
BULK0, BULK_PER_HUB = 10000, 200
ROW0 = 60000


def hand_graph():
    """Level 1 = {H_SRC}, level 2 = the hubs (H_LOW, H_BIG, H_LAST), whose 40 000 out-edges turn the level bottom-up on a frontier of 201.
    Non-members the candidates see: `fillers` (low ids without incoming edges: their filter bit is clear) and `aliases` h + 2^17, h + 2^18 and
    H_BIG - 2^17 (the filter bit of a hub, but not in the frontier).  The alias h + 2^17 of an EVEN hub h is a child of h (level 3), every other
    alias is never reached.  Returns src, dst and {row: expected level} (the source is level 1)."""
    assert HV % 64 != 0 and HV % FOLD_BITS != 0
    a1 = {h: h + FOLD_BITS for h in H_LOW}
    a2 = {h: h + 2 * FOLD_BITS for h in H_LOW if h + 2 * FOLD_BITS < HV}
    big_alias = H_BIG - FOLD_BITS
    assert len(a2) >= 20 and H_LAST not in a2.values() and big_alias not in H_LOW
    fillers = [u for u in range(1, 600) if u % 3 != 0] + [69]
    dead = [a1[h] for h in H_LOW if h % 2] + sorted(a2.values()) + [big_alias]      # aliases that are never reached
    live = [a1[h] for h in H_LOW if h % 2 == 0]                                      # aliases reached at level 3
    src, dst, want = [], [], {}

    def row(t, ins, level):
        assert len(set(ins)) == len(ins) and t not in want
        for u in ins:
            src.append(u)
            dst.append(t)
        want[t] = level

    for h in H_LOW + [H_BIG, H_LAST]:
        src.append(H_SRC)
        dst.append(h)
    for i, h in enumerate(H_LOW):
        for j in range(BULK_PER_HUB):
            src.append(h)
            dst.append(BULK0 + i * BULK_PER_HUB + j)
        if h % 2 == 0:
            src.append(h)
            dst.append(a1[h])
    t = ROW0
    # only aliases: stay undiscovered on the bottom-up level, level 4 through a live alias, never through dead ones
    for h in H_LOW[:60]:
        ins = [a1[h]] + ([a2[h]] if h in a2 else [])
        row(t, ins, 4 if h % 2 == 0 else -1)
        t += 1
    for k in range(1, 9):
        row(t, dead[10:10 + k], -1)
        row(t + 1, dead[30:30 + k - 1] + [live[k]], 4)
        t += 2
    # aliases and fillers mixed with ONE true member at every position of the eight head entries
    low_fill = [u for u in fillers if u < 300]
    for k in range(1, 9):
        row(t, low_fill[:k - 1] + [300] + live[20:20 + (8 - k) // 2] + dead[50:50 + (8 - k) - (8 - k) // 2], 3)
        t += 1
    row(t, [a1[3], a1[6], a2[3], H_LAST], 3)                                         # the member of the last bitmap word, behind aliases
    row(t + 1, dead[60:67] + [H_LAST], 3)
    row(t + 2, [a2[h] for h in sorted(a2)[:3]] + [H_BIG], 3)
    t += 3
    # deferred rows: more than eight in-neighbours, the eight smallest are non-members, the single member is found by the deferred scan
    row(t, fillers[:4] + dead[70:75] + [H_BIG], 3)
    row(t + 1, fillers[4:44] + dead[80:90] + [H_BIG], 3)                              # 51 in-neighbours: several rounds of the scan
    row(t + 2, fillers[50:54] + dead[0:3] + sorted(a2.values())[:4] + [H_LAST], 3)
    row(t + 3, fillers[60:65] + dead[90:96], -1)                                      # no member at all, dead aliases only
    row(t + 4, fillers[70:75] + dead[96:100] + [live[5]], 4)                          # no member, but a live alias: one level later
    row(t + 5, [big_alias] + fillers[80:88], -1)
    t += 6
    # candidates in the last partial 64-row group
    base = 1 << 18
    row(base + 1, [H_LAST], 3)
    row(base + 2, [a1[9]], -1)
    row(base + 4, [3], 3)
    row(base + 67, [H_BIG], 3)
    row(base + 5, fillers[100:105] + dead[40:44] + [H_BIG], 3)                        # deferred as well
    assert base + 67 < HV - 1
    for r, ins_n in ((t - 6, 10), (t - 5, 51), (t - 4, 12)):
        assert dst.count(r) == ins_n
    return np.array(src, np.int32), np.array(dst, np.int32), want


def test_hand_built_aliases_deferred_rows_and_last_word(ctx, oracle):
    from vectorgraphlibrary_amd import api
    src_np, dst_np, want = hand_graph()
    assert src_np.max() < HV and dst_np.max() < HV
    src, dst = torch.from_numpy(src_np).to(ctx.device), torch.from_numpy(dst_np).to(ctx.device)
    assert {3, 4, -1} == set(want.values())
    for form in ("wide", "packed"):
        with heads(form):
            g = api.Graph.from_coo(ctx, HV, src, dst)
        assert g.info()["bfs_heads"] == form
        rowptr, adj = host_csr(g)
        ref = oracle.bfs_top_down(rowptr, adj, H_SRC)[0]
        assert turns_bottom_up(rowptr, ref), "the hubs do not turn the traversal bottom-up: the probe kernel would not run"
        assert first_bottom_up_frontier(rowptr, ref) == len(H_LOW) + 2
        for t, level in want.items():
            assert ref[t] == level, (t, level, int(ref[t]))
        assert ref[H_LAST] == 2 and ref[H_BIG] == 2 and (ref[BULK0:BULK0 + len(H_LOW) * BULK_PER_HUB] == 3).all()
        st = run_settings(ctx, g, H_SRC, ref, small_first=True)
        assert st["bu_found"] >= len(H_LOW) * BULK_PER_HUB
        g.close()


# ---- RMAT: both head forms, the three settings ----
R_SCALE, R_EF, R_SEED, R_SOURCES = 18, 16, 11, 6


@pytest.fixture(scope="module")
def rmat_case(ctx, oracle):
    from vectorgraphlibrary_amd import api
    V = 1 << R_SCALE
    src, dst = ctx.gen_rmat(R_SCALE, R_EF, R_SEED)
    graphs = {}
    for form in ("wide", "packed"):
        with heads(form):
            graphs[form] = api.Graph.from_coo(ctx, V, src, dst, renumber="total")
    rowptr, adj = host_csr(graphs["wide"])
    out_deg = np.diff(rowptr)
    rng = np.random.default_rng(R_SEED)
    sources = [int(s) for s in rng.choice(np.nonzero(out_deg > 0)[0], R_SOURCES, replace=False)]
    refs = {s: oracle.bfs_top_down(rowptr, adj, s)[0] for s in sources}
    for r in refs.values():
        r.setflags(write=False)                 # computed once, shared by both forms
    yield graphs, rowptr, sources, refs
    for g in graphs.values():
        g.close()


@pytest.mark.parametrize("form", ["wide", "packed"])
def test_rmat18_three_settings_agree(ctx, rmat_case, form):
    graphs, rowptr, sources, refs = rmat_case
    g = graphs[form]
    assert g.info()["bfs_heads"] == form
    first = {s: first_bottom_up_frontier(rowptr, refs[s]) for s in sources}
    for s in sources:
        assert turns_bottom_up(rowptr, refs[s]) and first[s] is not None, ("source never turns bottom-up: the probe kernel would not run", s)
    assert any(f <= DEFAULT_F for f in first.values()), "no source meets the default rule: the filtered kernel would not run under it"
    for s in sources:
        run_settings(ctx, g, s, refs[s], small_first=first[s] <= DEFAULT_F)
