// primitives_contract: self-check of the operator primitives of GraphAbstractionsHIP one by one -- compute, reduce, generate_new_frontier, advance
// (static tiles, sparse plan, sequential rows), VGL_SRC_ID_ADD and ParallelPrimitives::copy_if_indexes -- against host evaluations over HostCSR and
// host copies of the inputs, in both directions, on every frontier kind the storage format produces.  The applications check end results; a
// primitive can be wrong without moving one (an edge visited twice while another is missed keeps every total).  Families:
//   A compute   every active vertex called exactly once, no inactive one, connections_count = the degree of the direction
//   B reduce    SUM / MAX of int, float and double operators whose f64 sum is exact in any order, MAX = max(0, values), empty frontier = 0,
//               REDUCE_AVG refused, one inexact double sum: the same bits twice and within (n - 1) * 2^-53 * sum|x| of the long double sum
//   C generate_new_frontier   size, neighbour count (degrees of the generation direction), sparsity type, ascending ids, DENSE flags, and the
//               predicate is never given an id outside [0, V); then A, B, D, E, F on the generated frontier (the plan the generation leaves behind)
//   D advance   visits[edge] == 1 on the edges of active rows and 0 elsewhere, dst_id and local_edge_pos per edge, pre / post once per active vertex
//   E sequential rows   as D, plus adjacency order (a cursor without atomics) and a float chain with the bits of the host's loop
//   F VGL_SRC_ID_ADD    int / float / double slots from a tile advance, values exact in any order, equal to the host per vertex
//   G copy_if_indexes   sizes 0, 1, 255, 256, 257, 256 * 4096 + 1; conditions none, all, i % 3 == 0, only the last index
// One frontier object per direction is regenerated through all predicates in turn (every 7th, all, none, every 7th again, ...): stale ids, flags
// or plans of the frontier before would show.  Prints one line per failed check, the coverage facts (which branch the input reached), then
// `error count: N`; exits 1 if N > 0.
#include "common.hpp"
#include <sstream>

namespace {

int g_errors = 0;
// coverage facts: what of the kernels' branch conditions this input reached (recomputed on the host from the CSR and the frontier's ids)
long long g_unstaged_tiles = 0, g_long_rows = 0, g_multi_chunk_blocks = 0, g_combined_waves = 0, g_mixed_waves = 0;
constexpr int ROWS_CHUNK = 4096;       // vgl_k_advance_rows streams the adjacency of 256 rows through LDS in chunks of this many entries

void fail(const std::string &where, const std::string &what)
{
    std::cout << "FAILED " << where << ": " << what << std::endl;
    g_errors++;
}

template <class T>
struct Dev {                           // a device array with host transfers; one allocation for the whole run (vgl_hip_free synchronises)
    T *p = nullptr; size_t n;
    explicit Dev(size_t count) : n(count) { MemoryAPI::allocate_device_array(&p, std::max<size_t>(n, 1)); }
    ~Dev() { MemoryAPI::free_device_array(p); }
    Dev(const Dev &) = delete;
    void fill_bytes(int byte) { VGL_HIP_CALL(vgl_hip_memset(VGL_RUNTIME::ctx(), p, byte, sizeof(T) * n)); }
    void zero() { fill_bytes(0); }
    void put(const std::vector<T> &h) { VGL_HIP_CALL(vgl_hip_memcpy_h2d(VGL_RUNTIME::ctx(), p, h.data(), sizeof(T) * std::min(n, h.size()))); }
    std::vector<T> get(size_t count) const
    {
        std::vector<T> h(std::min(count, n));
        VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), p, sizeof(T) * h.size()));
        return h;
    }
    std::vector<T> get() const { return get(n); }
};

// first index where got differs from want(i), as text; empty when all agree
template <class T, class Want>
std::string first_mismatch(const std::vector<T> &got, Want &&want)
{
    size_t bad = 0, first = 0;
    for (size_t i = 0; i < got.size(); i++)
        if (!(got[i] == want(i)) && bad++ == 0) first = i;
    if (!bad) return "";
    std::ostringstream s;
    s << bad << " of " << got.size() << " differ, first at " << first << ": " << got[first] << " vs " << want(first);
    return s.str();
}

// operands of the reductions and of VGL_SRC_ID_ADD: integers, and multiples of 2^-10 small enough that every partial sum is exact in f32 / f64
__host__ __device__ inline int op_int(int v) { return v % 1000 - 300; }
__host__ __device__ inline float op_flt(int v) { return (float)(v % 2048 - 1024) * (1.0f / 1024.0f); }
__host__ __device__ inline double op_dbl(int v) { return (double)((long long)v * 37 % 4096 - 2000) * (1.0 / 1024.0); }
__host__ __device__ inline int op_neg_int(int v) { return -(v % 5) - 1; }
__host__ __device__ inline float op_neg_flt(int v) { return -1.5f - (float)(v % 3); }
__host__ __device__ inline int add_int(int v) { return v % 7 - 3; }
__host__ __device__ inline float add_flt(int v) { return (float)(v % 64 - 32) * (1.0f / 1024.0f); }
__host__ __device__ inline double add_dbl(int v) { return (double)(v % 4096 - 2048) * (1.0 / 1024.0); }

enum BadSlot { BAD_SRC = 0, BAD_EDGE = 1, BAD_DST = 2, BAD_LOCAL = 3, BAD_INDEX = 4, BAD_SLOTS = 8 };
const char *const bad_names[BAD_SLOTS] = {"src_id outside [0, V)", "global_edge_pos outside the direction's edges", "dst_id != adjacency entry",
                                          "local_edge_pos != position in the row", "index outside [0, size)", "", "", ""};

struct State {
    VGL_Graph &graph; VGL_GRAPH_ABSTRACTIONS &api; VGL_FRONTIER &frontier; TraversalDirection dir; const HostCSR &h;
    int V; long long E, shift; vgl_csr_view view;
    std::vector<int> act; std::vector<char> on; std::string tag;          // the frontier as the host expects it: ascending ids, membership
    std::vector<float> h_val;
    Dev<int> calls, seen, pre_calls, post_calls, post_deg, cursor, post_cur, marks, sum_i, bad, lohi, visits, order;
    Dev<float> val, acc, sum_f;
    Dev<double> sum_d;
    State(VGL_Graph &g, VGL_GRAPH_ABSTRACTIONS &a, VGL_FRONTIER &f, TraversalDirection d, const HostCSR &host)
        : graph(g), api(a), frontier(f), dir(d), h(host), V(g.get_vertices_count()), E(g.get_edges_count()), shift(d == GATHER ? g.get_edges_count() : 0),
          view(g.get_direction_view(d)), on((size_t)V, 0), h_val((size_t)V), calls(V), seen(V), pre_calls(V), post_calls(V), post_deg(V), cursor(V), post_cur(V),
          marks(V), sum_i(V), bad(BAD_SLOTS), lohi(2), visits((size_t)E), order((size_t)E), val(V), acc(V), sum_f(V), sum_d(V)
    {
        for (int v = 0; v < V; v++) h_val[(size_t)v] = 1.0f / (float)(1 + v % 977) + (float)(v % 13) * 0.37f;
        val.put(h_val);
        bad.zero();
    }
    long long deg(int v) const { return h.rowptr[(size_t)v + 1] - h.rowptr[(size_t)v]; }
    std::string where(const char *family) const { return std::string(family) + " [" + tag + "]"; }
    void check_bad(const char *family)
    {
        const std::vector<int> b = bad.get();
        for (int i = 0; i < BAD_SLOTS; i++)
            if (b[(size_t)i]) { fail(where(family), std::string(bad_names[i]) + " in " + std::to_string(b[(size_t)i]) + " calls"); }
        bad.zero();
    }
    template <class EdgeOp, class PreOp, class PostOp>
    void advance(EdgeOp &&edge, PreOp &&pre, PostOp &&post)
    {
        if (dir == SCATTER) api.scatter(graph, frontier, edge, pre, post, edge, pre, post);
        else api.gather(graph, frontier, edge, pre, post, edge, pre, post);
        VGL_RUNTIME::sync();
    }
};

const char *type_name(FrontierSparsityType t) { return t == ALL_ACTIVE_FRONTIER ? "ALL_ACTIVE" : t == DENSE_FRONTIER ? "DENSE" : "SPARSE"; }

// ---- A: compute ----
void check_compute(State &s)
{
    const int V = s.V;
    int *calls = s.calls.p, *seen = s.seen.p, *bad = s.bad.p;
    s.calls.zero(); s.seen.fill_bytes(0xFF);
    auto op = [calls, seen, bad, V] __VGL_COMPUTE_ARGS__ {
        if ((unsigned)src_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        atomicAdd(&calls[src_id], 1);
        seen[src_id] = connections_count;
    };
    s.api.compute(s.graph, s.frontier, op);
    VGL_RUNTIME::sync();
    s.check_bad("A compute");
    std::string m = first_mismatch(s.calls.get(), [&](size_t v) { return (int)s.on[v]; });
    if (!m.empty()) fail(s.where("A compute"), "calls per vertex: " + m);
    m = first_mismatch(s.seen.get(), [&](size_t v) { return s.on[v] ? (int)s.deg((int)v) : -1; });
    if (!m.empty()) fail(s.where("A compute"), "connections_count: " + m);
}

// ---- B: reduce ----
template <class T, class Op, class HostOp>
void check_reduce_pair(State &s, const char *name, Op &&op, HostOp &&host_op)
{
    long double sum = 0, mx = 0;                   // exact: the operands are integers or multiples of 2^-10 far below 2^53 ulps
    for (int v : s.act) { const long double x = (long double)host_op(v); sum += x; if (x > mx) mx = x; }
    const T got_sum = s.api.template reduce<T>(s.graph, s.frontier, op, REDUCE_SUM), got_max = s.api.template reduce<T>(s.graph, s.frontier, op, REDUCE_MAX);
    if ((long double)got_sum != sum) { std::ostringstream t; t << name << " REDUCE_SUM " << got_sum << " vs " << (double)sum; fail(s.where("B reduce"), t.str()); }
    if ((long double)got_max != mx) { std::ostringstream t; t << name << " REDUCE_MAX " << got_max << " vs " << (double)mx; fail(s.where("B reduce"), t.str()); }
}
void check_reduce(State &s)
{
    check_reduce_pair<int>(s, "int", [] __VGL_REDUCE_INT_ARGS__ { return op_int(src_id); }, [](int v) { return op_int(v); });
    check_reduce_pair<float>(s, "float", [] __VGL_REDUCE_FLT_ARGS__ { return op_flt(src_id); }, [](int v) { return op_flt(v); });
    check_reduce_pair<double>(s, "double", [] __VGL_REDUCE_DBL_ARGS__ { return op_dbl(src_id); }, [](int v) { return op_dbl(v); });
    check_reduce_pair<int>(s, "negative int", [] __VGL_REDUCE_INT_ARGS__ { return op_neg_int(src_id); }, [](int v) { return op_neg_int(v); });
    check_reduce_pair<float>(s, "negative float", [] __VGL_REDUCE_FLT_ARGS__ { return op_neg_flt(src_id); }, [](int v) { return op_neg_flt(v); });
    check_reduce_pair<int>(s, "connections_count", [] __VGL_REDUCE_INT_ARGS__ { return connections_count; }, [&](int v) { return (int)s.deg(v); });
    // the inexact sum: any summation order of n terms is within (n - 1) * 2^-53 * sum|x| of the exact sum (and the result is a double of its own)
    auto harmonic = [] __VGL_REDUCE_DBL_ARGS__ { return 1.0 / (double)(src_id + 1); };
    const double r1 = s.api.reduce<double>(s.graph, s.frontier, harmonic, REDUCE_SUM), r2 = s.api.reduce<double>(s.graph, s.frontier, harmonic, REDUCE_SUM);
    long double want = 0;                          // of the operands as the operator returns them: doubles
    for (int v : s.act) want += (long double)(1.0 / (double)(v + 1));
    const long double bound = s.act.empty() ? 0.0L : (long double)(s.act.size() - 1) * std::ldexp(1.0L, -53) * want;
    if (std::memcmp(&r1, &r2, sizeof(double)) != 0) { std::ostringstream t; t.precision(17); t << "inexact sum differs between two calls: " << r1 << " vs " << r2; fail(s.where("B reduce"), t.str()); }
    if (std::fabs((long double)r1 - want) > bound) {
        std::ostringstream t; t.precision(17);
        t << "inexact sum " << r1 << " vs " << (double)want << ": off by " << (double)std::fabs((long double)r1 - want) << ", bound " << (double)bound;
        fail(s.where("B reduce"), t.str());
    }
    bool thrown = false;
    try { s.api.reduce<int>(s.graph, s.frontier, [] __VGL_REDUCE_INT_ARGS__ { return 1; }, REDUCE_AVG); } catch (const char *) { thrown = true; }
    if (!thrown) fail(s.where("B reduce"), "REDUCE_AVG not refused");
}

// sparse tiles the kernel takes unstaged: positions p_first .. p_last of a 2048-edge tile of the frontier's edge space, p_last = the owner of the
// next tile's first edge (the last tile: of the last edge), more than VGL_ADV_STAGE of them
long long unstaged_tiles(const State &s)
{
    std::vector<long long> offs(s.act.size() + 1, 0);
    for (size_t p = 0; p < s.act.size(); p++) offs[p + 1] = offs[p] + s.deg(s.act[p]);
    const long long M = offs.back();
    auto owner = [&](long long e) { return (long long)(std::upper_bound(offs.begin(), offs.end(), e) - offs.begin()) - 1; };
    long long count = 0;
    for (long long e0 = 0; e0 < M; e0 += VGL_TILE) {
        const long long p_first = owner(e0), p_last = e0 + VGL_TILE < M ? owner(e0 + VGL_TILE) : owner(M - 1);
        if (p_last - p_first + 1 > VGL_ADV_STAGE) count++;
    }
    return count;
}

// what D and E share: visits per edge, pre / post per vertex
void check_visits(State &s, const char *family)
{
    const std::vector<int> visits = s.visits.get();
    size_t bad = 0; long long first = -1;
    for (int v = 0; v < s.V; v++)
        for (long long e = s.h.rowptr[(size_t)v]; e < s.h.rowptr[(size_t)v + 1]; e++)
            if (visits[(size_t)e] != (int)s.on[(size_t)v] && bad++ == 0) first = e;
    if (bad) fail(s.where(family), "visits per edge: " + std::to_string(bad) + " edges differ, first at CSR position " + std::to_string(first) + ": " +
                                       std::to_string(visits[(size_t)first]) + " visits");
    std::string m = first_mismatch(s.pre_calls.get(), [&](size_t v) { return (int)s.on[v]; });
    if (!m.empty()) fail(s.where(family), "pre calls per vertex: " + m);
    m = first_mismatch(s.post_calls.get(), [&](size_t v) { return (int)s.on[v]; });
    if (!m.empty()) fail(s.where(family), "post calls per vertex: " + m);
    m = first_mismatch(s.post_deg.get(), [&](size_t v) { return s.on[v] ? (int)s.deg((int)v) : -1; });
    if (!m.empty()) fail(s.where(family), "connections_count of post: " + m);
}

// ---- D: advance over static tiles (ALL_ACTIVE, DENSE) or the sparse plan ----
void check_advance(State &s)
{
    const int V = s.V; const long long E = s.E, shift = s.shift;
    const vgl_csr_view view = s.view;
    int *visits = s.visits.p, *pre_calls = s.pre_calls.p, *post_calls = s.post_calls.p, *post_deg = s.post_deg.p, *bad = s.bad.p;
    s.visits.zero(); s.pre_calls.zero(); s.post_calls.zero(); s.post_deg.fill_bytes(0xFF);
    auto edge = [visits, bad, view, V, E, shift] __VGL_ADVANCE_ARGS__ {
        const long long e = global_edge_pos - shift;
        if ((unsigned)src_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        if (e < 0 || e >= E) { atomicAdd(&bad[BAD_EDGE], 1); return; }
        atomicAdd(&visits[e], 1);
        if (view.adj[e] != dst_id) atomicAdd(&bad[BAD_DST], 1);
        if (e - view.rowptr[src_id] != (long long)local_edge_pos) atomicAdd(&bad[BAD_LOCAL], 1);
    };
    auto pre = [pre_calls, bad, V] __VGL_ADVANCE_PREPROCESS_ARGS__ {
        if ((unsigned)src_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        atomicAdd(&pre_calls[src_id], 1);
    };
    auto post = [post_calls, post_deg, bad, V] __VGL_ADVANCE_POSTPROCESS_ARGS__ {
        if ((unsigned)src_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        atomicAdd(&post_calls[src_id], 1);
        post_deg[src_id] = connections_count;
    };
    s.advance(edge, pre, post);
    s.check_bad("D advance");
    check_visits(s, "D advance");
    if (s.frontier.get_sparsity_type() == SPARSE_FRONTIER) g_unstaged_tiles += unstaged_tiles(s);
}

// ---- E: sequential rows ----
void check_sequential_rows(State &s)
{
    const int V = s.V; const long long E = s.E, shift = s.shift;
    const vgl_csr_view view = s.view;
    int *visits = s.visits.p, *order = s.order.p, *cursor = s.cursor.p, *post_cur = s.post_cur.p, *pre_calls = s.pre_calls.p, *post_calls = s.post_calls.p,
        *post_deg = s.post_deg.p, *bad = s.bad.p;
    float *acc = s.acc.p; const float *val = s.val.p;
    s.visits.zero(); s.order.fill_bytes(0xFF); s.cursor.fill_bytes(0xFF); s.post_cur.fill_bytes(0xFF); s.pre_calls.zero(); s.post_calls.zero();
    s.post_deg.fill_bytes(0xFF); s.acc.fill_bytes(0xFF);
    auto pre = [cursor, acc, pre_calls, bad, V] __VGL_ADVANCE_PREPROCESS_ARGS__ {
        if ((unsigned)src_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        cursor[src_id] = 0; acc[src_id] = 0.0f;
        atomicAdd(&pre_calls[src_id], 1);
    };
    // no atomics on src-indexed state: one lane owns the row and walks it in adjacency order
    auto edge = [visits, order, cursor, acc, val, bad, view, V, E, shift] __VGL_ADVANCE_ARGS__ {
        const long long e = global_edge_pos - shift;
        if ((unsigned)src_id >= (unsigned)V || (unsigned)dst_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        if (e < 0 || e >= E) { atomicAdd(&bad[BAD_EDGE], 1); return; }
        atomicAdd(&visits[e], 1);
        if (view.adj[e] != dst_id) atomicAdd(&bad[BAD_DST], 1);
        if (e - view.rowptr[src_id] != (long long)local_edge_pos) atomicAdd(&bad[BAD_LOCAL], 1);
        order[e] = cursor[src_id]++;
        acc[src_id] += val[dst_id];
    };
    auto post = [cursor, post_cur, post_calls, post_deg, bad, V] __VGL_ADVANCE_POSTPROCESS_ARGS__ {
        if ((unsigned)src_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        post_cur[src_id] = cursor[src_id];
        atomicAdd(&post_calls[src_id], 1);
        post_deg[src_id] = connections_count;
    };
    s.api.enable_sequential_rows();
    s.advance(edge, pre, post);
    s.api.disable_sequential_rows();
    s.check_bad("E sequential rows");
    check_visits(s, "E sequential rows");
    const std::vector<int> order_h = s.order.get();
    size_t wrong = 0; long long first = -1;
    for (int v = 0; v < V; v++)
        for (long long e = s.h.rowptr[(size_t)v]; e < s.h.rowptr[(size_t)v + 1]; e++)
            if (order_h[(size_t)e] != (s.on[(size_t)v] ? (int)(e - s.h.rowptr[(size_t)v]) : -1) && wrong++ == 0) first = e;
    if (wrong) fail(s.where("E sequential rows"), "adjacency order: " + std::to_string(wrong) + " edges differ, first at CSR position " + std::to_string(first) +
                                                      ": step " + std::to_string(order_h[(size_t)first]));
    std::string m = first_mismatch(s.post_cur.get(), [&](size_t v) { return s.on[v] ? (int)s.deg((int)v) : -1; });
    if (!m.empty()) fail(s.where("E sequential rows"), "cursor seen by post: " + m);
    // the float chain: the bits of the host's sequential f32 loop over the row
    const std::vector<float> acc_h = s.acc.get();
    std::vector<int> acc_bits((size_t)V);
    std::memcpy(acc_bits.data(), acc_h.data(), sizeof(float) * (size_t)V);
    m = first_mismatch(acc_bits, [&](size_t v) {
        if (!s.on[v]) return -1;
        float a = 0.0f;
        for (long long e = s.h.rowptr[v]; e < s.h.rowptr[v + 1]; e++) a += s.h_val[(size_t)s.h.adj[(size_t)e]];
        int bits; std::memcpy(&bits, &a, sizeof(float));
        return bits;
    });
    if (!m.empty()) fail(s.where("E sequential rows"), "float chain (bit patterns): " + m);
}

// ---- F: VGL_SRC_ID_ADD ----
void check_src_id_add(State &s)
{
    const int V = s.V;
    int *sum_i = s.sum_i.p, *bad = s.bad.p; float *sum_f = s.sum_f.p; double *sum_d = s.sum_d.p;
    s.sum_i.zero(); s.sum_f.zero(); s.sum_d.zero();
    auto edge = [sum_i, sum_f, sum_d, bad, V] __VGL_ADVANCE_ARGS__ {
        if ((unsigned)src_id >= (unsigned)V) { atomicAdd(&bad[BAD_SRC], 1); return; }
        VGL_SRC_ID_ADD(sum_i[src_id], add_int(dst_id));
        VGL_SRC_ID_ADD(sum_f[src_id], add_flt(dst_id));
        VGL_SRC_ID_ADD(sum_d[src_id], add_dbl(dst_id));
    };
    if (s.dir == SCATTER) s.api.scatter(s.graph, s.frontier, edge); else s.api.gather(s.graph, s.frontier, edge);
    VGL_RUNTIME::sync();
    s.check_bad("F VGL_SRC_ID_ADD");
    std::vector<int> wi((size_t)V, 0); std::vector<float> wf((size_t)V, 0.0f); std::vector<double> wd((size_t)V, 0.0);
    for (int v : s.act)
        for (long long e = s.h.rowptr[(size_t)v]; e < s.h.rowptr[(size_t)v + 1]; e++) {
            const int d = s.h.adj[(size_t)e];
            wi[(size_t)v] += add_int(d); wf[(size_t)v] += add_flt(d); wd[(size_t)v] += add_dbl(d);
        }
    std::string m = first_mismatch(s.sum_i.get(), [&](size_t v) { return wi[v]; });
    if (!m.empty()) fail(s.where("F VGL_SRC_ID_ADD"), "int slots: " + m);
    m = first_mismatch(s.sum_f.get(), [&](size_t v) { return wf[v]; });
    if (!m.empty()) fail(s.where("F VGL_SRC_ID_ADD"), "float slots: " + m);
    m = first_mismatch(s.sum_d.get(), [&](size_t v) { return wd[v]; });
    if (!m.empty()) fail(s.where("F VGL_SRC_ID_ADD"), "double slots: " + m);
}

void check_all_families(State &s)
{
    check_compute(s);
    check_reduce(s);
    check_advance(s);
    check_sequential_rows(s);
    check_src_id_add(s);
}

// ---- C: generate_new_frontier with the predicate `want` (host) = marks (device), or connections_count > 0 ----
void generate_and_check(State &s, const std::string &name, const std::vector<char> &want, bool by_degree)
{
    const int V = s.V;
    std::vector<int> m((size_t)V);
    for (int v = 0; v < V; v++) m[(size_t)v] = by_degree ? -7 : (int)want[(size_t)v];       // (by_degree: the marks must not be looked at)
    s.marks.put(m);
    s.lohi.put(std::vector<int>{0x7FFFFFFF, -0x7FFFFFFF - 1});
    const int *marks = s.marks.p; int *lohi = s.lohi.p;
    auto pred = [marks, lohi, V, by_degree] __VGL_GNF_ARGS__ {
        atomicMin(&lohi[0], src_id); atomicMax(&lohi[1], src_id);
        if ((unsigned)src_id >= (unsigned)V) return 0;                                      // (user arrays are V long)
        return by_degree ? (connections_count > 0) : marks[src_id];
    };
    s.api.generate_new_frontier(s.graph, s.frontier, pred);
    VGL_RUNTIME::sync();
    s.act.clear();
    long long neighbours = 0;
    for (int v = 0; v < V; v++) {
        s.on[(size_t)v] = want[(size_t)v];
        if (want[(size_t)v]) { s.act.push_back(v); neighbours += s.deg(v); }
    }
    const int size = (int)s.act.size();
    const FrontierSparsityType type = s.frontier.get_sparsity_type();
    const FrontierSparsityType want_type = size == V ? ALL_ACTIVE_FRONTIER
                                           : (s.graph.get_format() == VECTOR_CSR_GRAPH && (double)size / V > 0.7) ? DENSE_FRONTIER : SPARSE_FRONTIER;
    s.tag = std::string(s.dir == SCATTER ? "scatter" : "gather") + " / " + name + " / " + type_name(type);
    const std::string w = s.where("C generate_new_frontier");
    const std::vector<int> lh = s.lohi.get();
    if (lh[0] < 0 || lh[1] >= V || lh[0] > lh[1]) fail(w, "predicate evaluated for ids " + std::to_string(lh[0]) + " .. " + std::to_string(lh[1]) + ", V = " + std::to_string(V));
    if (s.frontier.size() != size) fail(w, "size " + std::to_string(s.frontier.size()) + " vs " + std::to_string(size));
    if (s.frontier.get_neighbours_count() != neighbours) fail(w, "neighbour count " + std::to_string(s.frontier.get_neighbours_count()) + " vs " + std::to_string(neighbours));
    if (type != want_type) fail(w, std::string("sparsity type ") + type_name(type) + " vs " + type_name(want_type));
    if (type == SPARSE_FRONTIER && s.frontier.size() == size) {
        std::vector<int> ids((size_t)size);
        VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), ids.data(), s.frontier.get_ids(), sizeof(int) * ids.size()));
        const std::string d = first_mismatch(ids, [&](size_t p) { return s.act[p]; });
        if (!d.empty()) fail(w, "ids: " + d);
    }
    if (type == DENSE_FRONTIER) {
        std::vector<int> flags((size_t)V);
        VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), flags.data(), s.frontier.get_flags(), sizeof(int) * flags.size()));
        const std::string d = first_mismatch(flags, [&](size_t v) { return want[v] ? IN_FRONTIER_FLAG : NOT_IN_FRONTIER_FLAG; });
        if (!d.empty()) fail(w, "flags: " + d);
    }
    // the primitives on what the generation left behind (ids / flags, and for SCATTER the advance plan)
    if (type == want_type && s.frontier.size() == size) check_all_families(s);
    else fail(w, "the frontier is not what the predicate describes: the primitives were not run on it");
}

void check_direction(VGL_Graph &graph, TraversalDirection dir)
{
    VGL_GRAPH_ABSTRACTIONS api(graph, dir);
    VGL_FRONTIER frontier(graph, dir);
    api.change_traversal_direction(dir, frontier);
    const HostCSR h(graph, dir);
    State s(graph, api, frontier, dir, h);
    const int V = s.V;
    // static coverage facts of this direction's CSR
    std::vector<int> row_of((size_t)s.E);
    for (int v = 0; v < V; v++) {
        if (s.deg(v) > ROWS_CHUNK) g_long_rows++;
        for (long long e = h.rowptr[(size_t)v]; e < h.rowptr[(size_t)v + 1]; e++) row_of[(size_t)e] = v;
    }
    for (int r0 = 0; r0 < V; r0 += VGL_BLOCK)
        if (h.rowptr[(size_t)std::min(r0 + VGL_BLOCK, V)] - h.rowptr[(size_t)r0] > ROWS_CHUNK) g_multi_chunk_blocks++;
    for (long long e0 = 0; e0 < s.E; e0 += 64) {                  // a wavefront of a static tile: 64 consecutive CSR positions from a multiple of 64
        const long long e1 = std::min(e0 + 64, s.E) - 1;
        if (row_of[(size_t)e0] != row_of[(size_t)e1]) g_mixed_waves++;
        else if (e1 - e0 + 1 >= 8) g_combined_waves++;
    }
    // the frontier as constructed: all active (set_all_active, not a generation)
    s.tag = std::string(dir == SCATTER ? "scatter" : "gather") + " / as constructed / " + type_name(frontier.get_sparsity_type());
    for (int v = 0; v < V; v++) { s.on[(size_t)v] = 1; s.act.push_back(v); }
    if (frontier.get_sparsity_type() != ALL_ACTIVE_FRONTIER || frontier.size() != V) fail(s.where("C generate_new_frontier"), "a new frontier is not all active");
    check_all_families(s);
    // one frontier object through every predicate: sparse, all, empty, sparse again, then the rest
    const int k = std::max(1, V / 2 / VGL_TILE);
    const int b_lo = V > VGL_TILE ? k * VGL_TILE - 300 : V / 4, b_hi = V > VGL_TILE ? std::min(V, k * VGL_TILE + 500) : std::max(V / 4 + 1, 3 * V / 4);
    struct Pred { const char *name; int kind; };
    const Pred preds[] = {{"every 7th", 4}, {"all", 1}, {"none", 0}, {"every 7th again", 4}, {"all but every 11th", 5}, {"only vertex 0", 2}, {"only vertex V - 1", 3},
                          {"block across a multiple of 2048", 6}, {"connections_count > 0", 7}};
    for (const Pred &p : preds) {
        std::vector<char> want((size_t)V);
        for (int v = 0; v < V; v++)
            want[(size_t)v] = p.kind == 0 ? 0 : p.kind == 1 ? 1 : p.kind == 2 ? v == 0 : p.kind == 3 ? v == V - 1 : p.kind == 4 ? v % 7 == 0 : p.kind == 5 ? v % 11 != 0
                              : p.kind == 6 ? (v >= b_lo && v < b_hi) : s.deg(v) > 0;
        generate_and_check(s, p.name, want, p.kind == 7);
    }
}

// ---- G: ParallelPrimitives::copy_if_indexes ----
void check_copy_if()
{
    const long long sizes[] = {0, 1, 255, 256, 257, 256LL * 4096 + 1};
    const char *const cond_names[] = {"none", "all", "i % 3 == 0", "only the last index"};
    Dev<long long> out((size_t)(256LL * 4096 + 1));
    Dev<int> bad(BAD_SLOTS);
    bad.zero();
    for (const long long n : sizes)
        for (int mode = 0; mode < 4; mode++) {
            int *bad_p = bad.p;
            auto keep = [](int mode, long long i, long long n) { return mode == 0 ? false : mode == 1 ? true : mode == 2 ? i % 3 == 0 : i == n - 1; };
            auto cond = [mode, n, bad_p] __VGL_COPY_IF_INDEXES_ARGS__ {
                if (idx < 0 || idx >= n) { atomicAdd(&bad_p[BAD_INDEX], 1); return 0; }
                return mode == 0 ? 0 : mode == 1 ? 1 : mode == 2 ? (int)(idx % 3 == 0) : (int)(idx == n - 1);
            };
            out.fill_bytes(0xFF);
            const long long got = ParallelPrimitives::copy_if_indexes(cond, out.p, n);
            std::vector<long long> want;
            for (long long i = 0; i < n; i++) if (keep(mode, i, n)) want.push_back(i);
            const std::string w = "G copy_if_indexes [size " + std::to_string(n) + " / " + cond_names[mode] + "]";
            if (got != (long long)want.size()) { fail(w, "count " + std::to_string(got) + " vs " + std::to_string(want.size())); continue; }
            // one entry past the list must be untouched
            const std::vector<long long> list = out.get((size_t)std::min<long long>(got + 1, (long long)out.n));
            const std::string d = first_mismatch(list, [&](size_t p) { return p < want.size() ? want[p] : -1LL; });
            if (!d.empty()) fail(w, "indexes: " + d);
            if (bad.get()[BAD_INDEX]) { fail(w, "condition evaluated outside [0, size)"); bad.zero(); }
        }
}

}  // namespace

int main(int argc, char **argv)
{
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        {
            VGL_Graph graph(parser.format);
            prepare_graph(graph, parser);
            const int V = graph.get_vertices_count();
            std::cout << "vertices: " << V << ", edges: " << graph.get_edges_count() << ", format: " << (graph.get_format() == VECTOR_CSR_GRAPH ? "vcsr" : "csr") << std::endl;
            check_direction(graph, SCATTER);
            check_direction(graph, GATHER);
            check_copy_if();
            std::cout << "coverage: unstaged_sparse_tiles = " << g_unstaged_tiles << std::endl
                      << "coverage: rows_longer_than_chunk = " << g_long_rows << std::endl
                      << "coverage: row_blocks_over_one_chunk = " << g_multi_chunk_blocks << std::endl
                      << "coverage: combined_add_wavefronts = " << g_combined_waves << std::endl
                      << "coverage: mixed_add_wavefronts = " << g_mixed_waves << std::endl
                      << "coverage: v_mod_8_nonzero = " << (V % 8 != 0) << std::endl
                      << "coverage: v_mod_256_nonzero = " << (V % 256 != 0) << std::endl
                      << "coverage: v_mod_2048_nonzero = " << (V % 2048 != 0) << std::endl;
        }
        std::cout << "error count: " << g_errors << std::endl;
        VGL_RUNTIME::finalize_library();
        return g_errors ? 1 : 0;
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return 0;
}
