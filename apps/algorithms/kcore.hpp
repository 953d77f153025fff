// k-core decomposition: the fused HIP path (vgl_hip_kcore_run, the contract of include/vgl_hip.h) and a sequential host restatement of that contract
// for -check (Batagelj-Zaversnik bucket peel, O(V + E')).  The reference has no k-core.
#pragma once
#include <algorithm>
#include <vector>

struct KCore {
    // core: device int32[V] in the graph's own numbering.  Prepare (the symmetric simple CSR) stays outside the timing.
    static double hip_fused(VGL_Graph &graph, VerticesArray<int> &core, int k_limit, vgl_hip_kcore_stats *out = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        Timer prep;
        prep.start();
        VGL_HIP_CALL(vgl_hip_kcore_prepare(c, graph.get_handle()));
        prep.end();
        vgl_hip_kcore_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_kcore_run(c, graph.get_handle(), k_limit, core.get_ptr(), nullptr, &st));
        tm.end();
        std::cout << "KCORE: degeneracy " << st.degeneracy << ", " << st.rounds << " rounds, " << st.sub_rounds << " sub-rounds, " << st.undirected_edges
                  << " undirected edges, max degree " << st.max_degree << ", " << tm.get_time() * 1000.0 << " ms, prepare " << prep.get_time() * 1000.0 << " ms, "
                  << st.edges_examined << " entries examined, " << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s of the bytes model" << std::endl;
        if (out) *out = st;
        performance_stats.print_algorithm_performance_stats("KCORE (fused)", tm.get_time(), st.edges_examined);
        return performance_stats.get_algorithm_performance(tm.get_time(), st.edges_examined);
    }

    // launches per timing slot of one more (untimed) run with the event brackets on
    static void print_launches(VGL_Graph &graph, VerticesArray<int> &core, int k_limit)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        VGL_HIP_CALL(vgl_hip_kcore_run(c, graph.get_handle(), k_limit, core.get_ptr(), nullptr, nullptr));
        int64_t total = 0;
        std::cout << "KCORE launches:";
        for (const char *name : {"kcore_scan", "kcore_short", "kcore_wave", "kcore_wg", "kcore_small", "kcore_publish"}) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    // The simple undirected graph of the contract as a CSR: both directions of every stored entry, loops dropped, duplicates dropped with a
    // last-seen mark per row (no sort): O(V + E).
    static void simple_graph(const HostCSR &g, std::vector<long long> &rowptr, std::vector<int> &adj)
    {
        const size_t V = (size_t)g.V;
        rowptr.assign(V + 1, 0);
        for (size_t u = 0; u < V; u++)
            for (long long p = g.rowptr[u]; p < g.rowptr[u + 1]; p++) {
                const size_t v = (size_t)g.adj[(size_t)p];
                if (v != u) { rowptr[u + 1]++; rowptr[v + 1]++; }
            }
        for (size_t v = 0; v < V; v++) rowptr[v + 1] += rowptr[v];
        adj.resize((size_t)rowptr[V]);
        std::vector<long long> fill(rowptr.begin(), rowptr.end() - 1);
        for (size_t u = 0; u < V; u++)
            for (long long p = g.rowptr[u]; p < g.rowptr[u + 1]; p++) {
                const size_t v = (size_t)g.adj[(size_t)p];
                if (v != u) { adj[(size_t)fill[u]++] = (int)v; adj[(size_t)fill[v]++] = (int)u; }
            }
        std::vector<int> mark(V, -1);
        long long w = 0;                                          // compaction in place: the write position never passes the read position
        for (size_t u = 0; u < V; u++) {
            const long long lo = rowptr[u], hi = rowptr[u + 1];
            rowptr[u] = w;
            for (long long p = lo; p < hi; p++) {
                const int v = adj[(size_t)p];
                if (mark[(size_t)v] != (int)u) { mark[(size_t)v] = (int)u; adj[(size_t)w++] = v; }
            }
        }
        rowptr[V] = w;
        adj.resize((size_t)w);
    }

    // Batagelj-Zaversnik: vertices bucket-sorted by degree, taken in that order; a neighbour of larger degree moves one bucket down
    static std::vector<int> seq_core_numbers(const std::vector<long long> &rowptr, const std::vector<int> &adj, int k_limit)
    {
        const size_t V = rowptr.size() - 1;
        std::vector<int> deg(V), vert(V), pos(V);
        int md = 0;
        for (size_t v = 0; v < V; v++) { deg[v] = (int)(rowptr[v + 1] - rowptr[v]); md = std::max(md, deg[v]); }
        std::vector<int> bin((size_t)md + 2, 0);
        for (size_t v = 0; v < V; v++) bin[(size_t)deg[v] + 1]++;
        for (int d = 0; d <= md; d++) bin[(size_t)d + 1] += bin[(size_t)d];          // bin[d] = first position of degree d
        {
            std::vector<int> next(bin.begin(), bin.end() - 1);
            for (size_t v = 0; v < V; v++) { pos[v] = next[(size_t)deg[v]]++; vert[(size_t)pos[v]] = (int)v; }
        }
        for (size_t i = 0; i < V; i++) {
            const int v = vert[i];
            for (long long p = rowptr[(size_t)v]; p < rowptr[(size_t)v + 1]; p++) {
                const int u = adj[(size_t)p];
                if (deg[(size_t)u] > deg[(size_t)v]) {
                    const int du = deg[(size_t)u], pu = pos[(size_t)u], pw = bin[(size_t)du], w = vert[(size_t)pw];
                    if (u != w) { pos[(size_t)u] = pw; vert[(size_t)pu] = w; pos[(size_t)w] = pu; vert[(size_t)pw] = u; }
                    bin[(size_t)du]++;
                    deg[(size_t)u]--;
                }
            }
        }
        if (k_limit > 0)
            for (size_t v = 0; v < V; v++) deg[v] = std::min(deg[v], k_limit);
        return deg;                                               // what is left of a vertex's degree when it is taken is its core number
    }
};
