// Triangle counting (`tri`; tc.hpp is transitive closure): the fused HIP path (vgl_hip_tri_run, the contract of include/vgl_hip.h) and a sequential
// host restatement of that contract for -check.  The reference has no triangle counting.
#pragma once
#include <algorithm>
#include <vector>

struct TriangleCount {
    // per_vertex: device int64[V] in the graph's own numbering, or nullptr for the count alone.  Prepare (the oriented CSR) stays outside the timing.
    static double hip_fused(VGL_Graph &graph, long long *d_per_vertex, long long *triangles, vgl_hip_tri_stats *out = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        Timer prep;
        prep.start();
        VGL_HIP_CALL(vgl_hip_tri_prepare(c, graph.get_handle()));
        prep.end();
        vgl_hip_tri_stats st;
        int64_t t = 0;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_tri_run(c, graph.get_handle(), &t, (int64_t *)d_per_vertex, nullptr, &st));
        tm.end();
        std::cout << "TRI: " << t << " triangles, " << st.undirected_edges << " undirected edges, " << tm.get_time() * 1000.0 << " ms ("
                  << (d_per_vertex ? "count + per-vertex" : "count only") << "), prepare " << prep.get_time() * 1000.0 << " ms, rows light / table / huge "
                  << st.rows_light << " / " << st.rows_table << " / " << st.rows_huge << ", max oriented degree " << st.max_oriented_degree << ", "
                  << st.elements_examined << " elements examined, " << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s of the bytes model" << std::endl;
        if (triangles) *triangles = t;
        if (out) *out = st;
        performance_stats.print_algorithm_performance_stats("TRI (fused)", tm.get_time(), st.elements_examined);
        return performance_stats.get_algorithm_performance(tm.get_time(), st.elements_examined);
    }

    // the contract restated sequentially: symmetrise, drop loops and duplicates, orient by (degree, id), sorted-merge intersection per oriented edge
    static long long seq_triangle_count(const HostCSR &g, std::vector<long long> &per_vertex)
    {
        const size_t V = (size_t)g.V;
        std::vector<std::vector<int>> nb(V);
        for (size_t u = 0; u < V; u++)
            for (long long p = g.rowptr[u]; p < g.rowptr[u + 1]; p++) {
                const int v = g.adj[(size_t)p];
                if ((size_t)v != u) { nb[u].push_back(v); nb[(size_t)v].push_back((int)u); }
            }
        for (auto &l : nb) { std::sort(l.begin(), l.end()); l.erase(std::unique(l.begin(), l.end()), l.end()); }
        auto below = [&](int u, int v) { return nb[(size_t)u].size() != nb[(size_t)v].size() ? nb[(size_t)u].size() < nb[(size_t)v].size() : u < v; };
        std::vector<std::vector<int>> up(V);
        for (size_t u = 0; u < V; u++)
            for (int v : nb[u]) if (below((int)u, v)) up[u].push_back(v);          // ascending by id, as nb is
        per_vertex.assign(V, 0);
        long long total = 0;
        for (size_t a = 0; a < V; a++)
            for (int b : up[a]) {
                const std::vector<int> &x = up[a], &y = up[(size_t)b];
                for (size_t i = 0, j = 0; i < x.size() && j < y.size();) {
                    if (x[i] < y[j]) i++;
                    else if (x[i] > y[j]) j++;
                    else { total++; per_vertex[a]++; per_vertex[(size_t)b]++; per_vertex[(size_t)x[i]]++; i++; j++; }
                }
            }
        return total;
    }
};
#define TRI TriangleCount
