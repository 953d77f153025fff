// Label propagation (LabelPropagation, algorithms/lp/lp.h:15-30): the fused HIP path (vgl_hip_lp_run, the AlwaysActive contract of
// include/vgl_hip.h) and a host restatement of that contract for -check.
#pragma once
#include <algorithm>
#include <vector>

#define LP_DEFAULT_MAX_ITERATIONS 20      // lp.h:10

struct LabelPropagation {
    // labels start from the ORIGINAL vertex ids (the graph's stored -> original table when it is renumbered), so the answer does not
    // depend on the storage format.  mode: VGL_LP_ALL_ACTIVE / VGL_LP_FRONTIER / VGL_LP_AUTO (same labels).
    static double hip_fused(VGL_Graph &graph, VerticesArray<int> &labels, int max_iterations, int mode = VGL_LP_AUTO, vgl_hip_lp_stats *out = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const int32_t *init = graph.is_renumbered() ? graph.get_backward_conversion() : nullptr;
        VGL_HIP_CALL(vgl_hip_lp_prepare(c, graph.get_handle(), 0));      // degree classes: once per graph, outside the timing
        std::vector<int64_t> history((size_t)std::max(1, max_iterations));
        vgl_hip_lp_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_lp_run(c, graph.get_handle(), 0, mode, 0, max_iterations, init, labels.get_ptr(), history.data(), &st));
        tm.end();
        std::cout << "LP: " << st.iterations << " iterations (" << st.frontier_steps << " on a frontier), converged " << st.converged << ", "
                  << (st.iterations ? tm.get_time() * 1000.0 / st.iterations : 0.0) << " ms per iteration, changed:";
        for (int i = 0; i < st.iterations; i++) std::cout << " " << history[(size_t)i];
        std::cout << std::endl;
        if (out) *out = st;
        performance_stats.print_algorithm_performance_stats("LP (fused)", tm.get_time(), st.edges_examined);
        return performance_stats.get_algorithm_performance(tm.get_time(), st.edges_examined);
    }

    // the contract restated sequentially: synchronous steps, most frequent label of the stored adjacency, ties to the largest label
    static std::vector<int> seq_label_propagation(const HostCSR &g, std::vector<int> labels, int max_iterations)
    {
        std::vector<int> next(labels), seg;
        for (int it = 0; it < max_iterations; it++) {
            long long changed = 0;
            for (int v = 0; v < g.V; v++) {
                seg.clear();
                for (long long p = g.rowptr[(size_t)v]; p < g.rowptr[(size_t)v + 1]; p++) seg.push_back(labels[(size_t)g.adj[(size_t)p]]);
                next[(size_t)v] = labels[(size_t)v];
                if (seg.empty()) continue;
                std::sort(seg.begin(), seg.end());
                size_t best = 0;
                for (size_t i = 0; i < seg.size();) {
                    size_t j = i;
                    while (j < seg.size() && seg[j] == seg[i]) j++;
                    if (j - i >= best) { best = j - i; next[(size_t)v] = seg[i]; }      // ascending: >= keeps the largest of equal counts
                    i = j;
                }
                if (next[(size_t)v] != labels[(size_t)v]) changed++;
            }
            labels.swap(next);
            if (changed == 0) break;
        }
        return labels;
    }
};
#define LP LabelPropagation
