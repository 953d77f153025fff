// Betweenness centrality (`bc`): the fused HIP path (vgl_hip_bc_run, the contract of include/vgl_hip.h) and a sequential host Brandes (queue + stack)
// of the same contract for -check.  The reference has no betweenness centrality.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

struct BetweennessCentrality {
    // sources: host ids in the graph's own numbering; d_bc: device float64[V], overwritten.  Prepare (the row classes) stays outside the timing.
    static double hip_fused(VGL_Graph &graph, const std::vector<int> &sources, double *d_bc, vgl_hip_bc_stats *out = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        Timer prep;
        prep.start();
        VGL_HIP_CALL(vgl_hip_bc_prepare(c, graph.get_handle(), 0));
        prep.end();
        vgl_hip_bc_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_bc_run(c, graph.get_handle(), sources.data(), (int32_t)sources.size(), 0, 0, d_bc, nullptr, nullptr, nullptr, &st));
        tm.end();
        const long long edges = st.edges_forward + st.edges_backward;
        std::cout << "BC: " << st.sources << " sources, " << tm.get_time() * 1000.0 / std::max<size_t>(sources.size(), 1) << " ms per source, max depth " << st.max_depth
                  << ", reached " << st.reached_total << ", entries forward / backward " << st.edges_forward << " / " << st.edges_backward << ", sigma inexact "
                  << st.sigma_inexact << ", prepare " << prep.get_time() * 1000.0 << " ms, " << st.algorithmic_bytes / (tm.get_time() * 1e9)
                  << " GB/s of the bytes model" << std::endl;
        if (out) *out = st;
        performance_stats.print_algorithm_performance_stats("BC (fused)", tm.get_time(), edges);
        return performance_stats.get_algorithm_performance(tm.get_time(), edges);
    }

    // Brandes, sequentially: a queue for the levels and the path counts, the visit order as the stack for the dependencies.  Every stored entry is
    // an edge of its own.  *depth: the largest distance seen; *longest_row: the longest outgoing or incoming row (both enter the tolerance).
    static std::vector<double> seq_brandes(const HostCSR &g, const std::vector<int> &sources, int *depth, long long *longest_row)
    {
        const size_t V = (size_t)g.V;
        std::vector<double> bc(V, 0.0), sigma(V), delta(V);
        std::vector<int> dist(V), order;
        std::vector<long long> indeg(V, 0);
        *depth = 0;
        *longest_row = 0;
        for (size_t u = 0; u < V; u++) {
            *longest_row = std::max(*longest_row, g.rowptr[u + 1] - g.rowptr[u]);
            for (long long p = g.rowptr[u]; p < g.rowptr[u + 1]; p++) indeg[(size_t)g.adj[(size_t)p]]++;
        }
        for (size_t u = 0; u < V; u++) *longest_row = std::max(*longest_row, indeg[u]);
        for (int s : sources) {
            std::fill(sigma.begin(), sigma.end(), 0.0);
            std::fill(delta.begin(), delta.end(), 0.0);
            std::fill(dist.begin(), dist.end(), -1);
            order.clear();
            sigma[(size_t)s] = 1.0; dist[(size_t)s] = 0;
            order.push_back(s);
            for (size_t head = 0; head < order.size(); head++) {              // (the visit order is the queue)
                const int u = order[head];
                for (long long p = g.rowptr[(size_t)u]; p < g.rowptr[(size_t)u + 1]; p++) {
                    const int w = g.adj[(size_t)p];
                    if (dist[(size_t)w] < 0) { dist[(size_t)w] = dist[(size_t)u] + 1; order.push_back(w); *depth = std::max(*depth, dist[(size_t)w]); }
                    if (dist[(size_t)w] == dist[(size_t)u] + 1) sigma[(size_t)w] += sigma[(size_t)u];
                }
            }
            for (size_t i = order.size(); i-- > 0;) {
                const int u = order[i];
                double sum = 0.0;
                for (long long p = g.rowptr[(size_t)u]; p < g.rowptr[(size_t)u + 1]; p++) {
                    const int w = g.adj[(size_t)p];
                    if (dist[(size_t)w] == dist[(size_t)u] + 1) sum += (1.0 + delta[(size_t)w]) / sigma[(size_t)w];
                }
                delta[(size_t)u] = sigma[(size_t)u] * sum;
                if (u != s) bc[(size_t)u] += delta[(size_t)u];
            }
        }
        return bc;
    }

    // the tolerance of the tests: |got - want| <= 2 (D (d_max + 4) + S) 2^-53 want per vertex, exactly 0 where want is 0
    static int verify(const std::vector<double> &got, const std::vector<double> &want, int depth, long long longest_row, size_t n_sources)
    {
        const double tol = 2.0 * ((double)depth * (double)(longest_row + 4) + (double)n_sources) * std::ldexp(1.0, -53);
        int errors = 0;
        double worst = 0.0;
        for (size_t i = 0; i < got.size(); i++) {
            const bool same = want[i] == 0.0 ? got[i] == 0.0 : std::fabs(got[i] - want[i]) <= tol * want[i];
            if (want[i] != 0.0) worst = std::max(worst, std::fabs(got[i] - want[i]) / (tol * want[i]));
            if (!same && errors++ < 10) std::cout << "error at " << i << ": " << got[i] << " vs " << want[i] << std::endl;
        }
        std::cout << "largest error / bound: " << worst << " (bound " << tol << " relative)" << std::endl;
        std::cout << "error count: " << errors << std::endl;
        return errors;
    }
};
#define BC BetweennessCentrality
