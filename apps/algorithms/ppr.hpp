// Batched personalised PageRank (`ppr`): the fused HIP path (vgl_hip_ppr_run, the contract of include/vgl_hip.h) and a sequential host restatement
// of the same contract (float64, row order) for -check.  The reference has no personalised PageRank; apps/pr.cpp is its benchmark kernel.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

struct PersonalisedPageRank {
    struct Options { double alpha = 0.85, tol = 0.0; int iterations = 20; };

    // seeds: one vertex per problem, host ids in the graph's own numbering.  rank: K x V in the graph's numbering; iterations: per problem, what its
    // batch ran.  Prepare (the class lists) stays outside the timing.
    static double hip_fused(VGL_Graph &graph, const std::vector<int> &seeds, const Options &o, std::vector<double> &rank, std::vector<int> &iterations, vgl_hip_ppr_stats *stats = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const size_t K = seeds.size(), V = (size_t)graph.get_vertices_count();
        std::vector<int64_t> ptr(K + 1);
        for (size_t i = 0; i <= K; i++) ptr[i] = (int64_t)i;
        void *d_rank = nullptr, *d_it = nullptr;
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(double) * std::max<size_t>(K * V, 1), &d_rank));
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(int) * std::max<size_t>(K, 1), &d_it));
        Timer prep;
        prep.start();
        VGL_HIP_CALL(vgl_hip_ppr_prepare(c, graph.get_handle(), 0));
        prep.end();
        vgl_hip_ppr_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_ppr_run(c, graph.get_handle(), seeds.data(), ptr.data(), nullptr, (int32_t)K, o.alpha, o.iterations, o.tol, 0, (double *)d_rank, nullptr, (int32_t *)d_it, &st));
        tm.end();
        rank.assign(K * V, 0.0);
        iterations.assign(K, 0);
        if (K > 0) {
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, rank.data(), d_rank, sizeof(double) * K * V));
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, iterations.data(), d_it, sizeof(int) * K));
        }
        VGL_HIP_CALL(vgl_hip_free(c, d_rank));
        VGL_HIP_CALL(vgl_hip_free(c, d_it));
        const double ms = tm.get_time() * 1000.0;
        std::cout << "PPR: " << st.sources << " sources in " << st.batches << " batches (" << st.batches_converged << " stopped by the tolerance), " << ms / std::max(st.batches, 1)
                  << " ms per batch, " << ms / (double)std::max<int64_t>(st.iterations_total, 1) << " ms per iteration, " << ms / (double)std::max<size_t>(K, 1)
                  << " ms per source, iterations total / max " << st.iterations_total << " / " << st.iterations_max << ", entries walked " << st.entries_walked << ", largest err "
                  << st.max_err << ", prepare " << prep.get_time() * 1000.0 << " ms (built now: " << st.prepared_now << "), " << st.algorithmic_bytes << " bytes of the model, "
                  << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s" << std::endl;
        if (stats) *stats = st;
        performance_stats.print_algorithm_performance_stats("PPR (fused)", tm.get_time(), st.entries_walked);
        return performance_stats.get_algorithm_performance(tm.get_time(), st.entries_walked);
    }

    // launches per timing slot of one more (untimed) run with the event brackets on
    static void print_launches(VGL_Graph &graph, const std::vector<int> &seeds, const Options &o)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        std::vector<double> rank;
        std::vector<int> it;
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        const size_t K = seeds.size(), V = (size_t)graph.get_vertices_count();
        std::vector<int64_t> ptr(K + 1);
        for (size_t i = 0; i <= K; i++) ptr[i] = (int64_t)i;
        void *d_rank = nullptr;
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(double) * std::max<size_t>(K * V, 1), &d_rank));
        VGL_HIP_CALL(vgl_hip_ppr_run(c, graph.get_handle(), seeds.data(), ptr.data(), nullptr, (int32_t)K, o.alpha, o.iterations, o.tol, 0, (double *)d_rank, nullptr, nullptr, nullptr));
        VGL_HIP_CALL(vgl_hip_free(c, d_rank));
        int64_t total = 0;
        std::cout << "PPR launches:";
        for (const char *name : {"ppr_prepare", "ppr_pull_short", "ppr_pull_wave", "ppr_pull_wg", "ppr_fold", "ppr_teleport", "ppr_out"}) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    // the contract on the host, one seed per problem: `iterations[j]` iterations of the rule from x = p, every sum in row order.  in: the incoming
    // CSR, out: the outgoing.  *d_max: the largest in-degree, *dangling: the vertices without an outgoing entry (both enter the tolerance).
    static std::vector<double> seq_ppr(const HostCSR &out, const HostCSR &in, const std::vector<int> &seeds, const std::vector<int> &iterations, double alpha, long long *d_max,
                                       long long *dangling)
    {
        const size_t V = (size_t)out.V;
        *d_max = 0;
        *dangling = 0;
        for (size_t v = 0; v < V; v++) {
            *d_max = std::max(*d_max, in.rowptr[v + 1] - in.rowptr[v]);
            *dangling += out.rowptr[v + 1] == out.rowptr[v];
        }
        std::vector<double> rank(seeds.size() * V), x(V), y(V), xn(V);
        for (size_t j = 0; j < seeds.size(); j++) {
            std::fill(x.begin(), x.end(), 0.0);
            x[(size_t)seeds[j]] = 1.0;
            for (int t = 0; t < iterations[j]; t++) {
                double D = 0.0;
                for (size_t u = 0; u < V; u++) {
                    const long long od = out.rowptr[u + 1] - out.rowptr[u];
                    y[u] = od > 0 ? x[u] / (double)od : 0.0;
                    if (od == 0) D = D + x[u];
                }
                for (size_t v = 0; v < V; v++) {
                    double acc = 0.0;
                    for (long long p = in.rowptr[v]; p < in.rowptr[v + 1]; p++) acc = acc + y[(size_t)in.adj[(size_t)p]];
                    xn[v] = alpha * acc;
                }
                xn[(size_t)seeds[j]] = xn[(size_t)seeds[j]] + (alpha * D + (1.0 - alpha)) * 1.0;
                x.swap(xn);
            }
            std::copy(x.begin(), x.end(), rank.begin() + (std::ptrdiff_t)(j * V));
        }
        return rank;
    }

    // two float64 evaluations: per problem |got - want|_1 <= 2 gamma_k (1 - alpha^t) / (1 - alpha), k = max(d_max, dangling) + 6
    static int verify(const std::vector<double> &got, const std::vector<double> &want, size_t V, const std::vector<int> &iterations, double alpha, long long d_max, long long dangling)
    {
        const double ku = (double)(std::max(d_max, dangling) + 6) * std::ldexp(1.0, -53), gamma = ku / (1.0 - ku);
        int errors = 0;
        double worst = 0.0;
        for (size_t j = 0; j < iterations.size(); j++) {
            const double bound = 2.0 * gamma * (1.0 - std::pow(alpha, (double)iterations[j])) / (1.0 - alpha);
            double l1 = 0.0;
            for (size_t v = 0; v < V; v++) l1 += std::fabs(got[j * V + v] - want[j * V + v]);
            if (bound > 0.0) worst = std::max(worst, l1 / bound);
            if (!(l1 <= bound) && errors++ < 10) std::cout << "error at source " << j << ": L1 difference " << l1 << " above the bound " << bound << std::endl;
        }
        std::cout << "largest L1 difference / bound: " << worst << std::endl;
        std::cout << "error count: " << errors << std::endl;
        return errors;
    }
};
#define PPR PersonalisedPageRank
