// Multi-source BFS and closeness (`closeness`): the fused HIP path (vgl_hip_msbfs_run, the contract of include/vgl_hip.h) and a sequential host BFS per
// source of the same contract for -check.  The reference has no multi-source traversal.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

struct ClosenessCentrality {
    struct Record { long long reached, dist_sum; int ecc, pad; double harmonic; };      // one per source: the layout of -dump
    static_assert(sizeof(Record) == 32, "a dump record is 32 bytes");

    // sources: host ids in the graph's own numbering; direction 0 = along outgoing entries, 1 = along incoming.  Prepare (the row classes) stays outside the timing.
    static double hip_fused(VGL_Graph &graph, const std::vector<int> &sources, int direction, std::vector<Record> &out, vgl_hip_msbfs_stats *stats = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const size_t K = sources.size();
        void *d_reached = nullptr, *d_sum = nullptr, *d_ecc = nullptr, *d_harmonic = nullptr;
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(long long) * std::max<size_t>(K, 1), &d_reached));
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(long long) * std::max<size_t>(K, 1), &d_sum));
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(int) * std::max<size_t>(K, 1), &d_ecc));
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(double) * std::max<size_t>(K, 1), &d_harmonic));
        Timer prep;
        prep.start();
        VGL_HIP_CALL(vgl_hip_msbfs_prepare(c, graph.get_handle(), direction, 0));
        prep.end();
        vgl_hip_msbfs_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_msbfs_run(c, graph.get_handle(), sources.data(), (int32_t)K, direction, 0, (int64_t *)d_reached, (int64_t *)d_sum, (int32_t *)d_ecc, (double *)d_harmonic, nullptr, &st));
        tm.end();
        std::vector<long long> reached(K), sum(K);
        std::vector<int> ecc(K);
        std::vector<double> harmonic(K);
        if (K > 0) {
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, reached.data(), d_reached, sizeof(long long) * K));
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, sum.data(), d_sum, sizeof(long long) * K));
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, ecc.data(), d_ecc, sizeof(int) * K));
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, harmonic.data(), d_harmonic, sizeof(double) * K));
        }
        VGL_HIP_CALL(vgl_hip_free(c, d_reached));
        VGL_HIP_CALL(vgl_hip_free(c, d_sum));
        VGL_HIP_CALL(vgl_hip_free(c, d_ecc));
        VGL_HIP_CALL(vgl_hip_free(c, d_harmonic));
        out.assign(K, Record{0, 0, 0, 0, 0.0});
        for (size_t i = 0; i < K; i++) out[i] = Record{reached[i], sum[i], ecc[i], 0, harmonic[i]};
        // the aggregate rate: every traversal is charged the stored entries of the graph, as the bfs app charges one
        const long long edges = (long long)graph.get_edges_count() * (long long)K;
        const double ms = tm.get_time() * 1000.0;
        std::cout << "CLOSENESS: " << st.sources << " sources in " << st.batches << " batches, " << ms / std::max(st.batches, 1) << " ms per batch, " << ms / std::max<size_t>(K, 1)
                  << " ms per source, aggregate " << edges / (tm.get_time() * 1e9) << " GTEPS, max depth " << st.max_depth << ", levels " << st.levels_total << " (push "
                  << st.levels_push << ", pull " << st.levels_pull << "), reached " << st.reached_total << ", entries push / pull " << st.edges_push << " / " << st.edges_pull
                  << ", prepare " << prep.get_time() * 1000.0 << " ms, " << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s of the bytes model" << std::endl;
        if (stats) *stats = st;
        performance_stats.print_algorithm_performance_stats("CLOSENESS (fused)", tm.get_time(), edges);
        return performance_stats.get_algorithm_performance(tm.get_time(), edges);
    }

    // a queue BFS per source over g (the CSR of the traversal direction); harmonic by the contract's loop: ascending d, one division and one addition per level
    static std::vector<Record> seq_bfs_sums(const HostCSR &g, const std::vector<int> &sources)
    {
        const size_t V = (size_t)g.V;
        std::vector<Record> out;
        std::vector<int> dist(V), order;
        std::vector<long long> at;
        for (int s : sources) {
            std::fill(dist.begin(), dist.end(), -1);
            order.clear();
            at.assign(1, 1);
            dist[(size_t)s] = 0;
            order.push_back(s);
            for (size_t head = 0; head < order.size(); head++) {
                const int u = order[head];
                for (long long p = g.rowptr[(size_t)u]; p < g.rowptr[(size_t)u + 1]; p++) {
                    const int w = g.adj[(size_t)p];
                    if (dist[(size_t)w] >= 0) continue;
                    dist[(size_t)w] = dist[(size_t)u] + 1;
                    if ((size_t)dist[(size_t)w] >= at.size()) at.push_back(0);
                    at[(size_t)dist[(size_t)w]]++;
                    order.push_back(w);
                }
            }
            Record r{(long long)order.size(), 0, (int)at.size() - 1, 0, 0.0};
            for (size_t d = 1; d < at.size(); d++) {
                r.dist_sum += at[d] * (long long)d;
                r.harmonic = r.harmonic + (double)at[d] / (double)d;
            }
            out.push_back(r);
        }
        return out;
    }

    // all four outputs for equality, harmonic bit for bit
    static int verify(const std::vector<Record> &got, const std::vector<Record> &want)
    {
        int errors = 0;
        for (size_t i = 0; i < want.size(); i++) {
            const bool same = i < got.size() && got[i].reached == want[i].reached && got[i].dist_sum == want[i].dist_sum && got[i].ecc == want[i].ecc &&
                              std::memcmp(&got[i].harmonic, &want[i].harmonic, sizeof(double)) == 0;
            if (!same && errors++ < 10 && i < got.size())
                std::cout << "error at source " << i << ": reached " << got[i].reached << " vs " << want[i].reached << ", dist_sum " << got[i].dist_sum << " vs " << want[i].dist_sum
                          << ", ecc " << got[i].ecc << " vs " << want[i].ecc << ", harmonic " << got[i].harmonic << " vs " << want[i].harmonic << std::endl;
        }
        std::cout << "error count: " << errors << std::endl;
        return errors;
    }
};
#define CLOSENESS ClosenessCentrality
