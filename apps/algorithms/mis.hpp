// Maximal independent set and maximal matching: the fused HIP paths (vgl_hip_mis_run, vgl_hip_matching_run, the contract of include/vgl_hip.h) and
// the sequential host greedy that defines them, for -check: sort the vertices (edges) by (key, id), one pass.  The reference has neither algorithm.
#pragma once
#include <algorithm>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

struct MIS {
    static uint32_t fmix32(uint32_t h)
    {
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        return h;
    }
    static uint32_t key(uint32_t i, uint32_t seed) { return fmix32(i ^ fmix32(seed + 0x9e3779b9u)); }

    // device arrays per vertex and (matching) per edge of the library's numbering
    struct Result {
        long long n = 0;                                       // E' (matching)
        int V = 0;
        int *round = nullptr, *u = nullptr, *v = nullptr, *mate = nullptr;
        unsigned char *in_set = nullptr, *in_matching = nullptr;
        ~Result()
        {
            MemoryAPI::free_device_array(round); MemoryAPI::free_device_array(u); MemoryAPI::free_device_array(v); MemoryAPI::free_device_array(mate);
            MemoryAPI::free_device_array(in_set); MemoryAPI::free_device_array(in_matching);
        }
        template <class T>
        std::vector<T> host(const T *d, long long count) const
        {
            std::vector<T> h((size_t)count);
            if (count) VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), d, sizeof(T) * (size_t)count));
            return h;
        }
    };

    // the symmetric CSR (and, for the matching, the edge numbering): outside the timing of the runs; allocates the result arrays
    static double prepare(VGL_Graph &graph, Result &r, bool matching)
    {
        Timer prep;
        prep.start();
        int64_t n = 0;
        if (matching) VGL_HIP_CALL(vgl_hip_matching_prepare(VGL_RUNTIME::ctx(), graph.get_handle(), &n));
        else VGL_HIP_CALL(vgl_hip_mis_prepare(VGL_RUNTIME::ctx(), graph.get_handle()));
        prep.end();
        r.n = n;
        r.V = graph.get_vertices_count();
        const size_t cap = (size_t)std::max<int64_t>(n, 1), vcap = (size_t)std::max(r.V, 1);
        MemoryAPI::allocate_device_array(&r.round, vcap);
        if (matching) {
            MemoryAPI::allocate_device_array(&r.u, cap);
            MemoryAPI::allocate_device_array(&r.v, cap);
            MemoryAPI::allocate_device_array(&r.in_matching, cap);
            MemoryAPI::allocate_device_array(&r.mate, vcap);
        } else MemoryAPI::allocate_device_array(&r.in_set, vcap);
        return prep.get_time();
    }

    static double hip_fused(VGL_Graph &graph, Result &r, bool matching, uint32_t seed, double prepare_s)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        Timer tm;
        int64_t entries = 0;
        if (matching) {
            vgl_hip_matching_stats st;
            tm.start();
            VGL_HIP_CALL(vgl_hip_matching_run(c, graph.get_handle(), nullptr, seed, r.u, r.v, r.in_matching, r.mate, r.round, &st));
            tm.end();
            std::cout << "MATCHING: " << st.matched_edges << " edges, " << st.matched_vertices << " matched vertices, " << st.rounds << " rounds, live_total " << st.live_total
                      << ", entries_walked " << st.entries_walked << ", " << st.undirected_edges << " undirected edges, " << tm.get_time() * 1000.0 << " ms, prepare "
                      << prepare_s * 1000.0 << " ms, " << st.algorithmic_bytes << " bytes of the model, " << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s" << std::endl;
            entries = 2 * st.undirected_edges;
        } else {
            vgl_hip_mis_stats st;
            tm.start();
            VGL_HIP_CALL(vgl_hip_mis_run(c, graph.get_handle(), nullptr, seed, r.in_set, r.round, &st));
            tm.end();
            std::cout << "MIS: " << st.set_size << " vertices, " << st.rounds << " rounds, live_total " << st.live_total << ", entries_walked " << st.entries_walked << ", "
                      << tm.get_time() * 1000.0 << " ms, prepare " << prepare_s * 1000.0 << " ms, " << st.algorithmic_bytes << " bytes of the model, "
                      << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s" << std::endl;
            entries = st.entries_walked;
        }
        performance_stats.print_algorithm_performance_stats(matching ? "MATCHING (fused)" : "MIS (fused)", tm.get_time(), entries);
        return performance_stats.get_algorithm_performance(tm.get_time(), entries);
    }

    // launches per timing slot of one more (untimed) run with the event brackets on
    static void print_launches(VGL_Graph &graph, Result &r, bool matching, uint32_t seed)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        if (matching) VGL_HIP_CALL(vgl_hip_matching_run(c, graph.get_handle(), nullptr, seed, r.u, r.v, r.in_matching, r.mate, r.round, nullptr));
        else VGL_HIP_CALL(vgl_hip_mis_run(c, graph.get_handle(), nullptr, seed, r.in_set, r.round, nullptr));
        int64_t total = 0;
        std::cout << (matching ? "MATCHING launches:" : "MIS launches:");
        const std::vector<const char *> names = matching ? std::vector<const char *>{"mm_init", "mm_best_short", "mm_best_wave", "mm_best_wg", "mm_match", "mm_publish"}
                                                         : std::vector<const char *>{"mis_init", "mis_short", "mis_wave", "mis_wg", "mis_publish", "mis_finish"};
        for (const char *name : names) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    // ---- the contract on the host.  g: the stored outgoing CSR ----
    // the undirected edges in the library's numbering: lo < hi, ascending (lo, hi), every edge once
    static std::vector<std::pair<int, int>> host_edges(const HostCSR &g)
    {
        std::vector<std::pair<int, int>> all;
        all.reserve(g.adj.size());
        for (int u = 0; u < g.V; u++)
            for (long long p = g.rowptr[(size_t)u]; p < g.rowptr[(size_t)u + 1]; p++) {
                const int v = g.adj[(size_t)p];
                if (v != u) all.emplace_back(std::min(u, v), std::max(u, v));
            }
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        return all;
    }
    // ids 0 .. n - 1 ascending by (key, id)
    static std::vector<int> host_order(size_t n, uint32_t seed)
    {
        std::vector<std::pair<uint32_t, int>> k(n);
        for (size_t i = 0; i < n; i++) k[i] = {key((uint32_t)i, seed), (int)i};
        std::sort(k.begin(), k.end());
        std::vector<int> order(n);
        for (size_t i = 0; i < n; i++) order[i] = k[i].second;
        return order;
    }
    static std::vector<unsigned char> seq_greedy_mis(const HostCSR &g, uint32_t seed)
    {
        const std::vector<std::pair<int, int>> edges = host_edges(g);
        const size_t V = (size_t)g.V;
        std::vector<long long> ptr(V + 1, 0);
        for (const auto &e : edges) { ptr[(size_t)e.first + 1]++; ptr[(size_t)e.second + 1]++; }
        for (size_t v = 0; v < V; v++) ptr[v + 1] += ptr[v];
        std::vector<int> adj(2 * edges.size());
        {
            std::vector<long long> at(ptr.begin(), ptr.end() - 1);
            for (const auto &e : edges) { adj[(size_t)at[(size_t)e.first]++] = e.second; adj[(size_t)at[(size_t)e.second]++] = e.first; }
        }
        std::vector<unsigned char> in_set(V, 0), blocked(V, 0);
        for (int v : host_order(V, seed)) {
            if (blocked[(size_t)v]) continue;
            in_set[(size_t)v] = 1;
            for (long long p = ptr[(size_t)v]; p < ptr[(size_t)v + 1]; p++) blocked[(size_t)adj[(size_t)p]] = 1;
        }
        return in_set;
    }
    struct HostMatching {
        std::vector<int> u, v, mate;
        std::vector<unsigned char> in_matching;
    };
    static HostMatching seq_greedy_matching(const HostCSR &g, uint32_t seed)
    {
        const std::vector<std::pair<int, int>> edges = host_edges(g);
        HostMatching h;
        h.u.resize(edges.size()); h.v.resize(edges.size());
        for (size_t e = 0; e < edges.size(); e++) { h.u[e] = edges[e].first; h.v[e] = edges[e].second; }
        h.mate.assign((size_t)g.V, -1);
        h.in_matching.assign(edges.size(), 0);
        for (int e : host_order(edges.size(), seed)) {
            const int a = h.u[(size_t)e], b = h.v[(size_t)e];
            if (h.mate[(size_t)a] >= 0 || h.mate[(size_t)b] >= 0) continue;
            h.mate[(size_t)a] = b; h.mate[(size_t)b] = a;
            h.in_matching[(size_t)e] = 1;
        }
        return h;
    }
};
