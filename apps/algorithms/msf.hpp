// Minimum spanning forest: the fused HIP path (vgl_hip_msf_run, the contract of include/vgl_hip.h) and a sequential host restatement of that contract
// for -check (the stored entries folded to the lightest copy per undirected edge, Kruskal under (weight, edge id) with union-find).  The reference has
// no minimum spanning forest.
#pragma once
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

struct MSF {
    // device arrays of E' entries each, in the library's edge numbering (ascending (lo, hi) of the graph's own vertex ids)
    struct Edges {
        long long n = 0;
        int *u = nullptr, *v = nullptr;
        float *w = nullptr;
        unsigned char *in_forest = nullptr;
        ~Edges()
        {
            MemoryAPI::free_device_array(u); MemoryAPI::free_device_array(v); MemoryAPI::free_device_array(w); MemoryAPI::free_device_array(in_forest);
        }
        template <class T>
        std::vector<T> host(const T *d) const
        {
            std::vector<T> h((size_t)n);
            if (n) VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), d, sizeof(T) * (size_t)n));
            return h;
        }
    };
    // one undirected edge of the host restatement
    struct HostEdge { int lo, hi; float w; };

    // what is kept per graph (symmetric CSR, edge numbering, the edge of every stored entry): outside the timing of the runs; allocates the result arrays
    static double prepare(VGL_Graph &graph, Edges &e)
    {
        Timer prep;
        prep.start();
        int64_t n = 0;
        VGL_HIP_CALL(vgl_hip_msf_prepare(VGL_RUNTIME::ctx(), graph.get_handle(), &n));
        prep.end();
        e.n = n;
        const size_t cap = (size_t)std::max<int64_t>(n, 1);
        MemoryAPI::allocate_device_array(&e.u, cap);
        MemoryAPI::allocate_device_array(&e.v, cap);
        MemoryAPI::allocate_device_array(&e.w, cap);
        MemoryAPI::allocate_device_array(&e.in_forest, cap);
        return prep.get_time();
    }

    static double hip_fused(VGL_Graph &graph, EdgesArray<float> &weights, Edges &e, double prepare_s, vgl_hip_msf_stats *out = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        vgl_hip_msf_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_msf_run(c, graph.get_handle(), weights.get_ptr(), e.u, e.v, e.w, e.in_forest, nullptr, &st));
        tm.end();
        std::cout << "MSF: " << st.forest_edges << " forest edges, " << st.components << " components, total weight " << st.total_weight << ", " << st.rounds << " rounds, "
                  << st.undirected_edges << " undirected edges, " << tm.get_time() * 1000.0 << " ms, prepare " << prepare_s * 1000.0 << " ms, " << st.entries_walked
                  << " entries walked (" << (st.undirected_edges ? (double)st.entries_walked / (2.0 * (double)st.undirected_edges) : 0.0) << " x 2E'), "
                  << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s of the bytes model" << std::endl;
        if (out) *out = st;
        performance_stats.print_algorithm_performance_stats("MSF (fused)", tm.get_time(), st.entries_walked);
        return performance_stats.get_algorithm_performance(tm.get_time(), st.entries_walked);
    }

    // launches per timing slot of one more (untimed) run with the event brackets on
    static void print_launches(VGL_Graph &graph, EdgesArray<float> &weights, Edges &e)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        VGL_HIP_CALL(vgl_hip_msf_run(c, graph.get_handle(), weights.get_ptr(), e.u, e.v, e.w, e.in_forest, nullptr, nullptr));
        int64_t total = 0;
        std::cout << "MSF launches:";
        for (const char *name : {"msf_fold", "msf_min_short", "msf_min_wave", "msf_min_wg", "msf_hook", "msf_flatten", "msf_publish"}) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    // The undirected edges of the contract in the library's numbering (ascending (lo, hi)), each with its lightest stored copy.  g / w: the stored
    // outgoing CSR and its weights.  A NaN compares false and so never replaces a number: the library refuses such weights before this is asked.
    static std::vector<HostEdge> fold(const HostCSR &g, const std::vector<float> &w)
    {
        std::vector<HostEdge> all;
        all.reserve(g.adj.size());
        for (int u = 0; u < g.V; u++)
            for (long long p = g.rowptr[(size_t)u]; p < g.rowptr[(size_t)u + 1]; p++) {
                const int v = g.adj[(size_t)p];
                if (v != u) all.push_back(HostEdge{std::min(u, v), std::max(u, v), w[(size_t)p] == 0.0f ? 0.0f : w[(size_t)p]});      // (-0.0 is 0.0)
            }
        std::sort(all.begin(), all.end(), [](const HostEdge &a, const HostEdge &b) { return a.lo != b.lo ? a.lo < b.lo : a.hi != b.hi ? a.hi < b.hi : a.w < b.w; });
        size_t n = 0;
        for (size_t i = 0; i < all.size(); i++)
            if (n == 0 || all[i].lo != all[n - 1].lo || all[i].hi != all[n - 1].hi) all[n++] = all[i];
        all.resize(n);
        return all;
    }

    // Kruskal: the edges in ascending (weight, id), an edge joins the forest iff its ends lie in different trees
    static std::vector<unsigned char> seq_kruskal(int V, const std::vector<HostEdge> &edges, double *total_weight)
    {
        std::vector<int> order(edges.size()), parent((size_t)V);
        std::iota(order.begin(), order.end(), 0);
        std::iota(parent.begin(), parent.end(), 0);
        std::sort(order.begin(), order.end(), [&](int a, int b) { return edges[(size_t)a].w != edges[(size_t)b].w ? edges[(size_t)a].w < edges[(size_t)b].w : a < b; });
        auto find = [&](int x) {
            while (parent[(size_t)x] != x) { parent[(size_t)x] = parent[(size_t)parent[(size_t)x]]; x = parent[(size_t)x]; }
            return x;
        };
        std::vector<unsigned char> in_forest(edges.size(), 0);
        double total = 0.0;
        for (int e : order) {
            const int a = find(edges[(size_t)e].lo), b = find(edges[(size_t)e].hi);
            if (a == b) continue;
            parent[(size_t)std::max(a, b)] = std::min(a, b);
            in_forest[(size_t)e] = 1;
            total += (double)edges[(size_t)e].w;
        }
        if (total_weight) *total_weight = total;
        return in_forest;
    }
};
