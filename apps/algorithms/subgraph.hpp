// Subgraph extraction, k-hop reach and neighbour sampling: the fused HIP paths (vgl_hip_subgraph_plan_*, vgl_hip_khop_run, vgl_hip_sample_neighbors, the
// contract of include/vgl_hip.h) and the sequential host restatement for -check: a filter of the stored rows in order, a host BFS bounded by the hop
// count, and the selection as a sort of (key, position), take F, sort by position.  The reference has no such algorithm.
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

struct SUBG {
    static uint32_t fmix32(uint32_t h)
    {
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        return h;
    }
    // key(i, seed) of the contract; also the counter hash of the default masks and seeds
    static uint32_t key(uint32_t i, uint32_t seed) { return fmix32(i ^ fmix32(seed + 0x9e3779b9u)); }

    template <class T>
    struct Device {                                                  // an owned device array
        T *p = nullptr;
        size_t n = 0;
        Device() = default;
        Device(const Device &) = delete;
        Device &operator=(const Device &) = delete;
        ~Device() { MemoryAPI::free_device_array(p); }
        void alloc(size_t count)
        {
            MemoryAPI::free_device_array(p);
            p = nullptr;
            n = count;
            MemoryAPI::allocate_device_array(&p, std::max<size_t>(count, 1));
        }
        void upload(const std::vector<T> &h)
        {
            alloc(h.size());
            if (!h.empty()) VGL_HIP_CALL(vgl_hip_memcpy_h2d(VGL_RUNTIME::ctx(), p, h.data(), h.size() * sizeof(T)));
        }
        std::vector<T> host() const
        {
            std::vector<T> h(n);
            if (n) VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), p, n * sizeof(T)));
            return h;
        }
    };

    struct Sub {                                                     // one extracted subgraph, both directions
        int V = 0;
        long long E[2] = {0, 0};
        Device<int> old_id, adj[2];
        Device<long long> rowptr[2], origin;
        vgl_hip_subgraph_stats st;
    };

    // plan + fills of the vertex mask `keep` (device, V flags); returns (plan seconds, fill seconds)
    static std::pair<double, double> extract(VGL_Graph &graph, const unsigned char *d_keep, Sub &s)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        vgl_hip_subgraph_plan *plan = nullptr;
        Timer tp, tf;
        tp.start();
        VGL_HIP_CALL(vgl_hip_subgraph_plan_create(c, graph.get_handle(), d_keep, nullptr, &plan));
        tp.end();
        int32_t vk = 0;
        int64_t eo = 0, ei = 0;
        VGL_HIP_CALL(vgl_hip_subgraph_plan_info(plan, &vk, &eo, &ei, &s.st));
        s.V = vk; s.E[0] = eo; s.E[1] = ei < 0 ? 0 : ei;
        s.old_id.alloc((size_t)vk);
        for (int d = 0; d < 2; d++) { s.rowptr[d].alloc((size_t)vk + 1); s.adj[d].alloc((size_t)s.E[d]); }
        s.origin.alloc((size_t)eo);
        tf.start();
        VGL_HIP_CALL(vgl_hip_subgraph_plan_vertex_maps(c, plan, nullptr, s.old_id.p));
        VGL_HIP_CALL(vgl_hip_subgraph_plan_fill(c, plan, 0, (int64_t *)s.rowptr[0].p, s.adj[0].p, (int64_t *)s.origin.p));
        if (ei >= 0) VGL_HIP_CALL(vgl_hip_subgraph_plan_fill(c, plan, 1, (int64_t *)s.rowptr[1].p, s.adj[1].p, nullptr));
        VGL_HIP_CALL(vgl_hip_ctx_sync(c));
        tf.end();
        VGL_HIP_CALL(vgl_hip_subgraph_plan_destroy(c, plan));
        return {tp.get_time(), tf.get_time()};
    }

    static void print_launches(const char *what, const std::vector<const char *> &names)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        int64_t total = 0;
        std::cout << what << " launches:";
        for (const char *name : names) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
    }

    // ---- the contract on the host ----
    // the rows of `g` filtered by keep, in stored order; returns rowptr / adj / origin of the result (new ids = rank among the kept)
    static void seq_filter(const HostCSR &g, const std::vector<unsigned char> &keep, std::vector<long long> &rowptr, std::vector<int> &adj, std::vector<long long> &origin,
                           std::vector<int> &old_id)
    {
        std::vector<int> new_id((size_t)g.V, -1);
        old_id.clear();
        for (int v = 0; v < g.V; v++)
            if (keep[(size_t)v]) { new_id[(size_t)v] = (int)old_id.size(); old_id.push_back(v); }
        rowptr.assign(1, 0);
        adj.clear();
        origin.clear();
        for (int v : old_id) {
            for (long long p = g.rowptr[(size_t)v]; p < g.rowptr[(size_t)v + 1]; p++) {
                const int w = new_id[(size_t)g.adj[(size_t)p]];
                if (w >= 0) { adj.push_back(w); origin.push_back(p); }
            }
            rowptr.push_back((long long)adj.size());
        }
    }
    static std::vector<int> seq_khop(const HostCSR &g, const std::vector<int> &seeds, int hops)
    {
        std::vector<int> hop((size_t)g.V, -1), front, next;
        for (int s : seeds)
            if (hop[(size_t)s] < 0) { hop[(size_t)s] = 0; front.push_back(s); }
        for (int level = 0; level < hops && !front.empty(); level++) {
            next.clear();
            for (int v : front)
                for (long long p = g.rowptr[(size_t)v]; p < g.rowptr[(size_t)v + 1]; p++) {
                    const int w = g.adj[(size_t)p];
                    if (hop[(size_t)w] < 0) { hop[(size_t)w] = level + 1; next.push_back(w); }
                }
            front.swap(next);
        }
        return hop;
    }
    // the positions chosen for the row of v: sort of (key, p), take fanout, sort by p
    static std::vector<long long> seq_select(const HostCSR &g, int v, int fanout, uint32_t seed)
    {
        std::vector<std::pair<uint32_t, long long>> all;
        for (long long p = g.rowptr[(size_t)v]; p < g.rowptr[(size_t)v + 1]; p++) all.emplace_back(key((uint32_t)p, seed), p);
        std::sort(all.begin(), all.end());
        if ((long long)all.size() > fanout) all.resize((size_t)fanout);
        std::vector<long long> out;
        for (const auto &x : all) out.push_back(x.second);
        std::sort(out.begin(), out.end());
        return out;
    }
};
