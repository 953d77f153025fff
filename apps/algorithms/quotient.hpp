// Quotient graph: the fused HIP path (vgl_hip_quotient_plan_*, the contract of include/vgl_hip.h) and the sequential host restatement for -check:
// the (coarse row, coarse far end) key of every stored entry, a sort of the keys, a run-length sum.  The reference has no such algorithm.
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

struct QUOT {
    static uint32_t fmix32(uint32_t h)
    {
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        return h;
    }

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

    struct Quotient {                                                // one quotient graph, both directions
        int V = 0;
        long long E[2] = {0, 0};
        bool has_in = false;
        Device<int> cluster_of, label_of, size, adj[2];
        Device<long long> rowptr[2], count[2];
        vgl_hip_quotient_stats st;
    };

    // plan + fills of the labels (device, V entries); returns (plan seconds, fill seconds)
    static std::pair<double, double> run(VGL_Graph &graph, const int *d_label, bool drop_loops, Quotient &q)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        vgl_hip_quotient_plan *plan = nullptr;
        Timer tp, tf;
        tp.start();
        VGL_HIP_CALL(vgl_hip_quotient_plan_create(c, graph.get_handle(), d_label, drop_loops ? 1 : 0, &plan));
        tp.end();
        int32_t vc = 0;
        int64_t eo = 0, ei = 0;
        VGL_HIP_CALL(vgl_hip_quotient_plan_info(plan, &vc, &eo, &ei, &q.st));
        q.V = vc; q.E[0] = eo; q.E[1] = ei < 0 ? 0 : ei; q.has_in = ei >= 0;
        q.cluster_of.alloc((size_t)graph.get_vertices_count());
        q.label_of.alloc((size_t)vc);
        q.size.alloc((size_t)vc);
        for (int d = 0; d < 2; d++) { q.rowptr[d].alloc((size_t)vc + 1); q.adj[d].alloc((size_t)q.E[d]); q.count[d].alloc((size_t)q.E[d]); }
        tf.start();
        VGL_HIP_CALL(vgl_hip_quotient_plan_vertex_maps(c, plan, q.cluster_of.p, q.label_of.p, q.size.p));
        VGL_HIP_CALL(vgl_hip_quotient_plan_fill(c, plan, 0, nullptr, (int64_t *)q.rowptr[0].p, q.adj[0].p, (int64_t *)q.count[0].p));
        if (q.has_in) VGL_HIP_CALL(vgl_hip_quotient_plan_fill(c, plan, 1, nullptr, (int64_t *)q.rowptr[1].p, q.adj[1].p, (int64_t *)q.count[1].p));
        VGL_HIP_CALL(vgl_hip_ctx_sync(c));
        tf.end();
        VGL_HIP_CALL(vgl_hip_quotient_plan_destroy(c, plan));
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
    // the coarse ids: the rank of every label among the distinct label values
    static void seq_vertex_maps(const std::vector<int> &label, std::vector<int> &cluster_of, std::vector<int> &label_of, std::vector<int> &size)
    {
        label_of = label;
        std::sort(label_of.begin(), label_of.end());
        label_of.erase(std::unique(label_of.begin(), label_of.end()), label_of.end());
        cluster_of.resize(label.size());
        size.assign(label_of.size(), 0);
        for (size_t v = 0; v < label.size(); v++) {
            cluster_of[v] = (int)(std::lower_bound(label_of.begin(), label_of.end(), label[v]) - label_of.begin());
            size[(size_t)cluster_of[v]]++;
        }
    }
    // one direction: sort the (c(v), c(w)) pairs of the stored entries, run-length sum
    static void seq_quotient(const HostCSR &g, const std::vector<int> &cluster_of, int vc, bool drop_loops, std::vector<long long> &rowptr, std::vector<int> &adj,
                             std::vector<long long> &count)
    {
        std::vector<unsigned long long> keys;
        keys.reserve(g.adj.size());
        for (int v = 0; v < g.V; v++)
            for (long long p = g.rowptr[(size_t)v]; p < g.rowptr[(size_t)v + 1]; p++) {
                const unsigned long long c = (unsigned long long)cluster_of[(size_t)v], cw = (unsigned long long)cluster_of[(size_t)g.adj[(size_t)p]];
                if (!(drop_loops && c == cw)) keys.push_back(c << 32 | cw);
            }
        std::sort(keys.begin(), keys.end());
        rowptr.assign((size_t)vc + 1, 0);
        adj.clear();
        count.clear();
        for (size_t i = 0; i < keys.size(); i++) {
            if (i > 0 && keys[i] == keys[i - 1]) { count.back()++; continue; }
            adj.push_back((int)(keys[i] & 0xffffffffull));
            count.push_back(1);
            rowptr[(size_t)(keys[i] >> 32) + 1]++;
        }
        for (int c = 0; c < vc; c++) rowptr[(size_t)c + 1] += rowptr[(size_t)c];
    }
};
