// Vertex similarity and link prediction: the fused HIP paths (vgl_hip_sim_pairs, vgl_hip_sim_topk, the contract of include/vgl_hip.h) and the
// sequential host restatement for -check: the common neighbours of a pair by a merge of the two sorted rows; the top k of a query by a dense counter
// over its 2-paths and a sort by the total order.  The reference has no such algorithm.
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

struct SIM {
    static uint32_t fmix32(uint32_t h)
    {
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        return h;
    }
    // the counter hash of the default pairs: value i of the stream of `seed`
    static uint32_t hash(uint32_t i, uint32_t seed) { return fmix32(i ^ fmix32(seed + 0x9e3779b9u)); }

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

    struct Work {
        bool topk = false;
        int metric = VGL_HIP_SIM_JACCARD, k = 10, include = 0;
        Device<int> u, v, common;                                    // pairs (own numbering) and their counts
        Device<int> queries, label, ids, tk_common;                  // queries (own numbering), ORIGINAL ids as labels, n x k results
    };

    static double prepare(VGL_Graph &graph)
    {
        Timer prep;
        prep.start();
        VGL_HIP_CALL(vgl_hip_sim_prepare(VGL_RUNTIME::ctx(), graph.get_handle()));
        prep.end();
        return prep.get_time();
    }

    // d(v) of the simple undirected graph: a call without pairs writes nothing else
    static std::vector<int> degrees(VGL_Graph &graph)
    {
        Device<int> deg, dummy;
        deg.alloc((size_t)graph.get_vertices_count());
        dummy.alloc(1);
        VGL_HIP_CALL(vgl_hip_sim_pairs(VGL_RUNTIME::ctx(), graph.get_handle(), nullptr, nullptr, 0, nullptr, dummy.p, nullptr, deg.p, nullptr));
        return deg.host();
    }

    static void run(VGL_Graph &graph, Work &w, vgl_hip_sim_pairs_stats *ps, vgl_hip_sim_topk_stats *ts)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        if (w.topk)
            VGL_HIP_CALL(vgl_hip_sim_topk(c, graph.get_handle(), w.queries.p, (int32_t)w.queries.n, w.metric, w.k, w.include, w.label.p, w.ids.p, w.tk_common.p, ts));
        else
            VGL_HIP_CALL(vgl_hip_sim_pairs(c, graph.get_handle(), w.u.p, w.v.p, (int64_t)w.u.n, nullptr, w.common.p, nullptr, nullptr, ps));
    }

    static double hip_fused(VGL_Graph &graph, Work &w, double prepare_s)
    {
        vgl_hip_sim_pairs_stats ps;
        vgl_hip_sim_topk_stats ts;
        Timer tm;
        tm.start();
        run(graph, w, &ps, &ts);
        tm.end();
        long long work = 0, bytes = 0;
        if (w.topk) {
            std::cout << "SIM top-k: " << ts.queries << " queries, k " << w.k << ", rows small / table / global " << ts.rows_small << " / " << ts.rows_table << " / " << ts.rows_global
                      << ", two_paths_walked " << ts.two_paths_walked << ", candidates_total " << ts.candidates_total << ", filled " << ts.filled << ", scratch_slots "
                      << ts.scratch_slots;
            work = ts.two_paths_walked; bytes = ts.algorithmic_bytes;
        } else {
            std::cout << "SIM pairs: " << ps.pairs << " pairs, short / wave / wg " << ps.pairs_short << " / " << ps.pairs_wave << " / " << ps.pairs_wg << ", elements_examined "
                      << ps.elements_examined << ", common_total " << ps.common_total;
            work = ps.elements_examined; bytes = ps.algorithmic_bytes;
        }
        std::cout << ", " << tm.get_time() * 1000.0 << " ms, prepare " << prepare_s * 1000.0 << " ms, " << bytes << " bytes of the model, " << bytes / (tm.get_time() * 1e9) << " GB/s"
                  << std::endl;
        performance_stats.print_algorithm_performance_stats(w.topk ? "SIM top-k (fused)" : "SIM pairs (fused)", tm.get_time(), work);
        return performance_stats.get_algorithm_performance(tm.get_time(), work);
    }

    // launches per timing slot of one more (untimed) run with the event brackets on
    static void print_launches(VGL_Graph &graph, Work &w)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        run(graph, w, nullptr, nullptr);
        int64_t total = 0;
        std::cout << "SIM launches:";
        const std::vector<const char *> names = w.topk ? std::vector<const char *>{"sim_classify", "sim_publish", "sim_topk_small", "sim_topk_table", "sim_topk_global"}
                                                       : std::vector<const char *>{"sim_classify", "sim_publish", "sim_pairs_short", "sim_pairs_wave", "sim_pairs_wg"};
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
    struct HostSimple {                                              // the simple undirected graph: rows ascending, no duplicates, no loops
        std::vector<long long> ptr;
        std::vector<int> adj;
        int deg(int v) const { return (int)(ptr[(size_t)v + 1] - ptr[(size_t)v]); }
    };
    static HostSimple host_simple(const HostCSR &g)
    {
        std::vector<std::pair<int, int>> all;
        all.reserve(2 * g.adj.size());
        for (int u = 0; u < g.V; u++)
            for (long long p = g.rowptr[(size_t)u]; p < g.rowptr[(size_t)u + 1]; p++) {
                const int v = g.adj[(size_t)p];
                if (v != u) { all.emplace_back(u, v); all.emplace_back(v, u); }
            }
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        HostSimple s;
        s.ptr.assign((size_t)g.V + 1, 0);
        s.adj.resize(all.size());
        for (size_t i = 0; i < all.size(); i++) { s.ptr[(size_t)all[i].first + 1]++; s.adj[i] = all[i].second; }
        for (int v = 0; v < g.V; v++) s.ptr[(size_t)v + 1] += s.ptr[(size_t)v];
        return s;
    }
    // the undirected edges lo < hi, ascending (lo, hi): the library's edge numbering
    static void host_edges(const HostSimple &s, std::vector<int> &eu, std::vector<int> &ev)
    {
        const int V = (int)s.ptr.size() - 1;
        for (int u = 0; u < V; u++)
            for (long long p = s.ptr[(size_t)u]; p < s.ptr[(size_t)u + 1]; p++)
                if (s.adj[(size_t)p] > u) { eu.push_back(u); ev.push_back(s.adj[(size_t)p]); }
    }
    static int seq_common(const HostSimple &s, int u, int v)
    {
        long long a = s.ptr[(size_t)u], b = s.ptr[(size_t)v];
        const long long ae = s.ptr[(size_t)u + 1], be = s.ptr[(size_t)v + 1];
        int c = 0;
        while (a < ae && b < be) {
            const int x = s.adj[(size_t)a], y = s.adj[(size_t)b];
            if (x == y) { c++; a++; b++; }
            else if (x < y) a++;
            else b++;
        }
        return c;
    }
    struct Cand { long long num, den; int label, id; };
    // row `u` of the top-k: ids and counts, padded; cnt: V zeros on entry and on return
    static void seq_topk(const HostSimple &s, int u, int metric, int k, bool include, const std::vector<int> &label, std::vector<int> &cnt, int *ids, int *common)
    {
        std::vector<int> touched;
        for (long long p = s.ptr[(size_t)u]; p < s.ptr[(size_t)u + 1]; p++) {
            const int v = s.adj[(size_t)p];
            for (long long q = s.ptr[(size_t)v]; q < s.ptr[(size_t)v + 1]; q++) {
                const int w = s.adj[(size_t)q];
                if (cnt[(size_t)w]++ == 0) touched.push_back(w);
            }
        }
        std::vector<Cand> cand;
        const int du = s.deg(u);
        for (int w : touched) {
            const int c = cnt[(size_t)w];
            cnt[(size_t)w] = 0;
            if (w == u) continue;
            if (!include && std::binary_search(s.adj.begin() + s.ptr[(size_t)u], s.adj.begin() + s.ptr[(size_t)u + 1], w)) continue;
            const int dw = s.deg(w);
            const long long den = metric == VGL_HIP_SIM_COMMON ? 1 : metric == VGL_HIP_SIM_JACCARD ? (long long)du + dw - c : std::min(du, dw);
            cand.push_back(Cand{c, den, label[(size_t)w], w});
        }
        std::sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) {
            const long long l = a.num * b.den, r = b.num * a.den;
            return l > r || (l == r && a.label < b.label);
        });
        for (int j = 0; j < k; j++) {
            const bool have = (size_t)j < cand.size();
            ids[j] = have ? cand[(size_t)j].id : -1;
            common[j] = have ? (int)cand[(size_t)j].num : 0;
        }
    }
};
