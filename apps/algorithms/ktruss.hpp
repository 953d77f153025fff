// k-truss decomposition: the fused HIP path (vgl_hip_ktruss_run, the contract of include/vgl_hip.h) and a sequential host restatement of that contract
// for -check (supports by intersection, edges bucket-sorted by support, every removed edge intersects its two rows: Wang & Cheng's peel).  The
// reference has no k-truss.
#pragma once
#include <algorithm>
#include <vector>
#include "kcore.hpp"

struct KTruss {
    // device arrays of E' int32 each, in the library's edge numbering (ascending (lo, hi) of the graph's own vertex ids)
    struct Edges {
        long long n = 0;
        int *u = nullptr, *v = nullptr, *truss = nullptr;
        ~Edges() { MemoryAPI::free_device_array(u); MemoryAPI::free_device_array(v); MemoryAPI::free_device_array(truss); }
        std::vector<int> host(const int *d) const
        {
            std::vector<int> h((size_t)n);
            if (n) VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), d, sizeof(int) * (size_t)n));
            return h;
        }
    };

    // the edge numbering (and the symmetric simple CSR under it): outside the timing of the runs; allocates the result arrays
    static double prepare(VGL_Graph &graph, Edges &e)
    {
        Timer prep;
        prep.start();
        int64_t n = 0;
        VGL_HIP_CALL(vgl_hip_ktruss_prepare(VGL_RUNTIME::ctx(), graph.get_handle(), &n));
        prep.end();
        e.n = n;
        const size_t cap = (size_t)std::max<int64_t>(n, 1);
        MemoryAPI::allocate_device_array(&e.u, cap);
        MemoryAPI::allocate_device_array(&e.v, cap);
        MemoryAPI::allocate_device_array(&e.truss, cap);
        return prep.get_time();
    }

    static double hip_fused(VGL_Graph &graph, Edges &e, int k_limit, double prepare_s, vgl_hip_ktruss_stats *out = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        vgl_hip_ktruss_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_ktruss_run(c, graph.get_handle(), k_limit, e.u, e.v, e.truss, nullptr, &st));
        tm.end();
        const long long walked = st.support_elements + st.peel_elements;
        std::cout << "KTRUSS: max truss " << st.max_truss << ", " << st.rounds << " rounds, " << st.sub_rounds << " sub-rounds, " << st.undirected_edges
                  << " undirected edges, " << st.triangles << " triangles, max support " << st.max_support << ", " << tm.get_time() * 1000.0 << " ms, prepare "
                  << prepare_s * 1000.0 << " ms, " << st.support_elements << " + " << st.peel_elements << " entries walked, "
                  << st.algorithmic_bytes / (tm.get_time() * 1e9) << " GB/s of the bytes model" << std::endl;
        if (out) *out = st;
        performance_stats.print_algorithm_performance_stats("KTRUSS (fused)", tm.get_time(), walked);
        return performance_stats.get_algorithm_performance(tm.get_time(), walked);
    }

    // launches per timing slot of one more (untimed) run with the event brackets on
    static void print_launches(VGL_Graph &graph, Edges &e, int k_limit)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        VGL_HIP_CALL(vgl_hip_ktruss_run(c, graph.get_handle(), k_limit, e.u, e.v, e.truss, nullptr, nullptr));
        int64_t total = 0;
        std::cout << "KTRUSS launches:";
        for (const char *name : {"ktruss_classify", "ktruss_sup_short", "ktruss_sup_wave", "ktruss_sup_wg", "ktruss_scan", "ktruss_short", "ktruss_wave", "ktruss_wg",
                                 "ktruss_publish"}) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    // The host peel.  rowptr / adj: the simple undirected graph, every row ascending.  Returns the truss numbers in the library's edge numbering
    // (min(truss, k_limit) when k_limit >= 2); eu / ev receive the endpoints.
    static std::vector<int> seq_truss_numbers(const std::vector<long long> &rowptr, const std::vector<int> &adj, int k_limit, std::vector<int> &eu, std::vector<int> &ev)
    {
        const size_t V = rowptr.size() - 1, E = adj.size() / 2;
        std::vector<int> eid(adj.size());
        eu.assign(E, 0); ev.assign(E, 0);
        auto find = [&](int row, int w) -> long long {                // the slot of w in row `row`, or -1
            const int *b = adj.data() + rowptr[(size_t)row], *e = adj.data() + rowptr[(size_t)row + 1];
            const int *p = std::lower_bound(b, e, w);
            return p != e && *p == w ? (long long)(p - adj.data()) : -1;
        };
        {
            int next = 0;
            for (size_t u = 0; u < V; u++)
                for (long long p = rowptr[u]; p < rowptr[u + 1]; p++)
                    if (adj[(size_t)p] > (int)u) { eu[(size_t)next] = (int)u; ev[(size_t)next] = adj[(size_t)p]; eid[(size_t)p] = next++; }
            for (size_t u = 0; u < V; u++)
                for (long long p = rowptr[u]; p < rowptr[u + 1]; p++)
                    if (adj[(size_t)p] < (int)u) eid[(size_t)p] = eid[(size_t)find(adj[(size_t)p], (int)u)];
        }
        // f(e2, e3) for every triangle of edge e: the shorter row is walked, the longer searched
        auto for_triangles = [&](int e, auto &&f) {
            int a = eu[(size_t)e], b = ev[(size_t)e];
            if (rowptr[(size_t)a + 1] - rowptr[(size_t)a] > rowptr[(size_t)b + 1] - rowptr[(size_t)b]) std::swap(a, b);
            for (long long p = rowptr[(size_t)a]; p < rowptr[(size_t)a + 1]; p++) {
                const long long q = find(b, adj[(size_t)p]);
                if (q >= 0) f(eid[(size_t)p], eid[(size_t)q]);
            }
        };
        std::vector<int> sup(E, 0), order(E), pos(E);
        int ms = 0;
        for (size_t e = 0; e < E; e++) {
            int t = 0;
            for_triangles((int)e, [&](int, int) { t++; });
            sup[e] = t;
            ms = std::max(ms, t);
        }
        std::vector<int> bin((size_t)ms + 2, 0);
        for (size_t e = 0; e < E; e++) bin[(size_t)sup[e] + 1]++;
        for (int d = 0; d <= ms; d++) bin[(size_t)d + 1] += bin[(size_t)d];          // bin[d] = first position of support d
        {
            std::vector<int> next(bin.begin(), bin.end() - 1);
            for (size_t e = 0; e < E; e++) { pos[e] = next[(size_t)sup[e]]++; order[(size_t)pos[e]] = (int)e; }
        }
        std::vector<char> gone(E, 0);
        auto lower = [&](int x, int floor) {                          // one triangle less for edge x, which stays at or above the removed edge's support
            if (sup[(size_t)x] <= floor) return;
            const int sx = sup[(size_t)x], px = pos[(size_t)x], pw = bin[(size_t)sx], w = order[(size_t)pw];
            if (x != w) { pos[(size_t)x] = pw; order[(size_t)px] = w; pos[(size_t)w] = px; order[(size_t)pw] = x; }
            bin[(size_t)sx]++;
            sup[(size_t)x]--;
        };
        for (size_t i = 0; i < E; i++) {
            const int e = order[i];
            for_triangles(e, [&](int e2, int e3) {
                if (gone[(size_t)e2] || gone[(size_t)e3]) return;
                lower(e2, sup[(size_t)e]);
                lower(e3, sup[(size_t)e]);
            });
            gone[(size_t)e] = 1;
        }
        std::vector<int> truss(E);                                    // what is left of an edge's support when it is taken, + 2
        for (size_t e = 0; e < E; e++) truss[e] = k_limit >= 2 ? std::min(sup[e] + 2, k_limit) : sup[e] + 2;
        return truss;
    }
};
