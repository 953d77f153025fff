// Biconnectivity: the fused HIP path (vgl_hip_bicc_run, the contract of include/vgl_hip.h) and a sequential host restatement of that contract for
// -check: Hopcroft and Tarjan's depth-first search with lowpoints and an edge stack, iterative (a path of 2^24 vertices must not overflow the host
// stack), with the labels made canonical as the library's are.  The reference has no biconnectivity.
#pragma once
#include <algorithm>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

struct BICC {
    // device arrays in the library's edge numbering (ascending (lo, hi) of the graph's own vertex ids) and per vertex
    struct Result {
        long long n = 0;
        int V = 0;
        int *u = nullptr, *v = nullptr, *block = nullptr, *two_edge = nullptr;
        unsigned char *bridge = nullptr, *articulation = nullptr;
        ~Result()
        {
            MemoryAPI::free_device_array(u); MemoryAPI::free_device_array(v); MemoryAPI::free_device_array(block); MemoryAPI::free_device_array(two_edge);
            MemoryAPI::free_device_array(bridge); MemoryAPI::free_device_array(articulation);
        }
        template <class T>
        std::vector<T> host(const T *d, long long count) const
        {
            std::vector<T> h((size_t)count);
            if (count) VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), h.data(), d, sizeof(T) * (size_t)count));
            return h;
        }
    };
    // what the host restatement computes
    struct Host {
        std::vector<int> u, v, block, two_edge;
        std::vector<unsigned char> bridge, articulation;
    };

    // the edge numbering (and the symmetric CSR under it): outside the timing of the runs; allocates the result arrays
    static double prepare(VGL_Graph &graph, Result &r)
    {
        Timer prep;
        prep.start();
        int64_t n = 0;
        VGL_HIP_CALL(vgl_hip_bicc_prepare(VGL_RUNTIME::ctx(), graph.get_handle(), &n));
        prep.end();
        r.n = n;
        r.V = graph.get_vertices_count();
        const size_t cap = (size_t)std::max<int64_t>(n, 1), vcap = (size_t)std::max(r.V, 1);
        MemoryAPI::allocate_device_array(&r.u, cap);
        MemoryAPI::allocate_device_array(&r.v, cap);
        MemoryAPI::allocate_device_array(&r.block, cap);
        MemoryAPI::allocate_device_array(&r.bridge, cap);
        MemoryAPI::allocate_device_array(&r.two_edge, vcap);
        MemoryAPI::allocate_device_array(&r.articulation, vcap);
        return prep.get_time();
    }

    static double hip_fused(VGL_Graph &graph, Result &r, double prepare_s, vgl_hip_bicc_stats *out = nullptr)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        vgl_hip_bicc_stats st;
        Timer tm;
        tm.start();
        VGL_HIP_CALL(vgl_hip_bicc_run(c, graph.get_handle(), r.u, r.v, r.bridge, r.block, r.articulation, r.two_edge, &st));
        tm.end();
        std::cout << "BICC: " << st.biconnected_components << " blocks (largest " << st.largest_component_edges << " edges), " << st.bridges << " bridges, " << st.articulation_points
                  << " cut vertices, " << st.two_edge_components << " 2-edge-connected components, " << st.components << " components, depth " << st.depth << ", " << st.undirected_edges
                  << " undirected edges, " << tm.get_time() * 1000.0 << " ms, prepare " << prepare_s * 1000.0 << " ms, " << st.algorithmic_bytes / (tm.get_time() * 1e9)
                  << " GB/s of the bytes model" << std::endl;
        if (out) *out = st;
        performance_stats.print_algorithm_performance_stats("BICC (fused)", tm.get_time(), 2 * st.undirected_edges);
        return performance_stats.get_algorithm_performance(tm.get_time(), 2 * st.undirected_edges);
    }

    // launches per timing slot of one more (untimed) run with the event brackets on
    static void print_launches(VGL_Graph &graph, Result &r)
    {
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        VGL_HIP_CALL(vgl_hip_timing_reset(c));
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
        VGL_HIP_CALL(vgl_hip_bicc_run(c, graph.get_handle(), r.u, r.v, r.bridge, r.block, r.articulation, r.two_edge, nullptr));
        int64_t total = 0;
        std::cout << "BICC launches:";
        for (const char *name : {"bicc_classify", "bicc_roots", "bicc_seed", "bicc_bfs_short", "bicc_bfs_wave", "bicc_bfs_wg", "bicc_publish", "bicc_size", "bicc_pre", "bicc_local_short",
                                 "bicc_local_wave", "bicc_local_wg", "bicc_lowhigh", "bicc_reset", "bicc_edge", "bicc_flatten", "bicc_block", "bicc_art_short", "bicc_art_wave", "bicc_art_wg", "bicc_twoecc"}) {
            int64_t n = 0;
            double ms = 0.0;
            VGL_HIP_CALL(vgl_hip_timing_get(c, name, &n, &ms));
            std::cout << " " << name << " " << n << " (" << ms << " ms)";
            total += n;
        }
        std::cout << ", total " << total << std::endl;
        VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
    }

    // The contract on the host.  g: the stored outgoing CSR.  The undirected edges in the library's numbering, the symmetric rows with the edge of
    // every slot, then one depth-first search per component with an explicit stack of (vertex, entering edge, next slot) and a stack of edges.
    static Host seq_hopcroft_tarjan(const HostCSR &g)
    {
        Host h;
        const int V = g.V;
        std::vector<std::pair<int, int>> all;
        all.reserve(g.adj.size());
        for (int u = 0; u < V; u++)
            for (long long p = g.rowptr[(size_t)u]; p < g.rowptr[(size_t)u + 1]; p++) {
                const int v = g.adj[(size_t)p];
                if (v != u) all.emplace_back(std::min(u, v), std::max(u, v));
            }
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        const size_t E = all.size();
        h.u.resize(E); h.v.resize(E);
        std::vector<long long> ptr((size_t)V + 1, 0);
        for (size_t e = 0; e < E; e++) {
            h.u[e] = all[e].first; h.v[e] = all[e].second;
            ptr[(size_t)all[e].first + 1]++; ptr[(size_t)all[e].second + 1]++;
        }
        for (int v = 0; v < V; v++) ptr[(size_t)v + 1] += ptr[(size_t)v];
        std::vector<int> adj(2 * E), eid(2 * E);
        {
            std::vector<long long> at(ptr.begin(), ptr.end() - 1);
            for (size_t e = 0; e < E; e++) {
                const int a = all[e].first, b = all[e].second;
                adj[(size_t)at[(size_t)a]] = b; eid[(size_t)at[(size_t)a]++] = (int)e;
                adj[(size_t)at[(size_t)b]] = a; eid[(size_t)at[(size_t)b]++] = (int)e;
            }
        }
        h.block.assign(E, -1);
        h.bridge.assign(E, 0);
        h.articulation.assign((size_t)V, 0);
        std::vector<int> disc((size_t)V, -1), low((size_t)V, 0), estack, members;
        struct frame { int v, pe; long long at; };
        std::vector<frame> stack;
        int clock = 0;
        for (int root = 0; root < V; root++) {
            if (disc[(size_t)root] >= 0) continue;
            disc[(size_t)root] = low[(size_t)root] = clock++;
            int root_children = 0;
            stack.push_back(frame{root, -1, ptr[(size_t)root]});
            while (!stack.empty()) {
                frame &f = stack.back();
                const int v = f.v;
                if (f.at < ptr[(size_t)v + 1]) {
                    const int w = adj[(size_t)f.at], e = eid[(size_t)f.at];
                    f.at++;
                    if (e == f.pe) continue;
                    if (disc[(size_t)w] < 0) {
                        disc[(size_t)w] = low[(size_t)w] = clock++;
                        estack.push_back(e);
                        if (v == root) root_children++;
                        stack.push_back(frame{w, e, ptr[(size_t)w]});      // (f is void from here on)
                    } else if (disc[(size_t)w] < disc[(size_t)v]) {       // a back edge, seen from its lower end
                        estack.push_back(e);
                        low[(size_t)v] = std::min(low[(size_t)v], disc[(size_t)w]);
                    }
                    continue;
                }
                const int pe = f.pe;
                stack.pop_back();
                if (stack.empty()) break;
                const int u = stack.back().v;
                low[(size_t)u] = std::min(low[(size_t)u], low[(size_t)v]);
                if (low[(size_t)v] >= disc[(size_t)u]) {                  // u separates the subtree of v: the edges above (u, v) are one block
                    if (u != root) h.articulation[(size_t)u] = 1;
                    members.clear();
                    int name = pe;
                    for (;;) {
                        const int e = estack.back();
                        estack.pop_back();
                        members.push_back(e);
                        name = std::min(name, e);
                        if (e == pe) break;
                    }
                    for (int e : members) h.block[(size_t)e] = name;
                }
                if (low[(size_t)v] > disc[(size_t)u]) h.bridge[(size_t)pe] = 1;
            }
            if (root_children >= 2) h.articulation[(size_t)root] = 1;
        }
        // the 2-edge-connected components: a union-find over the edges that are no bridges, the smaller root on top
        std::vector<int> parent((size_t)V);
        std::iota(parent.begin(), parent.end(), 0);
        auto find = [&](int x) {
            while (parent[(size_t)x] != x) { parent[(size_t)x] = parent[(size_t)parent[(size_t)x]]; x = parent[(size_t)x]; }
            return x;
        };
        for (size_t e = 0; e < E; e++) {
            if (h.bridge[e]) continue;
            const int a = find(h.u[e]), b = find(h.v[e]);
            if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
        }
        h.two_edge.resize((size_t)V);
        for (int v = 0; v < V; v++) h.two_edge[(size_t)v] = find(v);
        return h;
    }
};
