// tri app: triangle counting (global count and per-vertex counts) on the simple undirected graph underlying the stored edges; heat run + timed runs.
// (`tc` is transitive closure; this is `tri`.)  The oriented CSR is prepared outside the timing.
//   -check           compare the count and the per-vertex counts with the sequential host restatement of the contract
//   -dump FILE       int64 per-vertex counts in ORIGINAL vertex order
#define INT_ELEMENTS_PER_EDGE 1.0      // one adjacency entry per examined element
#include "common.hpp"
#include "algorithms/tri.hpp"
int main(int argc, char **argv)
{
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        if (!parser.fused) throw "tri: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const size_t V = (size_t)graph.get_vertices_count();
        void *d_pv = nullptr;
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(long long) * std::max<size_t>(V, 1), &d_pv));
        long long count_only = 0, triangles = 0;
        TriangleCount::hip_fused(graph, nullptr, &count_only);                       // heat run (builds the oriented CSR)
        TriangleCount::hip_fused(graph, nullptr, &count_only);                       // timed: count only
        const double perf = TriangleCount::hip_fused(graph, (long long *)d_pv, &triangles);      // timed: count + per-vertex
        report_performance(perf);
        std::vector<long long> stored(V), original(V);
        VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, stored.data(), d_pv, sizeof(long long) * V));
        VGL_HIP_CALL(vgl_hip_free(c, d_pv));
        if (parser.get_check_flag()) {
            HostCSR h(graph);
            std::vector<long long> want;
            const long long t = TriangleCount::seq_triangle_count(h, want);
            verify_results(std::vector<long long>{triangles, count_only}, std::vector<long long>{t, t});
            verify_results(stored, want);
        }
        if (graph.is_renumbered()) {                                                  // 8-byte values: the 4-byte device reorder does not apply
            std::vector<int> bwd(V);
            VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, bwd.data(), graph.get_backward_conversion(), sizeof(int) * V));
            for (size_t s = 0; s < V; s++) original[(size_t)bwd[s]] = stored[s];
        } else original = stored;
        dump_array(parser.dump, original);
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return 0;
}
