// bc app: betweenness centrality (Brandes) of the stored directed graph from K sources; heat run + timed run.  The row classes are prepared outside
// the timing.
//   -sources K       the first K vertices (ORIGINAL ids) with outgoing edges are the sources (default 16); -source S: that one vertex instead
//   -check           compare with the sequential host Brandes of the same contract, within the tolerance of the tests
//   -dump FILE       float64 values in ORIGINAL vertex order
#define INT_ELEMENTS_PER_EDGE 2.0      // one adjacency entry and the level of its endpoint per entry walked
#include "common.hpp"
#include "algorithms/bc.hpp"
int main(int argc, char **argv)
{
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        if (!parser.fused) throw "bc: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const size_t V = (size_t)graph.get_vertices_count();
        std::vector<int> sources;                                                     // in the graph's own numbering
        if (parser.source >= 0) sources.push_back(graph.reorder(checked_vertex(graph, parser.source, "source"), ORIGINAL, SCATTER));
        else
            for (int v = 0; v < (int)V && (int)sources.size() < parser.sources; v++) {
                const int stored = graph.reorder(v, ORIGINAL, SCATTER);
                if (graph.get_outgoing_connections_count(stored) > 0) sources.push_back(stored);
            }
        void *d_bc = nullptr;
        VGL_HIP_CALL(vgl_hip_malloc(c, sizeof(double) * std::max<size_t>(V, 1), &d_bc));
        BC::hip_fused(graph, std::vector<int>(sources.begin(), sources.begin() + std::min<size_t>(sources.size(), 1)), (double *)d_bc);      // heat run (builds the classes)
        const double perf = BC::hip_fused(graph, sources, (double *)d_bc);            // timed
        report_performance(perf);
        std::vector<double> stored(V), original(V);
        VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, stored.data(), d_bc, sizeof(double) * V));
        VGL_HIP_CALL(vgl_hip_free(c, d_bc));
        if (parser.get_check_flag()) {
            HostCSR h(graph);
            int depth = 0;
            long long longest_row = 0;
            const std::vector<double> want = BC::seq_brandes(h, sources, &depth, &longest_row);
            BC::verify(stored, want, depth, longest_row, sources.size());
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
