// closeness app: bit-parallel multi-source BFS from K sources and the per-source sums of closeness, harmonic centrality and eccentricity; heat run +
// timed run.  The row classes are prepared outside the timing.
//   -sources K       the first K vertices (ORIGINAL ids) with outgoing edges are the sources (default 64: one batch)
//   -in              distances along incoming entries (the distance TO the source: networkx's closeness on a directed graph); default: outgoing
//   -check           compare reached, dist_sum, ecc and harmonic (bit for bit) with a sequential host BFS per source; exit status 1 on a difference
//   -dump FILE       K records (int64 reached, int64 dist_sum, int32 ecc, int32 pad, float64 harmonic) in source order
#define INT_ELEMENTS_PER_EDGE 3.0      // one adjacency entry and one 8-byte word of its far end per entry walked
#include "common.hpp"
#include "algorithms/closeness.hpp"
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        if (!parser.fused) throw "closeness: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        const size_t V = (size_t)graph.get_vertices_count();
        const int K = parser.sources_given ? parser.sources : 64;
        const int direction = parser.incoming ? 1 : 0;
        std::vector<int> sources;                                                     // in the graph's own numbering
        for (int v = 0; v < (int)V && (int)sources.size() < K; v++) {
            const int stored = graph.reorder(v, ORIGINAL, SCATTER);
            if (graph.get_outgoing_connections_count(stored) > 0) sources.push_back(stored);
        }
        std::vector<CLOSENESS::Record> got;
        CLOSENESS::hip_fused(graph, std::vector<int>(sources.begin(), sources.begin() + std::min<size_t>(sources.size(), 1)), direction, got);      // heat run (builds the classes)
        const double perf = CLOSENESS::hip_fused(graph, sources, direction, got);     // timed
        report_performance(perf);
        if (parser.get_check_flag()) {
            HostCSR h(graph, direction ? GATHER : SCATTER);
            errors = CLOSENESS::verify(got, CLOSENESS::seq_bfs_sums(h, sources));
        }
        dump_array(parser.dump, got);
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors > 0 ? 1 : 0;
}
