// bicc app: bridges, cut vertices, biconnected components (blocks) and 2-edge-connected components of the simple undirected graph underlying the
// stored edges; heat run + timed run.  The edge numbering (and the symmetric simple CSR under it) is prepared outside the timing.
//   -check           compare all outputs with a sequential host Hopcroft-Tarjan (its time is printed: the yardstick of the GPU numbers)
//   -dump FILE       E' records (int32 lo, int32 hi, int32 block, int32 bridge) in ORIGINAL vertex ids, ascending by (lo, hi); the block of an edge
//                    is named by the smallest record index of an edge of that block
#define INT_ELEMENTS_PER_EDGE 2.0      // the walked adjacency entry and one word of its far end
#include "common.hpp"
#include "algorithms/bicc.hpp"
#include <array>
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        if (!parser.fused) throw "bicc: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        {
            BICC::Result r;
            const double prep = BICC::prepare(graph, r);
            vgl_hip_bicc_stats st;
            BICC::hip_fused(graph, r, prep);                                                           // heat run
            const double perf = BICC::hip_fused(graph, r, prep, &st);                                  // timed
            BICC::print_launches(graph, r);
            report_performance(perf);
            const std::vector<int> eu = r.host(r.u, r.n), ev = r.host(r.v, r.n), block = r.host(r.block, r.n), two_edge = r.host(r.two_edge, r.V);
            const std::vector<unsigned char> bridge = r.host(r.bridge, r.n), articulation = r.host(r.articulation, r.V);
            if (parser.get_check_flag()) {
                HostCSR h(graph);
                Timer tm;
                tm.start();
                const BICC::Host want = BICC::seq_hopcroft_tarjan(h);
                tm.end();
                std::cout << "BICC host Hopcroft-Tarjan (sequential, edge list + depth-first search + union-find): " << tm.get_time() * 1000.0 << " ms" << std::endl;
                if (want.u != eu || want.v != ev) {
                    std::cout << "the edge numbering differs from the host's" << std::endl;
                    errors = (int)std::max<size_t>(1, std::max(eu.size(), want.u.size()));
                    std::cout << "error count: " << errors << std::endl;
                } else {
                    size_t bad = 0;
                    auto differ = [&](const char *what, size_t i, long long a, long long b) {
                        if (bad++ < 10) std::cout << "error in " << what << " at " << i << ": " << a << " vs " << b << std::endl;
                    };
                    for (size_t i = 0; i < eu.size(); i++) {
                        if (bridge[i] != want.bridge[i]) differ("bridge", i, bridge[i], want.bridge[i]);
                        if (block[i] != want.block[i]) differ("block", i, block[i], want.block[i]);
                    }
                    for (size_t v = 0; v < articulation.size(); v++) {
                        if (articulation[v] != want.articulation[v]) differ("articulation", v, articulation[v], want.articulation[v]);
                        if (two_edge[v] != want.two_edge[v]) differ("two_edge_component", v, two_edge[v], want.two_edge[v]);
                    }
                    errors = (int)std::min<size_t>(bad, 1u << 30);
                    std::cout << "error count: " << errors << std::endl;
                }
            }
            if (!parser.dump.empty()) {
                std::vector<std::array<int, 4>> rows(eu.size());
                for (size_t i = 0; i < eu.size(); i++) {
                    const int a = graph.reorder(eu[i], SCATTER, ORIGINAL), b = graph.reorder(ev[i], SCATTER, ORIGINAL);
                    rows[i] = {std::min(a, b), std::max(a, b), block[i], (int)bridge[i]};
                }
                std::sort(rows.begin(), rows.end());
                std::vector<int> first(rows.size(), (int)rows.size());                                 // the smallest record index of every block
                for (size_t i = 0; i < rows.size(); i++) first[(size_t)rows[i][2]] = std::min(first[(size_t)rows[i][2]], (int)i);
                std::vector<int> flat;
                flat.reserve(rows.size() * 4);
                for (const auto &row : rows) { flat.push_back(row[0]); flat.push_back(row[1]); flat.push_back(first[(size_t)row[2]]); flat.push_back(row[3]); }
                dump_array(parser.dump, flat);
            }
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors ? 1 : 0;
}
