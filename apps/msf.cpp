// msf app: minimum spanning forest of the simple undirected graph underlying the stored edges, with the random weights of the sssp app; heat run +
// timed run.  What is kept per graph (symmetric simple CSR, edge numbering, the edge of every stored entry) is prepared outside the timing.
//   -check           compare the forest with a sequential host Kruskal under (weight, edge id) (its time is printed: the yardstick of the GPU numbers)
//   -dump FILE       forest_edges records (int32 lo, int32 hi, float32 weight) in ORIGINAL vertex ids, ascending by (lo, hi)
#define INT_ELEMENTS_PER_EDGE 3.0      // the walked adjacency entry, its edge id, the far end's component
#include "common.hpp"
#include "algorithms/msf.hpp"
#include <array>
#include <tuple>
int main(int argc, char **argv)
{
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        if (!parser.fused) throw "msf: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        {
            EdgesArray<float> weights(graph);
            weights.set_all_random(MAX_WEIGHT);
            MSF::Edges edges;
            const double prep = MSF::prepare(graph, edges);
            vgl_hip_msf_stats st;
            MSF::hip_fused(graph, weights, edges, prep);                                               // heat run
            const double perf = MSF::hip_fused(graph, weights, edges, prep, &st);                      // timed
            MSF::print_launches(graph, weights, edges);
            report_performance(perf);
            const std::vector<int> eu = edges.host(edges.u), ev = edges.host(edges.v);
            const std::vector<float> ew = edges.host(edges.w);
            const std::vector<unsigned char> in_forest = edges.host(edges.in_forest);
            if (parser.get_check_flag()) {
                HostCSR h(graph);
                const std::vector<float> w = weights.outgoing_to_host();
                Timer tm;
                tm.start();
                const std::vector<MSF::HostEdge> want_edges = MSF::fold(h, w);
                double want_total = 0.0;
                const std::vector<unsigned char> want = MSF::seq_kruskal(h.V, want_edges, &want_total);
                tm.end();
                std::cout << "MSF host Kruskal (sequential, fold + sort + union-find): " << tm.get_time() * 1000.0 << " ms, total weight " << want_total << std::endl;
                bool same_edges = want_edges.size() == eu.size();
                for (size_t i = 0; same_edges && i < eu.size(); i++)
                    same_edges = eu[i] == want_edges[i].lo && ev[i] == want_edges[i].hi && std::memcmp(&ew[i], &want_edges[i].w, sizeof(float)) == 0;
                if (!same_edges) {
                    std::cout << "the edge numbering or the folded weights differ from the host's" << std::endl;
                    std::cout << "error count: " << std::max<size_t>(1, std::max(eu.size(), want_edges.size())) << std::endl;
                } else
                    verify_results(in_forest, want);                                                   // set equality of the forest
            }
            if (!parser.dump.empty()) {
                std::vector<std::tuple<int, int, float>> rows;
                for (size_t i = 0; i < in_forest.size(); i++) {
                    if (!in_forest[i]) continue;
                    const int a = graph.reorder(eu[i], SCATTER, ORIGINAL), b = graph.reorder(ev[i], SCATTER, ORIGINAL);
                    rows.emplace_back(std::min(a, b), std::max(a, b), ew[i]);
                }
                std::sort(rows.begin(), rows.end());
                std::vector<int> flat;
                flat.reserve(rows.size() * 3);
                for (const auto &r : rows) {
                    int bits;
                    std::memcpy(&bits, &std::get<2>(r), sizeof(bits));
                    flat.push_back(std::get<0>(r)); flat.push_back(std::get<1>(r)); flat.push_back(bits);
                }
                dump_array(parser.dump, flat);
            }
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return 0;
}
