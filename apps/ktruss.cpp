// ktruss app: k-truss decomposition (truss number of every edge) of the simple undirected graph underlying the stored edges; heat run + timed run.
// The edge numbering (and the symmetric simple CSR under it) is prepared outside the timing.
//   -klimit K        stop the peel at K (>= 2): the dump holds min(truss, K)
//   -check           compare the truss numbers with a sequential host peel (its time is printed: the yardstick of the GPU numbers)
//   -dump FILE       E' int32 triples (lo, hi, truss) in ORIGINAL vertex ids, ascending by (lo, hi)
#define INT_ELEMENTS_PER_EDGE 1.0      // the walked adjacency entry
#include "common.hpp"
#include "algorithms/ktruss.hpp"
#include <array>
int main(int argc, char **argv)
{
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        if (!parser.fused) throw "ktruss: only the fused path exists (pass -fused)";
        if (parser.k_limit < 0 || parser.k_limit == 1) throw "ktruss: -klimit must be 0 or at least 2";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        {
            KTruss::Edges edges;
            const double prep = KTruss::prepare(graph, edges);
            KTruss::hip_fused(graph, edges, parser.k_limit, prep);                                     // heat run
            const double perf = KTruss::hip_fused(graph, edges, parser.k_limit, prep);                 // timed
            KTruss::print_launches(graph, edges, parser.k_limit);
            report_performance(perf);
            const std::vector<int> eu = edges.host(edges.u), ev = edges.host(edges.v), truss = edges.host(edges.truss);
            if (parser.get_check_flag()) {
                HostCSR h(graph);
                std::vector<long long> rowptr;
                std::vector<int> adj, want_u, want_v;
                KCore::simple_graph(h, rowptr, adj);
                for (size_t v = 0; v + 1 < rowptr.size(); v++) std::sort(adj.begin() + rowptr[v], adj.begin() + rowptr[v + 1]);
                Timer tm;
                tm.start();
                const std::vector<int> want = KTruss::seq_truss_numbers(rowptr, adj, parser.k_limit, want_u, want_v);
                tm.end();
                std::cout << "KTRUSS host peel (sequential): " << tm.get_time() * 1000.0 << " ms" << std::endl;
                if (truss.size() != want.size() || eu != want_u || ev != want_v) {
                    std::cout << "the edge numbering differs from the host's" << std::endl;
                    std::cout << "error count: " << std::max<size_t>(1, std::max(truss.size(), want.size())) << std::endl;
                } else
                    verify_results(truss, want);
            }
            if (!parser.dump.empty()) {
                std::vector<std::array<int, 3>> rows(truss.size());
                for (size_t i = 0; i < rows.size(); i++) {
                    const int a = graph.reorder(eu[i], SCATTER, ORIGINAL), b = graph.reorder(ev[i], SCATTER, ORIGINAL);
                    rows[i] = {std::min(a, b), std::max(a, b), truss[i]};
                }
                std::sort(rows.begin(), rows.end());
                std::vector<int> flat;
                flat.reserve(rows.size() * 3);
                for (const auto &r : rows) flat.insert(flat.end(), r.begin(), r.end());
                dump_array(parser.dump, flat);
            }
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return 0;
}
