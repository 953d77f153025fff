// kcore app: k-core decomposition (core numbers, degeneracy) of the simple undirected graph underlying the stored edges; heat run + timed run.
// The symmetric simple CSR is prepared outside the timing.
//   -klimit K        stop the peel at K: the dump holds min(core, K)
//   -check           compare the core numbers with a sequential host bucket peel (its time is printed: the yardstick of the GPU numbers)
//   -dump FILE       int32 core numbers in ORIGINAL vertex order
#define INT_ELEMENTS_PER_EDGE 2.0      // adjacency entry + the neighbour's degree
#include "common.hpp"
#include "algorithms/kcore.hpp"
int main(int argc, char **argv)
{
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        if (!parser.fused) throw "kcore: only the fused path exists (pass -fused)";
        if (parser.k_limit < 0) throw "kcore: -klimit must not be negative";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        VerticesArray<int> core(graph);
        KCore::hip_fused(graph, core, parser.k_limit);                               // heat run (builds the symmetric CSR)
        const double perf = KCore::hip_fused(graph, core, parser.k_limit);           // timed
        KCore::print_launches(graph, core, parser.k_limit);
        report_performance(perf);
        if (parser.get_check_flag()) {
            HostCSR h(graph);
            std::vector<long long> rowptr;
            std::vector<int> adj;
            KCore::simple_graph(h, rowptr, adj);
            Timer tm;
            tm.start();
            const std::vector<int> want = KCore::seq_core_numbers(rowptr, adj, parser.k_limit);
            tm.end();
            std::cout << "KCORE host bucket peel (sequential): " << tm.get_time() * 1000.0 << " ms" << std::endl;
            verify_results(core.to_host(), want);
        }
        core.reorder(ORIGINAL);
        dump_array(parser.dump, core.to_host());
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return 0;
}
