// lp app: label propagation (the reference's algorithms/lp, AlwaysActive GPU path), heat run + timed run.
//   -it N            maximum iterations (default 20, lp.h:10)
//   -all-active      every row every iteration; -partial-active: only the rows whose neighbours changed; default: the library's AUTO
//   -check           compare with the host restatement of the contract;  -dump FILE: int32 labels in ORIGINAL vertex order
#define INT_ELEMENTS_PER_EDGE 2.0      // adjacency entry + gathered label
#include "common.hpp"
#include "algorithms/lp.hpp"
#include <cstring>
int main(int argc, char **argv)
{
    try {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        int max_iterations = LP_DEFAULT_MAX_ITERATIONS, mode = VGL_LP_AUTO;
        for (int i = 1; i < argc; i++) {          // the parser's defaults (1 round, all-active) are those of the other apps
            if (!strcmp(argv[i], "-it")) max_iterations = parser.get_number_of_rounds();
            else if (!strcmp(argv[i], "-all-active")) mode = VGL_LP_ALL_ACTIVE;
            else if (!strcmp(argv[i], "-partial-active")) mode = VGL_LP_FRONTIER;
        }
        if (!parser.fused) throw "lp: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        VerticesArray<int> labels(graph);
        LabelPropagation::hip_fused(graph, labels, max_iterations, mode);           // heat run
        report_performance(LabelPropagation::hip_fused(graph, labels, max_iterations, mode));
        if (parser.get_check_flag()) {
            HostCSR h(graph);
            std::vector<int> init((size_t)h.V);
            if (graph.is_renumbered())
                VGL_HIP_CALL(vgl_hip_memcpy_d2h(VGL_RUNTIME::ctx(), init.data(), graph.get_backward_conversion(), sizeof(int) * init.size()));
            else
                for (int v = 0; v < h.V; v++) init[(size_t)v] = v;
            verify_results(labels.to_host(), LabelPropagation::seq_label_propagation(h, init, max_iterations));
        }
        labels.reorder(ORIGINAL);
        dump_array(parser.dump, labels.to_host());
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return 0;
}
