// agg app: neighbour aggregation of a V x F float32 feature matrix over a stored direction of the graph; plan, heat run + timed run.
//   -features F      columns (default 64)
//   -op NAME         sum | mean | max | min (default sum)
//   -weighted        one float32 weight per entry (sum and mean)
//   -out             aggregate over the outgoing entries (default: the incoming direction)
//   -backward        also the transposed run on a gradient of the same shape; the transpose build is timed apart
//   -check           compare with the sequential host restatement in float64 within the derived bound, the arg for equality; exit status 1 on a difference
//   -dump FILE       n_rows x F float32, the forward result in the graph's own row order
#define INT_ELEMENTS_PER_EDGE 2.0      // one adjacency entry and (per column) one 4-byte value of its far end per entry walked
#include "common.hpp"
#include "algorithms/agg.hpp"
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        VGL_RUNTIME::init_library(argc, argv);
        // the options of this app alone are taken out before the shared parser sees the rest
        AGG::Options opt;
        std::vector<char *> rest{argv[0]};
        for (int i = 1; i < argc; i++) {
            const std::string a = argv[i];
            if (a == "-features" || a == "-op") {
                if (i + 1 >= argc) throw "missing value for command line option";
                const std::string v = argv[++i];
                if (a == "-features") opt.features = atoi(v.c_str());
                else if (v == "sum") opt.op = VGL_HIP_AGG_SUM;
                else if (v == "mean") opt.op = VGL_HIP_AGG_MEAN;
                else if (v == "max") opt.op = VGL_HIP_AGG_MAX;
                else if (v == "min") opt.op = VGL_HIP_AGG_MIN;
                else throw "agg: unknown value for -op (sum, mean, max or min)";
            } else if (a == "-weighted") opt.weighted = true;
            else if (a == "-out") opt.outgoing = true;
            else if (a == "-backward") opt.backward = true;
            else rest.push_back(argv[i]);
        }
        if (opt.features < 1) throw "agg: -features must be at least 1";
        if (opt.weighted && (opt.op == VGL_HIP_AGG_MAX || opt.op == VGL_HIP_AGG_MIN)) throw "agg: max and min take no weights";
        Parser parser;
        parser.parse_args((int)rest.size(), rest.data());
        if (!parser.fused) throw "agg: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        const TraversalDirection dir = opt.outgoing ? SCATTER : GATHER;
        const vgl_csr_view view = graph.get_direction_view(dir);
        {
            AGG::Inputs in(graph, view, opt, parser.seed);                              // (freed before the library is finalised)
            AGG::Result r;
            const double perf = AGG::hip_fused(view, in, opt, r);
            report_performance(perf);
            AGG::print_launches(view, in, opt);
            if (parser.get_check_flag()) {
                HostCSR host(graph, dir);
                errors = AGG::verify(host, in, opt, r);
            }
            if (!parser.dump.empty()) dump_array(parser.dump, r.out);
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors > 0 ? 1 : 0;
}
