// attn app: edge scores, edge softmax and dot-product graph attention of V x F float32 features over a stored direction of the graph; plan, every
// call of the stage once to heat and once timed.
//   -features F      columns (default 64)
//   -heads H         H heads in one walk: the heads form of every call, head h on the columns [h F / H, (h + 1) F / H); H must divide F (default: the
//                    single-head calls)
//   -stage NAME      dot | softmax | attention (default attention: dot, softmax, weighted sum)
//   -out             over the outgoing entries (default: the incoming direction)
//   -backward        also the gradients of the stage; the transpose build is timed apart
//   -score NAME      dot | add (default dot).  add: the additive score of GAT, leaky_relu(a[row] + b[adj]) from two V x H terms, in place of the dot
//                    product in the stages dot and attention; its gradients are the two entry sums
//   -slope X         the negative slope of -score add (default 0.2; not negative)
//   -check           compare every stage with the sequential host restatement in float64 within the derived bounds; exit status 1 on a difference
//   -dump FILE       float32: the forward result of the stage (e, the weights, or n_rows x F) in the graph's own order
#define INT_ELEMENTS_PER_EDGE 2.0      // one adjacency entry and (per column) one 4-byte value of its far end per entry walked
#include "common.hpp"
#include "algorithms/attn.hpp"
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        VGL_RUNTIME::init_library(argc, argv);
        // the options of this app alone are taken out before the shared parser sees the rest
        ATTN::Options opt;
        std::vector<char *> rest{argv[0]};
        for (int i = 1; i < argc; i++) {
            const std::string a = argv[i];
            if (a == "-features" || a == "-stage" || a == "-heads" || a == "-score" || a == "-slope") {
                if (i + 1 >= argc) throw "missing value for command line option";
                const std::string v = argv[++i];
                if (a == "-features") opt.features = atoi(v.c_str());
                else if (a == "-heads") { opt.heads = atoi(v.c_str()); opt.use_heads = true; }
                else if (a == "-slope") opt.slope = (float)atof(v.c_str());
                else if (a == "-score") {
                    if (v != "dot" && v != "add") throw "attn: unknown value for -score (dot or add)";
                    opt.score_add = v == "add";
                }
                else if (v == "dot") opt.stage = ATTN::DOT;
                else if (v == "softmax") opt.stage = ATTN::SOFTMAX;
                else if (v == "attention") opt.stage = ATTN::ATTENTION;
                else throw "attn: unknown value for -stage (dot, softmax or attention)";
            } else if (a == "-out") opt.outgoing = true;
            else if (a == "-backward") opt.backward = true;
            else rest.push_back(argv[i]);
        }
        if (opt.features < 1) throw "attn: -features must be at least 1";
        if (opt.heads < 1) throw "attn: -heads must be at least 1";
        if (opt.features % opt.heads != 0) throw "attn: -heads must divide -features";
        if (!(opt.slope >= 0.0f) || std::isinf(opt.slope)) throw "attn: -slope must be a finite number that is not negative";
        Parser parser;
        parser.parse_args((int)rest.size(), rest.data());
        if (!parser.fused) throw "attn: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        const TraversalDirection dir = opt.outgoing ? SCATTER : GATHER;
        const vgl_csr_view view = graph.get_direction_view(dir);
        {
            ATTN::Inputs in(graph, view, opt, parser.seed);                             // (freed before the library is finalised)
            ATTN::Result r;
            const double perf = ATTN::hip_fused(view, in, opt, r);
            report_performance(perf);
            ATTN::print_launches(view, in, opt);
            if (parser.get_check_flag()) {
                HostCSR host(graph, dir);
                errors = ATTN::verify(host, in, opt, r);
            }
            if (!parser.dump.empty()) dump_array(parser.dump, opt.stage == ATTN::DOT ? r.e : opt.stage == ATTN::SOFTMAX ? r.w : r.out);
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors > 0 ? 1 : 0;
}
