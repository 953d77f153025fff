// ppr app: batched personalised PageRank from K single-vertex seed sets; heat run + timed run.  The class lists are prepared outside the timing.
//   -sources K       the first K vertices (ORIGINAL ids) with an outgoing entry, one seed each (default 16: one batch)
//   -alpha A         the damping (default 0.85)
//   -iters N         exactly N iterations per batch (default 20), or with -tol: at most N (default 1000)
//   -tol T           stop a batch once its largest err is <= T
//   -check           compare with the sequential host restatement of the contract within the derived tolerance; exit status 1 on a difference
//   -dump FILE       K x V float64, every row in ORIGINAL vertex order
#define INT_ELEMENTS_PER_EDGE 3.0      // one adjacency entry and one 8-byte value of its far end per entry walked and column
#include "common.hpp"
#include "algorithms/ppr.hpp"
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        VGL_RUNTIME::init_library(argc, argv);
        // the options of this app alone are taken out before the shared parser sees the rest
        PPR::Options opt;
        bool iters_given = false;
        std::vector<char *> rest{argv[0]};
        for (int i = 1; i < argc; i++) {
            const std::string a = argv[i];
            if (a == "-alpha" || a == "-iters" || a == "-tol") {
                if (i + 1 >= argc) throw "missing value for command line option";
                const char *v = argv[++i];
                if (a == "-alpha") opt.alpha = atof(v);
                else if (a == "-tol") opt.tol = atof(v);
                else { opt.iterations = atoi(v); iters_given = true; }
            } else rest.push_back(argv[i]);
        }
        if (opt.tol > 0.0 && !iters_given) opt.iterations = 1000;
        Parser parser;
        parser.parse_args((int)rest.size(), rest.data());
        if (!parser.fused) throw "ppr: only the fused path exists (pass -fused)";
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        vgl_hip_ctx *c = VGL_RUNTIME::ctx();
        const size_t V = (size_t)graph.get_vertices_count();
        std::vector<int> seeds;                                                       // in the graph's own numbering
        for (int v = 0; v < (int)V && (int)seeds.size() < parser.sources; v++) {
            const int stored = graph.reorder(v, ORIGINAL, SCATTER);
            if (graph.get_outgoing_connections_count(stored) > 0) seeds.push_back(stored);
        }
        std::vector<double> rank;
        std::vector<int> iterations;
        PPR::hip_fused(graph, std::vector<int>(seeds.begin(), seeds.begin() + std::min<size_t>(seeds.size(), 1)), opt, rank, iterations);      // heat run (builds the lists)
        const double perf = PPR::hip_fused(graph, seeds, opt, rank, iterations);      // timed
        report_performance(perf);
        PPR::print_launches(graph, seeds, opt);
        if (parser.get_check_flag()) {
            HostCSR out(graph, SCATTER), in(graph, GATHER);
            long long d_max = 0, dangling = 0;
            Timer host;
            host.start();
            const std::vector<double> want = PPR::seq_ppr(out, in, seeds, iterations, opt.alpha, &d_max, &dangling);
            host.end();
            std::cout << "host restatement: " << host.get_time() * 1000.0 << " ms" << std::endl;
            errors = PPR::verify(rank, want, V, iterations, opt.alpha, d_max, dangling);
        }
        if (!parser.dump.empty()) {
            std::vector<double> original(rank.size());
            if (graph.is_renumbered()) {                                              // 8-byte values: the 4-byte device reorder does not apply
                std::vector<int> bwd(V);
                VGL_HIP_CALL(vgl_hip_memcpy_d2h(c, bwd.data(), graph.get_backward_conversion(), sizeof(int) * V));
                for (size_t j = 0; j < seeds.size(); j++)
                    for (size_t s = 0; s < V; s++) original[j * V + (size_t)bwd[s]] = rank[j * V + s];
            } else original = rank;
            dump_array(parser.dump, original);
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors > 0 ? 1 : 0;
}
