// sim app: vertex similarity of the simple undirected graph underlying the stored edges: the common neighbours of vertex pairs (default) or, with
// -topk, link prediction -- the K most similar vertices of every query over its 2-hop neighbourhood; heat run + timed run.  The symmetric simple CSR
// and the 2-path counts are prepared outside the timing.
//   -pairs N         N pairs (u, v) of ORIGINAL vertex ids from a counter hash of the seed (default 1048576); -pairs 0: all undirected edges instead
//   -topk K          link prediction with 1 <= K <= 64 instead of pairs
//   -metric M        common | jaccard | overlap: the score of -topk (default jaccard); equal scores go to the smaller ORIGINAL id
//   -queries Q       -topk: the first Q vertices that have a neighbour, in the graph's own numbering (default 1024)
//   -neighbours      -topk: the neighbours of a query are candidates too
//   -seed S          the seed of the pairs (also the generator's seed, as in every app; default 1)
//   -check           compare with the sequential host restatement (pairs: a merge of the two sorted rows; top-k: a dense counter, then a sort by the
//                    total order; its time is printed: the yardstick of the GPU numbers); exit status 1 on a difference
//   -dump FILE       int32 records in ORIGINAL vertex ids: (u, v, c) per pair in input order, or (query, candidate or -1, c) per output slot, row-major
#define INT_ELEMENTS_PER_EDGE 1.0      // the walked entry
#include "common.hpp"
#include "algorithms/sim.hpp"
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        long long n_pairs = 1 << 20;
        int topk = 0, n_queries = 1024, metric = VGL_HIP_SIM_JACCARD;
        bool neighbours = false;
        std::vector<char *> args;
        for (int i = 0; i < argc; i++) {
            const std::string a = argv[i];
            auto next = [&]() -> const char * { if (i + 1 >= argc) throw "missing value for command line option"; return argv[++i]; };
            if (i > 0 && a == "-pairs") n_pairs = atoll(next());
            else if (i > 0 && a == "-topk") topk = atoi(next());
            else if (i > 0 && a == "-queries") n_queries = atoi(next());
            else if (i > 0 && a == "-neighbours") neighbours = true;
            else if (i > 0 && a == "-metric") {
                const std::string m = next();
                if (m != "common" && m != "jaccard" && m != "overlap") throw "unknown value for -metric (common, jaccard or overlap)";
                metric = m == "common" ? VGL_HIP_SIM_COMMON : m == "jaccard" ? VGL_HIP_SIM_JACCARD : VGL_HIP_SIM_OVERLAP;
            }
            else args.push_back(argv[i]);
        }
        if (n_pairs < 0 || n_queries < 0) throw "-pairs and -queries take a count";
        VGL_RUNTIME::init_library((int)args.size(), args.data());
        Parser parser;
        parser.parse_args((int)args.size(), args.data());
        if (!parser.fused) throw "sim: only the fused path exists (pass -fused)";
        const uint32_t seed = (uint32_t)parser.seed;
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        {
            const int V = graph.get_vertices_count();
            const double prep = SIM::prepare(graph);
            SIM::Work w;
            w.topk = topk != 0;
            w.metric = metric; w.k = topk; w.include = neighbours ? 1 : 0;
            std::vector<int> hu, hv, hq, label((size_t)V);
            for (int v = 0; v < V; v++) label[(size_t)v] = graph.reorder(v, SCATTER, ORIGINAL);
            if (w.topk) {
                const std::vector<int> deg = SIM::degrees(graph);
                for (int v = 0; v < V && (int)hq.size() < n_queries; v++)
                    if (deg[(size_t)v] > 0) hq.push_back(v);
                w.queries.upload(hq);
                w.label.upload(label);
                w.ids.alloc(hq.size() * (size_t)std::max(topk, 1));
                w.tk_common.alloc(hq.size() * (size_t)std::max(topk, 1));
            } else {
                if (n_pairs == 0) {
                    HostCSR h(graph);
                    SIM::host_edges(SIM::host_simple(h), hu, hv);
                } else
                    for (long long i = 0; i < n_pairs; i++) {
                        hu.push_back(graph.reorder((int)(SIM::hash((uint32_t)(2 * i), seed) % (uint32_t)V), ORIGINAL, SCATTER));
                        hv.push_back(graph.reorder((int)(SIM::hash((uint32_t)(2 * i + 1), seed) % (uint32_t)V), ORIGINAL, SCATTER));
                    }
                w.u.upload(hu);
                w.v.upload(hv);
                w.common.alloc(hu.size());
            }
            SIM::hip_fused(graph, w, prep);                                                            // heat run
            const double perf = SIM::hip_fused(graph, w, prep);                                        // timed
            SIM::print_launches(graph, w);
            report_performance(perf);
            const std::vector<int> got = w.topk ? w.ids.host() : w.common.host();
            const std::vector<int> got_c = w.topk ? w.tk_common.host() : std::vector<int>();
            if (parser.get_check_flag()) {
                HostCSR h(graph);
                Timer tm;
                tm.start();
                const SIM::HostSimple s = SIM::host_simple(h);
                size_t bad = 0;
                auto differ = [&](const char *what, size_t i, long long a, long long b) {
                    if (bad++ < 10) std::cout << "error in " << what << " at " << i << ": " << a << " vs " << b << std::endl;
                };
                if (w.topk) {
                    std::vector<int> cnt((size_t)V, 0), ids((size_t)topk), com((size_t)topk);
                    for (size_t i = 0; i < hq.size(); i++) {
                        SIM::seq_topk(s, hq[i], metric, topk, neighbours, label, cnt, ids.data(), com.data());
                        for (int j = 0; j < topk; j++) {
                            if (got[i * (size_t)topk + (size_t)j] != ids[(size_t)j]) differ("ids", i * (size_t)topk + (size_t)j, got[i * (size_t)topk + (size_t)j], ids[(size_t)j]);
                            if (got_c[i * (size_t)topk + (size_t)j] != com[(size_t)j]) differ("common", i * (size_t)topk + (size_t)j, got_c[i * (size_t)topk + (size_t)j], com[(size_t)j]);
                        }
                    }
                } else
                    for (size_t i = 0; i < hu.size(); i++) {
                        const int c = SIM::seq_common(s, hu[i], hv[i]);
                        if (got[i] != c) differ("common", i, got[i], c);
                    }
                tm.end();
                std::cout << "SIM host restatement (sequential, " << (w.topk ? "dense counter + sort by the total order" : "merge of the two sorted rows")
                          << ", the simple graph built from the stored rows included): " << tm.get_time() * 1000.0 << " ms" << std::endl;
                errors = (int)std::min<size_t>(bad, 1u << 30);
                std::cout << "error count: " << errors << std::endl;
            }
            if (!parser.dump.empty()) {
                std::vector<int> flat;
                if (w.topk)
                    for (size_t i = 0; i < hq.size(); i++)
                        for (int j = 0; j < topk; j++) {
                            const int id = got[i * (size_t)topk + (size_t)j];
                            flat.push_back(label[(size_t)hq[i]]);
                            flat.push_back(id < 0 ? -1 : label[(size_t)id]);
                            flat.push_back(got_c[i * (size_t)topk + (size_t)j]);
                        }
                else
                    for (size_t i = 0; i < hu.size(); i++) { flat.push_back(label[(size_t)hu[i]]); flat.push_back(label[(size_t)hv[i]]); flat.push_back(got[i]); }
                dump_array(parser.dump, flat);
            }
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors ? 1 : 0;
}
