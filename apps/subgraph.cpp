// subgraph app: the part of a graph that a mask or a neighbourhood selects, handed back as CSR in both directions (the stable row filter of
// include/vgl_hip.h), or fixed-fanout neighbour sampling; heat run + timed run, the plan and the fill timed separately.
//   -mask P          keep the vertices whose counter hash of the seed is below P percent (default mode, P = 50)
//   -kcore K         keep the K-core (the core numbers are computed outside the timing)
//   -hops H          keep the H-hop neighbourhood of the seed vertices along outgoing entries (vgl_hip_khop_run, timed too)
//   -sample F        instead of a subgraph: F neighbours without replacement for every seed vertex (vgl_hip_sample_neighbors)
//   -seeds N         the seed vertices of -hops / -sample: N vertex ids from the counter hash (default 1024), repeats possible
//   -seed S          the seed of masks, seed vertices and sampling keys (also the generator's seed, as in every app; default 1)
//   -check           compare with the sequential host restatement (a filter of the stored rows in order, a host BFS, a sort of (key, position) per
//                    row; its time is printed: the yardstick of the GPU numbers); exit status 1 on a difference
//   -dump FILE       int32 records in the graph's own numbering: (row, entry) per outgoing entry of the subgraph in CSR order with the PARENT'S ids,
//                    or (seed vertex, sampled neighbour) per sampled entry
#define INT_ELEMENTS_PER_EDGE 1.0      // the examined entry
#include "common.hpp"
#include "algorithms/subgraph.hpp"
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        int mask_percent = 50, kcore = 0, hops = -1, fanout = 0, n_seeds = 1024;
        std::vector<char *> args;
        for (int i = 0; i < argc; i++) {
            const std::string a = argv[i];
            auto next = [&]() -> const char * { if (i + 1 >= argc) throw "missing value for command line option"; return argv[++i]; };
            if (i > 0 && a == "-mask") mask_percent = atoi(next());
            else if (i > 0 && a == "-kcore") kcore = atoi(next());
            else if (i > 0 && a == "-hops") hops = atoi(next());
            else if (i > 0 && a == "-sample") fanout = atoi(next());
            else if (i > 0 && a == "-seeds") n_seeds = atoi(next());
            else args.push_back(argv[i]);
        }
        if (mask_percent < 0 || mask_percent > 100 || kcore < 0 || n_seeds < 0 || fanout < 0) throw "-mask takes a percentage; -kcore, -seeds and -sample take a count";
        VGL_RUNTIME::init_library((int)args.size(), args.data());
        Parser parser;
        parser.parse_args((int)args.size(), args.data());
        if (!parser.fused) throw "subgraph: only the fused path exists (pass -fused)";
        const uint32_t seed = (uint32_t)parser.seed;
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        {
            vgl_hip_ctx *c = VGL_RUNTIME::ctx();
            const int V = graph.get_vertices_count();
            std::vector<int> hseeds;
            for (int i = 0; i < n_seeds; i++) hseeds.push_back((int)(SUBG::key((uint32_t)i, seed + 1u) % (uint32_t)V));
            SUBG::Device<int> seeds;
            seeds.upload(hseeds);
            auto differ = [&](const char *what, size_t i, long long a, long long b) {
                if (errors++ < 10) std::cout << "error in " << what << " at " << i << ": " << a << " vs " << b << std::endl;
            };
            auto compare = [&](const char *what, const auto &got, const auto &want) {
                if (got.size() != want.size()) { differ(what, 0, (long long)got.size(), (long long)want.size()); return; }
                for (size_t i = 0; i < got.size(); i++)
                    if ((long long)got[i] != (long long)want[i]) differ(what, i, (long long)got[i], (long long)want[i]);
            };
            if (fanout > 0) {
                // ---- sampling ----
                SUBG::Device<long long> rowptr, origin;
                SUBG::Device<int> adj;
                rowptr.alloc(hseeds.size() + 1);
                adj.alloc(hseeds.size() * (size_t)fanout);
                origin.alloc(hseeds.size() * (size_t)fanout);
                vgl_hip_sample_stats st;
                double secs = 0.0;
                for (int run = 0; run < 3; run++) {                                                    // heat, timed, launches
                    if (run == 2) { VGL_HIP_CALL(vgl_hip_timing_reset(c)); VGL_HIP_CALL(vgl_hip_timing_enable(c, 1)); }
                    Timer tm;
                    tm.start();
                    VGL_HIP_CALL(vgl_hip_sample_neighbors(c, graph.get_handle(), seeds.p, (int64_t)hseeds.size(), fanout, 0, seed, (int64_t *)rowptr.p, adj.p, (int64_t *)origin.p, &st));
                    tm.end();
                    if (run == 1) secs = tm.get_time();
                }
                VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
                std::cout << "SAMPLE: " << st.seeds << " seeds, fanout " << fanout << ", rows short / wave / wg " << st.rows_short << " / " << st.rows_wave << " / " << st.rows_wg
                          << ", entries_examined " << st.entries_examined << ", sampled_total " << st.sampled_total << ", " << secs * 1000.0 << " ms, " << st.algorithmic_bytes
                          << " bytes of the model, " << st.algorithmic_bytes / (secs * 1e9) << " GB/s" << std::endl;
                SUBG::print_launches("SAMPLE", {"sample_count", "sample_publish", "sample_short", "sample_wave", "sample_wg"});
                performance_stats.print_algorithm_performance_stats("SAMPLE (fused)", secs, st.entries_examined);
                report_performance(performance_stats.get_algorithm_performance(secs, st.entries_examined));
                const std::vector<long long> got_rp = rowptr.host(), got_org = origin.host();
                const std::vector<int> got_adj = adj.host();
                if (parser.get_check_flag()) {
                    HostCSR h(graph);
                    Timer tm;
                    tm.start();
                    std::vector<long long> rp(1, 0), org;
                    std::vector<int> ad;
                    for (int v : hseeds) {
                        for (long long p : SUBG::seq_select(h, v, fanout, seed)) { org.push_back(p); ad.push_back(h.adj[(size_t)p]); }
                        rp.push_back((long long)org.size());
                    }
                    tm.end();
                    compare("rowptr", got_rp, rp);
                    compare("adj", std::vector<int>(got_adj.begin(), got_adj.begin() + (size_t)st.sampled_total), ad);
                    compare("origin", std::vector<long long>(got_org.begin(), got_org.begin() + (size_t)st.sampled_total), org);
                    std::cout << "SAMPLE host restatement (sequential, sort of (key, position) per row): " << tm.get_time() * 1000.0 << " ms" << std::endl;
                    std::cout << "error count: " << errors << std::endl;
                }
                if (!parser.dump.empty()) {
                    std::vector<int> flat;
                    for (size_t i = 0; i < hseeds.size(); i++)
                        for (long long p = got_rp[i]; p < got_rp[i + 1]; p++) { flat.push_back(hseeds[i]); flat.push_back(got_adj[(size_t)p]); }
                    dump_array(parser.dump, flat);
                }
            } else {
                // ---- a vertex mask, then the row filter ----
                std::vector<unsigned char> hkeep((size_t)V, 0);
                SUBG::Device<unsigned char> keep;
                SUBG::Device<int> hop;
                vgl_hip_khop_stats ks;
                memset(&ks, 0, sizeof(ks));
                double khop_secs = 0.0;
                const char *mode = hops >= 0 ? "ego" : kcore > 0 ? "kcore" : "mask";
                if (hops >= 0) {
                    hop.alloc((size_t)V);
                    for (int run = 0; run < 2; run++) {
                        Timer tm;
                        tm.start();
                        VGL_HIP_CALL(vgl_hip_khop_run(c, graph.get_handle(), seeds.p, (int64_t)hseeds.size(), hops, 0, 0, hop.p, &ks));
                        tm.end();
                        khop_secs = tm.get_time();
                    }
                    const std::vector<int> hh = hop.host();
                    for (int v = 0; v < V; v++) hkeep[(size_t)v] = hh[(size_t)v] >= 0;
                    std::cout << "KHOP: " << hseeds.size() << " seeds, hops " << hops << ", reached " << ks.reached << ", levels_run " << ks.levels_run << ", frontier_total "
                              << ks.frontier_total << ", edges_examined " << ks.edges_examined << ", " << khop_secs * 1000.0 << " ms" << std::endl;
                    if (parser.get_check_flag()) {
                        HostCSR h(graph);
                        Timer tm;
                        tm.start();
                        const std::vector<int> want = SUBG::seq_khop(h, hseeds, hops);
                        tm.end();
                        compare("hop", hh, want);
                        std::cout << "KHOP host restatement (sequential BFS): " << tm.get_time() * 1000.0 << " ms" << std::endl;
                    }
                } else if (kcore > 0) {
                    SUBG::Device<int> core;
                    core.alloc((size_t)V);
                    VGL_HIP_CALL(vgl_hip_kcore_run(c, graph.get_handle(), kcore, core.p, nullptr, nullptr));
                    const std::vector<int> hc = core.host();
                    for (int v = 0; v < V; v++) hkeep[(size_t)v] = hc[(size_t)v] >= kcore;
                } else
                    for (int v = 0; v < V; v++) hkeep[(size_t)v] = SUBG::key((uint32_t)graph.reorder(v, SCATTER, ORIGINAL), seed) % 100u < (uint32_t)mask_percent;
                keep.upload(hkeep);
                SUBG::Sub s;
                SUBG::extract(graph, keep.p, s);                                                       // heat run
                const std::pair<double, double> t = SUBG::extract(graph, keep.p, s);                   // timed
                VGL_HIP_CALL(vgl_hip_timing_reset(c));
                VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
                SUBG::extract(graph, keep.p, s);
                VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
                const vgl_hip_subgraph_stats &st = s.st;
                const double secs = t.first + t.second;
                std::cout << "SUBGRAPH " << mode << ": vertices_kept " << st.vertices_kept << " of " << V << ", rows short / wave / wg out " << st.rows_short_out << " / "
                          << st.rows_wave_out << " / " << st.rows_wg_out << ", in " << st.rows_short_in << " / " << st.rows_wave_in << " / " << st.rows_wg_in << ", entries_read "
                          << st.entries_read_out << " / " << st.entries_read_in << ", entries_kept " << st.entries_kept_out << " / " << st.entries_kept_in << ", plan "
                          << t.first * 1000.0 << " ms, fill " << t.second * 1000.0 << " ms, " << st.algorithmic_bytes << " bytes of the model, "
                          << st.algorithmic_bytes / (secs * 1e9) << " GB/s" << std::endl;
                SUBG::print_launches("SUBGRAPH", {"sub_scan", "sub_count_short", "sub_count_wave", "sub_count_wg", "sub_publish", "sub_fill_short", "sub_fill_wave", "sub_fill_wg"});
                const long long work = st.entries_read_out + st.entries_read_in;
                performance_stats.print_algorithm_performance_stats("SUBGRAPH (fused)", secs, work);
                report_performance(performance_stats.get_algorithm_performance(secs, work));
                const std::vector<int> got_old = s.old_id.host();
                const std::vector<long long> got_rp = s.rowptr[0].host();
                const std::vector<int> got_adj = s.adj[0].host();
                if (parser.get_check_flag()) {
                    Timer tm;
                    tm.start();
                    double host_secs = 0.0;
                    for (int d = 0; d < 2; d++) {
                        HostCSR h(graph, d == 0 ? SCATTER : GATHER);
                        std::vector<long long> rp, org;
                        std::vector<int> ad, old;
                        Timer th;
                        th.start();
                        SUBG::seq_filter(h, hkeep, rp, ad, org, old);
                        th.end();
                        host_secs += th.get_time();
                        compare(d == 0 ? "old_id" : "old_id (in)", got_old, old);
                        if (s.V > 0) {
                            compare(d == 0 ? "out rowptr" : "in rowptr", s.rowptr[d].host(), rp);
                            compare(d == 0 ? "out adj" : "in adj", s.adj[d].host(), ad);
                            if (d == 0) compare("origin", s.origin.host(), org);
                        }
                    }
                    tm.end();
                    std::cout << "SUBGRAPH host restatement (sequential filter of the stored rows, both directions): " << host_secs * 1000.0 << " ms" << std::endl;
                    std::cout << "error count: " << errors << std::endl;
                }
                if (!parser.dump.empty() && s.V > 0) {
                    std::vector<int> flat;
                    for (int i = 0; i < s.V; i++)
                        for (long long p = got_rp[(size_t)i]; p < got_rp[(size_t)i + 1]; p++) { flat.push_back(got_old[(size_t)i]); flat.push_back(got_old[(size_t)got_adj[(size_t)p]]); }
                    dump_array(parser.dump, flat);
                }
            }
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors ? 1 : 0;
}
