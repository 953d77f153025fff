// quotient app: the quotient graph of a vertex labelling, handed back as CSR in both directions with the multiplicity of every coarse entry (the row
// merge of include/vgl_hip.h); heat run + timed run, the plan and the fill timed separately.
//   -clusters K      label every vertex fmix32(original id ^ seed) mod K (default mode, K = max(1, V / 64))
//   -cc              label by vgl_hip_cc_run, -scc by vgl_hip_scc_run (the labels are computed outside the timing; -scc -noloops is the condensation)
//   -noloops         leave out the entries inside a cluster
//   -seed S          the seed of the hashed labels (also the generator's seed, as in every app; default 1)
//   -check           compare with the sequential host restatement (sort the key pairs of the stored entries, run-length sum; its time is printed: the
//                    yardstick of the GPU numbers); exit status 1 on a difference
//   -dump FILE       int64 records (c, c', count) per outgoing coarse entry in CSR order
#define INT_ELEMENTS_PER_EDGE 2.0      // the examined entry and the cluster of its far end
#include "common.hpp"
#include "algorithms/quotient.hpp"
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        long long clusters = 0;
        bool use_cc = false, use_scc = false, noloops = false;
        std::vector<char *> args;
        for (int i = 0; i < argc; i++) {
            const std::string a = argv[i];
            auto next = [&]() -> const char * { if (i + 1 >= argc) throw "missing value for command line option"; return argv[++i]; };
            if (i > 0 && a == "-clusters") clusters = atoll(next());
            else if (i > 0 && a == "-cc") use_cc = true;
            else if (i > 0 && a == "-scc") use_scc = true;
            else if (i > 0 && a == "-noloops") noloops = true;
            else args.push_back(argv[i]);
        }
        if (clusters < 0 || (use_cc && use_scc)) throw "-clusters takes a count; -cc and -scc exclude each other";
        VGL_RUNTIME::init_library((int)args.size(), args.data());
        Parser parser;
        parser.parse_args((int)args.size(), args.data());
        if (!parser.fused) throw "quotient: only the fused path exists (pass -fused)";
        const uint32_t seed = (uint32_t)parser.seed;
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        {
            vgl_hip_ctx *c = VGL_RUNTIME::ctx();
            const int V = graph.get_vertices_count();
            const char *mode = use_cc ? "cc" : use_scc ? "scc" : "hashed";
            std::vector<int> hlabel((size_t)V, 0);
            QUOT::Device<int> label;
            if (use_cc || use_scc) {
                label.alloc((size_t)V);
                if (use_cc) VGL_HIP_CALL(vgl_hip_cc_run(c, graph.get_handle(), label.p, nullptr));
                else VGL_HIP_CALL(vgl_hip_scc_run(c, graph.get_handle(), label.p, nullptr));
                hlabel = label.host();
            } else {
                const uint32_t K = (uint32_t)(clusters > 0 ? clusters : std::max(1, V / 64));
                for (int v = 0; v < V; v++) hlabel[(size_t)v] = (int)(QUOT::fmix32((uint32_t)graph.reorder(v, SCATTER, ORIGINAL) ^ seed) % K);
                label.upload(hlabel);
            }
            auto differ = [&](const char *what, size_t i, long long a, long long b) {
                if (errors++ < 10) std::cout << "error in " << what << " at " << i << ": " << a << " vs " << b << std::endl;
            };
            auto compare = [&](const char *what, const auto &got, const auto &want) {
                if (got.size() != want.size()) { differ(what, 0, (long long)got.size(), (long long)want.size()); return; }
                for (size_t i = 0; i < got.size(); i++)
                    if ((long long)got[i] != (long long)want[i]) differ(what, i, (long long)got[i], (long long)want[i]);
            };
            QUOT::Quotient q;
            QUOT::run(graph, label.p, noloops, q);                                                     // heat run
            const std::pair<double, double> t = QUOT::run(graph, label.p, noloops, q);                 // timed
            VGL_HIP_CALL(vgl_hip_timing_reset(c));
            VGL_HIP_CALL(vgl_hip_timing_enable(c, 1));
            QUOT::run(graph, label.p, noloops, q);
            VGL_HIP_CALL(vgl_hip_timing_enable(c, 0));
            const vgl_hip_quotient_stats &st = q.st;
            const double secs = t.first + t.second;
            std::cout << "QUOTIENT " << mode << (noloops ? " (no loops)" : "") << ": vertices " << st.vertices << " of " << V << ", rows short / wave / table / sorted out "
                      << st.rows_short_out << " / " << st.rows_wave_out << " / " << st.rows_table_out << " / " << st.rows_sorted_out << ", in " << st.rows_short_in << " / "
                      << st.rows_wave_in << " / " << st.rows_table_in << " / " << st.rows_sorted_in << ", entries_read " << st.entries_read_out << " / " << st.entries_read_in
                      << ", entries " << st.entries_out << " / " << st.entries_in << ", sorted_keys " << st.sorted_keys_out << " / " << st.sorted_keys_in << ", sort_pieces "
                      << st.sort_pieces_out << " / " << st.sort_pieces_in << ", plan " << t.first * 1000.0 << " ms, fill " << t.second * 1000.0 << " ms, " << st.algorithmic_bytes
                      << " bytes of the model, " << st.algorithmic_bytes / (secs * 1e9) << " GB/s" << std::endl;
            QUOT::print_launches("QUOTIENT", {"quot_check", "quot_vertex", "quot_member_off", "quot_classify", "quot_lists", "quot_count_short", "quot_count_wave", "quot_count_table",
                                              "quot_count_sorted", "quot_scan", "quot_publish", "quot_fill_short", "quot_fill_wave", "quot_fill_table", "quot_fill_sorted"});
            const long long work = st.entries_read_out + st.entries_read_in;
            performance_stats.print_algorithm_performance_stats("QUOTIENT (fused)", secs, work);
            report_performance(performance_stats.get_algorithm_performance(secs, work));
            const std::vector<long long> got_rp = q.rowptr[0].host(), got_cnt = q.count[0].host();
            const std::vector<int> got_adj = q.adj[0].host();
            if (parser.get_check_flag()) {
                double host_secs = 0.0;
                std::vector<int> cluster_of, label_of, size;
                {
                    Timer th;
                    th.start();
                    QUOT::seq_vertex_maps(hlabel, cluster_of, label_of, size);
                    th.end();
                    host_secs += th.get_time();
                }
                compare("cluster_of", q.cluster_of.host(), cluster_of);
                compare("label_of", q.label_of.host(), label_of);
                compare("size", q.size.host(), size);
                for (int d = 0; d < (q.has_in ? 2 : 1); d++) {
                    HostCSR h(graph, d == 0 ? SCATTER : GATHER);
                    std::vector<long long> rp, cnt;
                    std::vector<int> ad;
                    Timer th;
                    th.start();
                    QUOT::seq_quotient(h, cluster_of, (int)label_of.size(), noloops, rp, ad, cnt);
                    th.end();
                    host_secs += th.get_time();
                    compare(d == 0 ? "out rowptr" : "in rowptr", q.rowptr[d].host(), rp);
                    compare(d == 0 ? "out adj" : "in adj", q.adj[d].host(), ad);
                    compare(d == 0 ? "out count" : "in count", q.count[d].host(), cnt);
                }
                std::cout << "QUOTIENT host restatement (sequential: sort of the key pairs, run-length sum, both directions): " << host_secs * 1000.0 << " ms" << std::endl;
                std::cout << "error count: " << errors << std::endl;
            }
            if (!parser.dump.empty()) {
                std::vector<long long> flat;
                for (int i = 0; i < q.V; i++)
                    for (long long p = got_rp[(size_t)i]; p < got_rp[(size_t)i + 1]; p++) { flat.push_back(i); flat.push_back(got_adj[(size_t)p]); flat.push_back(got_cnt[(size_t)p]); }
                dump_array(parser.dump, flat);
            }
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors ? 1 : 0;
}
