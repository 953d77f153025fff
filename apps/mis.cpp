// mis app: the lexicographically first maximal independent set (default) or maximal matching (-matching) of the simple undirected graph underlying
// the stored edges, under the library's default keys key(id, seed); heat run + timed run.  The symmetric simple CSR (and the edge numbering) is
// prepared outside the timing.
//   -matching        the maximal matching instead of the independent set
//   -seed S          the seed of the keys (also the generator's seed, as in every app; default 1).  The keys are those of the graph's OWN vertex
//                    (edge) numbering: under -format vcsr the set differs from that of -format csr; it is the greedy set of its order either way
//   -check           compare with the sequential host greedy (sort by (key, id), one pass; its time is printed: the yardstick of the GPU numbers);
//                    exit status 1 on a difference
//   -dump FILE       int32 records in ORIGINAL vertex ids: V records (v, in_set, round) ascending by v, or E' records (lo, hi, in_matching) ascending
//                    by (lo, hi)
#define INT_ELEMENTS_PER_EDGE 2.0      // the walked adjacency entry and one word of its far end
#include "common.hpp"
#include "algorithms/mis.hpp"
#include <array>
int main(int argc, char **argv)
{
    int errors = 0;
    try {
        bool matching = false;
        std::vector<char *> args;
        for (int i = 0; i < argc; i++) {
            if (i > 0 && std::string(argv[i]) == "-matching") matching = true;
            else args.push_back(argv[i]);
        }
        VGL_RUNTIME::init_library((int)args.size(), args.data());
        Parser parser;
        parser.parse_args((int)args.size(), args.data());
        if (!parser.fused) throw "mis: only the fused path exists (pass -fused)";
        const uint32_t seed = (uint32_t)parser.seed;
        VGL_Graph graph(parser.format);
        prepare_graph(graph, parser);
        {
            MIS::Result r;
            const double prep = MIS::prepare(graph, r, matching);
            MIS::hip_fused(graph, r, matching, seed, prep);                                            // heat run
            const double perf = MIS::hip_fused(graph, r, matching, seed, prep);                        // timed
            MIS::print_launches(graph, r, matching, seed);
            report_performance(perf);
            const std::vector<int> round = r.host(r.round, r.V);
            size_t bad = 0;
            auto differ = [&](const char *what, size_t i, long long a, long long b) {
                if (bad++ < 10) std::cout << "error in " << what << " at " << i << ": " << a << " vs " << b << std::endl;
            };
            if (matching) {
                const std::vector<int> eu = r.host(r.u, r.n), ev = r.host(r.v, r.n), mate = r.host(r.mate, r.V);
                const std::vector<unsigned char> mask = r.host(r.in_matching, r.n);
                if (parser.get_check_flag()) {
                    HostCSR h(graph);
                    Timer tm;
                    tm.start();
                    const MIS::HostMatching want = MIS::seq_greedy_matching(h, seed);
                    tm.end();
                    std::cout << "MATCHING host greedy (sequential, edge list + sort by (key, id) + one pass): " << tm.get_time() * 1000.0 << " ms" << std::endl;
                    if (want.u != eu || want.v != ev) {
                        std::cout << "the edge numbering differs from the host's" << std::endl;
                        bad = std::max<size_t>(1, std::max(eu.size(), want.u.size()));
                    } else {
                        for (size_t i = 0; i < mask.size(); i++)
                            if (mask[i] != want.in_matching[i]) differ("in_matching", i, mask[i], want.in_matching[i]);
                        for (size_t v = 0; v < mate.size(); v++) {
                            if (mate[v] != want.mate[v]) differ("mate", v, mate[v], want.mate[v]);
                            if ((round[v] > 0) != (mate[v] >= 0)) differ("round", v, round[v], mate[v]);
                        }
                    }
                    errors = (int)std::min<size_t>(bad, 1u << 30);
                    std::cout << "error count: " << errors << std::endl;
                }
                if (!parser.dump.empty()) {
                    std::vector<std::array<int, 3>> rows(eu.size());
                    for (size_t i = 0; i < eu.size(); i++) {
                        const int a = graph.reorder(eu[i], SCATTER, ORIGINAL), b = graph.reorder(ev[i], SCATTER, ORIGINAL);
                        rows[i] = {std::min(a, b), std::max(a, b), (int)mask[i]};
                    }
                    std::sort(rows.begin(), rows.end());
                    std::vector<int> flat;
                    flat.reserve(rows.size() * 3);
                    for (const auto &row : rows) { flat.push_back(row[0]); flat.push_back(row[1]); flat.push_back(row[2]); }
                    dump_array(parser.dump, flat);
                }
            } else {
                const std::vector<unsigned char> in_set = r.host(r.in_set, r.V);
                if (parser.get_check_flag()) {
                    HostCSR h(graph);
                    Timer tm;
                    tm.start();
                    const std::vector<unsigned char> want = MIS::seq_greedy_mis(h, seed);
                    tm.end();
                    std::cout << "MIS host greedy (sequential, edge list + sort by (key, id) + one pass): " << tm.get_time() * 1000.0 << " ms" << std::endl;
                    for (size_t v = 0; v < in_set.size(); v++) {
                        if (in_set[v] != want[v]) differ("in_set", v, in_set[v], want[v]);
                        if ((round[v] > 0) != (in_set[v] != 0) || round[v] == 0) differ("round", v, round[v], in_set[v]);
                    }
                    errors = (int)std::min<size_t>(bad, 1u << 30);
                    std::cout << "error count: " << errors << std::endl;
                }
                if (!parser.dump.empty()) {
                    std::vector<std::array<int, 3>> rows(in_set.size());
                    for (size_t v = 0; v < in_set.size(); v++) rows[v] = {graph.reorder((int)v, SCATTER, ORIGINAL), (int)in_set[v], round[v]};
                    std::sort(rows.begin(), rows.end());
                    std::vector<int> flat;
                    flat.reserve(rows.size() * 3);
                    for (const auto &row : rows) { flat.push_back(row[0]); flat.push_back(row[1]); flat.push_back(row[2]); }
                    dump_array(parser.dump, flat);
                }
            }
        }
        VGL_RUNTIME::finalize_library();
    } catch (std::string error) { std::cout << error << std::endl; return 1; }
    catch (const char *error) { std::cout << error << std::endl; return 1; }
    return errors ? 1 : 0;
}
