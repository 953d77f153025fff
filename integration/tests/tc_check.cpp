// tc_check -- a program against the VGL tree WITH the HIP binding applied (oracle/Makefile, target `binding`; not part of the reference).
//
// TransitiveClosure::vgl_purdoms (algorithms/tc/tc.hpp:5-163) UNCHANGED on the HIP backend: SCC labels, the edge filter through an EdgesArray indexed by
// global_edge_pos, ParallelPrimitives::copy_if_indexes on a device condition (vgl_compute_api/hip/parallel_primitives_hip.h), reduce(REDUCE_MAX), the
// condensed graph as an EDGES_LIST_GRAPH and BFS::fast_vgl_top_down over it (the class's edges-list workers).  The reference's own `tc -check` compares
// zero elements (apps/tc/tc.cpp:67: verify_results(..., 0)) and its checker reads levels[i] where it means levels[end_vertex] (tc.hpp:183), so the
// answers are checked HERE: every pair against a sequential breadth-first search over the same graph through VGL_Graph's public accessors.
//
// The graph is SEEDED (-seed, default 1), as in scc_check.cpp: the reference's generators seed themselves with time(NULL), and its forward-backward
// SCC puts a few vertices into the wrong component on some small graphs on any backend (tests/golden/scc_reference_disagreements.json), so an
// unseeded run answers a pair wrongly now and then whatever the backend does.  With a seed the outcome is a fixed function of the arguments.
//
// usage: vgl_hip_tc_check -s <scale> -e <edge factor> -type rmat|ru -format csr [-it <pairs>] [-seed <n>]          prints TC CHECK PASSED / FAILED

#define INT_ELEMENTS_PER_EDGE 5.0
#define VECTOR_ENGINE_THRESHOLD_VALUE VECTOR_LENGTH*MAX_SX_AURORA_THREADS*128
#define VECTOR_CORE_THRESHOLD_VALUE 3*VECTOR_LENGTH

#include "graph_library.h"
#include <queue>

static inline unsigned long long splitmix64(unsigned long long &state)
{
    unsigned long long z = (state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// a directed edge list from a splitmix64 stream: R-MAT (the quadrant probabilities of graph_generation.hpp:131-169, ids scrambled as in
// scc_check.cpp) or uniformly random endpoints
static void fill_edges(EdgesContainer &edges, int scale, int edge_factor, bool rmat, unsigned long long seed)
{
    const int vertices_count = 1 << scale;
    const long long edges_count = (long long)vertices_count * edge_factor;
    edges.resize(vertices_count, edges_count);
    int *src_ids = edges.get_src_ids(), *dst_ids = edges.get_dst_ids();
    unsigned long long state = seed * 0x2545F4914F6CDD1DULL + 12345;
    for (long long e = 0; e < edges_count; e++) {
        if (!rmat) {
            src_ids[e] = (int)(splitmix64(state) % (unsigned long long)vertices_count);
            dst_ids[e] = (int)(splitmix64(state) % (unsigned long long)vertices_count);
            continue;
        }
        int row = 0, col = 0;
        for (int bit = 0; bit < scale; bit++) {
            const unsigned r = (unsigned)(splitmix64(state) % 100);
            const int quadrant = r < 57 ? 0 : (r < 76 ? 1 : (r < 95 ? 2 : 3));
            row = (row << 1) | (quadrant >> 1);
            col = (col << 1) | (quadrant & 1);
        }
        src_ids[e] = (int)(((unsigned long long)row * 2654435761ULL + 7) % (unsigned long long)vertices_count);
        dst_ids[e] = (int)(((unsigned long long)col * 2654435761ULL + 7) % (unsigned long long)vertices_count);
    }
}

// is `to` reachable from `from` along stored edges (a vertex reaches itself)
static bool reachable(VGL_Graph &graph, int from, int to, std::vector<int> &seen, int stamp)
{
    if (from == to) return true;
    std::queue<int> todo;
    todo.push(from);
    seen[from] = stamp;
    while (!todo.empty()) {
        const int v = todo.front();
        todo.pop();
        const int n = graph.get_connections_count(v, SCATTER);
        for (int k = 0; k < n; k++) {
            const int u = graph.get_edge_dst(v, k, SCATTER);
            if (u == to) return true;
            if (seen[u] != stamp) { seen[u] = stamp; todo.push(u); }
        }
    }
    return false;
}

int main(int argc, char **argv)
{
    int failures = 0;
    try
    {
        VGL_RUNTIME::init_library(argc, argv);
        Parser parser;
        parser.parse_args(argc, argv);
        unsigned long long seed = 1;
        for (int i = 1; i + 1 < argc; i++)
            if (string(argv[i]) == "-seed") seed = strtoull(argv[i + 1], NULL, 10);
        VGL_Graph graph(VGL_RUNTIME::select_graph_format(parser), VGL_RUNTIME::select_graph_optimizations(parser));
        {
            EdgesContainer edges;
            fill_edges(edges, parser.get_scale(), parser.get_avg_degree(), parser.get_synthetic_graph_type() == RMAT, seed);
            graph.import(edges);
        }
        if (graph.get_container_type() != CSR_GRAPH) throw "tc_check: -format csr (pairs and answers are vertex ids of ONE numbering there)";
        const int vertices_count = graph.get_vertices_count();

        // pairs: random ones (mostly different components), plus pairs along stored edges and their reversals (same component or one-way)
        const int wanted = std::max(8, parser.get_number_of_rounds());
        vector<pair<int, int>> pairs;
        srand(20260105);
        for (int i = 0; i < wanted; i++) pairs.push_back(make_pair(rand() % vertices_count, rand() % vertices_count));
        for (int i = 0; i < wanted; i++) {
            const int v = rand() % vertices_count, n = graph.get_connections_count(v, SCATTER);
            if (n == 0) continue;
            const int u = graph.get_edge_dst(v, rand() % n, SCATTER);
            pairs.push_back(make_pair(v, u));
            pairs.push_back(make_pair(u, v));
        }
        vector<int> answer(pairs.size(), -1);
        TC::vgl_purdoms(graph, pairs, answer);

        std::vector<int> seen((size_t)vertices_count, 0);
        int yes = 0;
        for (size_t i = 0; i < pairs.size(); i++) {
            const bool truth = reachable(graph, pairs[i].first, pairs[i].second, seen, (int)i + 1);
            yes += truth;
            if ((answer[i] != 0) != truth) {
                failures++;
                if (failures <= 10) cout << "pair " << i << " (" << pairs[i].first << " -> " << pairs[i].second << "): vgl_purdoms says " << answer[i] << ", a sequential search says " << truth << endl;
            }
        }
        cout << pairs.size() << " pairs, " << yes << " reachable, " << failures << " wrong answers" << endl;
        if (yes == 0 || yes == (int)pairs.size()) { cout << "(the pairs do not tell the two answers apart)" << endl; failures++; }
        cout << (failures ? "TC CHECK FAILED" : "TC CHECK PASSED") << endl;
        VGL_RUNTIME::finalize_library();
    }
    catch (string error) { cout << error << endl; return 2; }
    catch (const char *error) { cout << error << endl; return 2; }
    return failures ? 1 : 0;
}
