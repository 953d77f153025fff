// vgl_simple.h -- the simple undirected graph under the stored outgoing CSR (loops dropped, parallel and antiparallel entries merged), built in
// simple.hip for tri, kcore, ktruss, msf and bicc.  DESIGN section 18.
#pragma once
#include "vgl_hip_internal.h"

// A CSR over the V vertices of that graph, with rows ascending by vertex id and free of duplicates, as the key sort leaves it.
struct vgl_simple_csr {
    vgl_dev<int64_t> rowptr;                     // V + 1
    vgl_dev<int32_t> adj;                        // nnz
    vgl_dev<int32_t> deg;                        // V: degree in the simple undirected graph
    int64_t nnz = 0;
    int32_t max_deg = 0;                         // the longest row
};

// The oriented CSR (every edge once, in the row of its lower endpoint under the order (stored out-degree [+ in-degree], id)): nnz = E'.  tri.hip
// keeps it next to its row classes.
int vgl_simple_build_oriented(vgl_hip_ctx *c, vgl_hip_graph *g, vgl_simple_csr *out);

// What the handle keeps of the simple graph (g->simple), in three lazy stages; every stage needs the ones before it.
struct vgl_simple_cache {
    int stages = 0;                              // how many of the stages below are built
    vgl_simple_csr csr;                          // 1: the symmetric CSR (every edge in both rows): nnz = 2 E', deg = row length
    int64_t ne = 0;                              // 2: E', and the numbering of the edges (ascending with (lo, hi)):
    vgl_dev<int32_t> eid;                        //    2 E': the edge of every slot of the symmetric CSR
    vgl_dev<int32_t> eu, ev;                     //    E' each: lo, hi
    vgl_dev<int32_t> slot_eid;                   // 3: E: the edge of every STORED outgoing entry, -1 for a loop
};
// The cache with at least the stage named built (the stages below it too, when they are missing); *built_now: this call built the stage named.
// The arrays live as long as the handle.
int vgl_simple_ensure_csr(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_simple_cache **out, bool *built_now);
int vgl_simple_ensure_edge_ids(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_simple_cache **out, bool *built_now);
int vgl_simple_ensure_slot_ids(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_simple_cache **out, bool *built_now);
