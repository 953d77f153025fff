// vgl_chunks.h -- chunked workgroup rows: how a row of the workgroup class becomes work items (kcore, msf, msbfs, bc).  The host rule and the device
// mapping, once.  Includes nothing of HIP, so a plain host compiler can build it (tests/rc_chunks_main.cpp).  Included from vgl_rowclass.h.
// DESIGN section 21, "Chunked workgroup rows".
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VGL_HD __host__ __device__ __forceinline__
#else
#define VGL_HD inline
#endif

// grid.y of the 2-D forms (kcore_wg, bc_hub), which must stay <= 65535, and the bound of the flat forms' item count: rows * VGL_RC_MAX_CHUNKS
constexpr int32_t VGL_RC_MAX_CHUNKS = 32768;

// A row [row_lo, row_end) is cut into pieces of `chunk` entries, one workgroup per piece; every row of a launch gets `nchunks` items, as many as the
// longest row needs, and an item past the end of its row is empty.
struct vgl_rc_chunks {
    int32_t chunk, nchunks;
    // the host rule: the switch's chunk, raised until the longest row has at most max_chunks pieces; a graph without entries has one (empty) piece
    static vgl_rc_chunks of(int64_t chunk_env, int64_t longest_row, int64_t max_chunks = VGL_RC_MAX_CHUNKS)
    {
        const int64_t longest = longest_row > 1 ? longest_row : 1, need = (longest + max_chunks - 1) / max_chunks;
        const int64_t chunk = chunk_env > need ? chunk_env : need, n = (longest + chunk - 1) / chunk;
        return vgl_rc_chunks{(int32_t)chunk, (int32_t)(n > 1 ? n : 1)};
    }
    // one piece per row: what a kernel without chunks runs on
    static constexpr vgl_rc_chunks whole() { return vgl_rc_chunks{INT32_MAX, 1}; }
    // piece k of the row: [*lo, *hi), false when it is empty (*hi is not written then)
    VGL_HD bool range(int64_t row_lo, int64_t row_end, int64_t k, int64_t *lo, int64_t *hi) const
    {
        *lo = row_lo + k * chunk;
        if (*lo >= row_end) return false;
        *hi = row_end < *lo + chunk ? row_end : *lo + chunk;
        return true;
    }
    // the flat forms: item it = row_index * nchunks + k
    VGL_HD void split(int64_t it, int64_t *row_index, int64_t *k) const
    {
        *row_index = it / nchunks;
        *k = it % nchunks;
    }
    // the non-empty pieces of a row of `len` entries (they are the first ones)
    VGL_HD int64_t pieces(int64_t len) const
    {
        const int64_t p = (len + chunk - 1) / chunk;
        return p < nchunks ? p : nchunks;
    }
};

// the chunk of a VGL_<ALG>_CHUNK switch: 16384 unless set, 16 <= chunk <= 2^28
struct vgl_hip_ctx;
int64_t vgl_env_int(vgl_hip_ctx *c, const char *name, int64_t dflt, int64_t lo, int64_t hi);
static inline int64_t vgl_rc_env_chunk(vgl_hip_ctx *c, const char *env_chunk) { return vgl_env_int(c, env_chunk, 16384, 16, 1 << 28); }
