// agg.hip -- neighbour aggregation over a borrowed CSR: out[i, :] = the sum, mean, max or min over the entries p of row i of x[adj[p], :] (float32, any
// width F, optionally weighted per entry), and the exact backward of it: gx[u, :] = the sum over the entries p with adj[p] = u, in ascending p, of a
// coefficient times g[row(p), :].  The contract is written out in include/vgl_hip.h; DESIGN section 29 has the kernels, their resources, the bytes
// model, the tolerance and the measurements.
//
//   plan       checks the CSR (one count over the rows, one over the entries), classifies the rows once (short: 8 lanes per row, wave: a wavefront,
//              wg: a workgroup per chunk of VGL_AGG_CHUNK entries), sorts each class list ascending and cuts the workgroup rows into chunks.
//   transpose  built by the first backward run and kept: the entry list in CSR order, (adj[p], row(p)), through the stable vgl_hip_coo_to_csr with its
//              permutation, which is the origin p of every transposed entry; class lists and chunks of its own.
//   rows       ONE team kernel serves the forward pass on the plan's CSR and the backward pass on its transpose.  The lanes of a team are (entry slot
//              x column group): NQ lanes cover one tile of NQ * VEC columns, slot s adds entries s, s + SLOTS, ... in row order with four gathers
//              in flight, then the slots of a column group are folded by an xor butterfly and, in a workgroup, the four waves from LDS in wave order.
//              A wider F walks the row once per column tile.  Max / min carry (value, position) and prefer the smaller position on equal values.
//   hubs       a row of more than one chunk leaves one partial per chunk; one writer per (row, column) finishes them in chunk order.
//   heads      vgl_hip_agg_run_heads / _run_transposed_heads: E x H weights, head h weighs the columns [h D, (h + 1) D); the team kernel's HEADS
//              instantiations differ in the coefficient alone, the hub kernel serves as it is.
// Every value has one writer and every sum a shape fixed by (row length, F, VEC, the three switches): no floating-point atomic, no scratch memory, no
// cooperative launch, no wait on a flag, no retry loop.
#include "vgl_agg.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

enum { AGG_K_SUM = 0, AGG_K_EXT = 1 };           // the kernel's OP: a sum of coefficient x value (sum, mean, every backward), an extreme (max, min)
constexpr int64_t AGG_MAX_ENTRIES = 0x7FFFFFF0LL;  // positions are int32 in d_arg and in the transpose's origin
enum { AC_ROWS = 0, AC_TAIL = 3, AC_BAD = 6, AC_WORK = 7, AC_ENT = 8, AC_NCNT = 11 };
static_assert(AC_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

// one pass.  Forward: the CSR is the plan's, a term's source row is adj[p], its coefficient weight[p].  Transposed: the CSR is the transpose, adj[p] is
// row(o) of the origin o = origin[p], the coefficient is read through o.
struct agg_args {
    const int64_t *rowptr;       // the CSR walked
    const int32_t *adj;
    const int32_t *origin;       // transposed: the position in the plan's CSR of a transposed entry
    const int64_t *len_rowptr;   // transposed MEAN: the plan's rowptr, for len(row(o)); else nullptr
    const float *weight;         // per entry of the plan's CSR, or nullptr
    const int32_t *arg;          // transposed MAX / MIN: n_rows x F, the position that attained the extreme; else nullptr
    const float *x;              // the rows gathered, leading dimension ldx
    float *out;                  // the rows written, leading dimension ldo
    int32_t *oarg;               // forward MAX / MIN: rows x F, or nullptr
    float *cpart;                // F per workgroup item: the chunk results of the rows of more than one chunk
    int32_t *cpart_arg;          // ... and their positions (MAX / MIN)
    int64_t ldx, ldo;
    int32_t F, chunk;
    int32_t lognq[VGL_RC_N];     // log2 of the lanes that cover a column tile, per class
    int32_t mean, neg;           // forward MEAN: divide by the row's length at the end; MIN: the extreme of -x
    int32_t H, D;                // the heads form: weight is E x H, head h owns the columns [h D, (h + 1) D); else 0
};

// the source row, the coefficient and the origin of the term at position p of the walked CSR; the heads form reads the weight of head hd of the origin
template <bool TR, bool HEADS>
__device__ __forceinline__ void agg_term(const agg_args &a, int64_t p, int hd, int32_t &u, float &cf, int32_t &o)
{
    u = a.adj[p];
    if constexpr (TR) {
        o = a.origin[p];
        if constexpr (HEADS) cf = a.weight[(int64_t)o * a.H + hd];
        else cf = a.weight ? a.weight[o] : 1.0f;
        if (a.len_rowptr) cf = cf / (float)(a.len_rowptr[u + 1] - a.len_rowptr[u]);
    } else {
        o = (int32_t)p;
        if constexpr (HEADS) cf = a.weight[p * a.H + hd];
        else cf = a.weight ? a.weight[p] : 1.0f;
    }
}
// the VEC values of the term at column c0; transposed MAX / MIN: 0 where the origin did not attain the extreme
template <int VEC, bool TR>
__device__ __forceinline__ void agg_values(const agg_args &a, int32_t u, int32_t o, int c0, float *t)
{
    agg_load<VEC>(a.x + (int64_t)u * a.ldx + c0, t);
    if constexpr (TR)
        if (a.arg) {
            int32_t w[VEC];
            agg_load<VEC>(a.arg + (int64_t)u * a.F + c0, w);
#pragma unroll
            for (int k = 0; k < VEC; k++) t[k] = w[k] == o ? t[k] : 0.0f;
        }
}
// (v2, p2) replaces (v, p): it exists and is larger, or equal at a smaller position
__device__ __forceinline__ bool agg_better(float v, int32_t p, float v2, int32_t p2) { return p2 >= 0 && (p < 0 || v2 > v || (v2 == v && p2 < p)); }

// ---- rows: a team per row (short, wave) or per chunk (workgroup) ----
// HEADS: the same walk, slots and fold; the coefficient of a term is the weight of the lane's head, taken per column tile (the tile changes the head)
template <int CLS, int OP, int VEC, bool TR, bool HEADS = false>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_agg_rows(agg_list l, int32_t n, agg_args a)
{
    using T = vgl_rc_team<CLS>;
    static_assert(!(TR && OP == AGG_K_EXT), "every backward is a sum");
    static_assert(!(HEADS && OP == AGG_K_EXT), "heads weigh a sum");
    constexpr int FOLD = T::LANES < 64 ? T::LANES : 64;
    const int lognq = a.lognq[CLS], nq = 1 << lognq, slots = T::LANES >> lognq;
    const int q = T::lane() & (nq - 1), slot = T::lane() >> lognq;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int32_t v = 0;
        int64_t lo = 0, hi = 0, len = 0;
        bool whole = true;
        if (has) {
            v = l.rows[i];
            lo = a.rowptr[v]; hi = a.rowptr[v + 1];
            len = hi - lo;
            if constexpr (CLS == VGL_RC_WG) {
                const int64_t end = hi;
                whole = len <= a.chunk;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        for (int base = 0; base < a.F; base += nq * VEC) {              // the column tiles: the same trips in every lane of the workgroup
            const int c0 = base + q * VEC;
            const bool act = c0 < a.F;
            const int64_t end = act ? hi : lo;                          // a lane past the last column walks nothing
            const int hd = HEADS && act ? c0 / a.D : 0;                 // one division per tile, none per term
            int64_t p = lo + slot;
            if constexpr (OP == AGG_K_SUM) {
                float acc[VEC];
#pragma unroll
                for (int k = 0; k < VEC; k++) acc[k] = 0.0f;
                for (; p + 3 * (int64_t)slots < end; p += 4 * (int64_t)slots) {      // four gathers in flight; the additions keep the row's order
                    int32_t u[4], o[4];
                    float cf[4], t[4][VEC];
#pragma unroll
                    for (int j = 0; j < 4; j++) agg_term<TR, HEADS>(a, p + j * (int64_t)slots, hd, u[j], cf[j], o[j]);
#pragma unroll
                    for (int j = 0; j < 4; j++) agg_values<VEC, TR>(a, u[j], o[j], c0, t[j]);
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int k = 0; k < VEC; k++) acc[k] = acc[k] + cf[j] * t[j][k];
                }
                for (; p < end; p += slots) {
                    int32_t u, o;
                    float cf, t[VEC];
                    agg_term<TR, HEADS>(a, p, hd, u, cf, o);
                    agg_values<VEC, TR>(a, u, o, c0, t);
#pragma unroll
                    for (int k = 0; k < VEC; k++) acc[k] = acc[k] + cf * t[k];
                }
                // the slots of a column group: an xor butterfly inside the wave, then the waves in order
                for (int o = nq; o < FOLD; o <<= 1)
#pragma unroll
                    for (int k = 0; k < VEC; k++) acc[k] = acc[k] + __shfl_xor(acc[k], o);
                if constexpr (CLS == VGL_RC_WG) {
                    __shared__ float s_acc[VGL_WAVES][64 * VEC];
                    __syncthreads();                                    // the sums of the tile before have been read
                    if (vgl_lane() < nq)
#pragma unroll
                        for (int k = 0; k < VEC; k++) s_acc[vgl_wave()][vgl_lane() * VEC + k] = acc[k];
                    __syncthreads();
                    if ((int)threadIdx.x < nq)
#pragma unroll
                        for (int k = 0; k < VEC; k++) {
                            float t = s_acc[0][q * VEC + k];
#pragma unroll
                            for (int w = 1; w < VGL_WAVES; w++) t = t + s_acc[w][q * VEC + k];
                            acc[k] = t;
                        }
                }
                if (slot == 0 && has && act) {
                    if (CLS == VGL_RC_WG && !whole) agg_store<VEC>(a.cpart + i * a.F + c0, acc);
                    else {
                        if (a.mean)
#pragma unroll
                            for (int k = 0; k < VEC; k++) acc[k] = len > 0 ? acc[k] / (float)len : 0.0f;
                        agg_store<VEC>(a.out + (int64_t)v * a.ldo + c0, acc);
                    }
                }
            } else {
                float val[VEC];
                int32_t pos[VEC];
#pragma unroll
                for (int k = 0; k < VEC; k++) { val[k] = 0.0f; pos[k] = -1; }
                for (; p + 3 * (int64_t)slots < end; p += 4 * (int64_t)slots) {      // four gathers in flight; ascending positions, so > keeps the first
                    int32_t u[4];
                    float t[4][VEC];
#pragma unroll
                    for (int j = 0; j < 4; j++) u[j] = a.adj[p + j * (int64_t)slots];
#pragma unroll
                    for (int j = 0; j < 4; j++) agg_load<VEC>(a.x + (int64_t)u[j] * a.ldx + c0, t[j]);
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int k = 0; k < VEC; k++) {
                            const float x = a.neg ? -t[j][k] : t[j][k];
                            if (pos[k] < 0 || x > val[k]) { val[k] = x; pos[k] = (int32_t)(p + j * (int64_t)slots); }
                        }
                }
                for (; p < end; p += slots) {
                    float t[VEC];
                    agg_load<VEC>(a.x + (int64_t)a.adj[p] * a.ldx + c0, t);
#pragma unroll
                    for (int k = 0; k < VEC; k++) {
                        const float x = a.neg ? -t[k] : t[k];
                        if (pos[k] < 0 || x > val[k]) { val[k] = x; pos[k] = (int32_t)p; }
                    }
                }
                for (int o = nq; o < FOLD; o <<= 1)
#pragma unroll
                    for (int k = 0; k < VEC; k++) {
                        const float v2 = __shfl_xor(val[k], o);
                        const int32_t p2 = __shfl_xor(pos[k], o);
                        if (agg_better(val[k], pos[k], v2, p2)) { val[k] = v2; pos[k] = p2; }
                    }
                if constexpr (CLS == VGL_RC_WG) {
                    __shared__ float s_val[VGL_WAVES][64 * VEC];
                    __shared__ int32_t s_pos[VGL_WAVES][64 * VEC];
                    __syncthreads();                                    // the extremes of the tile before have been read
                    if (vgl_lane() < nq)
#pragma unroll
                        for (int k = 0; k < VEC; k++) {
                            s_val[vgl_wave()][vgl_lane() * VEC + k] = val[k];
                            s_pos[vgl_wave()][vgl_lane() * VEC + k] = pos[k];
                        }
                    __syncthreads();
                    if ((int)threadIdx.x < nq)
#pragma unroll
                        for (int k = 0; k < VEC; k++) {
                            val[k] = s_val[0][q * VEC + k]; pos[k] = s_pos[0][q * VEC + k];
#pragma unroll
                            for (int w = 1; w < VGL_WAVES; w++) {
                                const float v2 = s_val[w][q * VEC + k];
                                const int32_t p2 = s_pos[w][q * VEC + k];
                                if (agg_better(val[k], pos[k], v2, p2)) { val[k] = v2; pos[k] = p2; }
                            }
                        }
                }
                if (slot == 0 && has && act) {
                    if (CLS == VGL_RC_WG && !whole) {
                        agg_store<VEC>(a.cpart + i * a.F + c0, val);
                        agg_store<VEC>(a.cpart_arg + i * a.F + c0, pos);
                    } else {
#pragma unroll
                        for (int k = 0; k < VEC; k++) val[k] = pos[k] < 0 ? 0.0f : a.neg ? -val[k] : val[k];
                        agg_store<VEC>(a.out + (int64_t)v * a.ldo + c0, val);
                        if (a.oarg) agg_store<VEC>(a.oarg + (int64_t)v * a.F + c0, pos);
                    }
                }
            }
        }
    }
}

// the rows of more than one chunk: a thread per (row, column) takes the row's chunk results in chunk order and writes the value
struct agg_hubs { const int32_t *row, *first, *nch; int32_t n; };
template <int OP>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_agg_hubs(agg_hubs h, agg_args a)
{
    const int64_t total = (int64_t)h.n * a.F;
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t k = (int32_t)(i / a.F);
        const int c = (int)(i % a.F);
        const int32_t v = h.row[k], nch = h.nch[k];
        const int64_t at = (int64_t)h.first[k] * a.F + c;
        if constexpr (OP == AGG_K_SUM) {
            float acc = a.cpart[at];
            for (int32_t j = 1; j < nch; j++) acc = acc + a.cpart[at + (int64_t)j * a.F];
            if (a.mean) acc = acc / (float)(a.rowptr[v + 1] - a.rowptr[v]);
            a.out[(int64_t)v * a.ldo + c] = acc;
        } else {
            float val = a.cpart[at];
            int32_t pos = a.cpart_arg[at];
            for (int32_t j = 1; j < nch; j++) {
                const float v2 = a.cpart[at + (int64_t)j * a.F];
                const int32_t p2 = a.cpart_arg[at + (int64_t)j * a.F];
                if (agg_better(val, pos, v2, p2)) { val = v2; pos = p2; }
            }
            a.out[(int64_t)v * a.ldo + c] = pos < 0 ? 0.0f : a.neg ? -val : val;
            if (a.oarg) a.oarg[(int64_t)v * a.F + c] = pos;
        }
    }
}

// ---- the small kernels of the plan ----
// the class of a row; a row whose bounds decrease, or a first bound that is not 0, is no item
struct agg_row_src {
    const int64_t *rowptr; vgl_rc_bounds b;
    __device__ __forceinline__ int cls(int64_t v, int64_t &work) const
    {
        const int64_t lo = rowptr[v], hi = rowptr[v + 1];
        if (hi < lo || (v == 0 && lo != 0)) return -1;
        work = hi - lo;
        return vgl_rc_class_of(work, b);
    }
};
// the entries of the rows of each class (the bytes model's walks)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_agg_class_entries(const int64_t *rowptr, int64_t n, vgl_rc_bounds b, unsigned long long *ent)
{
    int64_t e[VGL_RC_N] = {0, 0, 0};
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t d = rowptr[v + 1] - rowptr[v];
        if (d > 0) e[vgl_rc_class_of(d, b)] += d;
    }
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) vgl_wave_flush_add(ent + c, e[c]);
}
// the entries outside [0, n_cols)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_agg_check_adj(const int32_t *adj, int64_t E, int32_t n_cols, unsigned long long *bad)
{
    int64_t b = 0;
    for (int64_t p = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; p < E; p += (int64_t)gridDim.x * VGL_BLOCK) b += adj[p] < 0 || adj[p] >= n_cols ? 1 : 0;
    vgl_wave_flush_add(bad, b);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_agg_lengths(const int32_t *rows, int32_t n, const int64_t *rowptr, int64_t *len)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) len[i] = rowptr[rows[i] + 1] - rowptr[rows[i]];
}
// the transpose's entry list: the row of every entry of the CSR
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_agg_entry_rows(const int64_t *rowptr, int32_t n_rows, int64_t E, int32_t *row)
{
    for (int64_t p = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; p < E; p += (int64_t)gridDim.x * VGL_BLOCK) row[p] = vgl_row_of(rowptr, n_rows, p);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_agg_narrow(const int64_t *in, int64_t n, int32_t *out)
{
    for (int64_t p = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * VGL_BLOCK) out[p] = (int32_t)in[p];
}

// rowptr: n + 1 bounds on the device.  check: a bad rowptr is the caller's (refused by `bad_msg`), else an internal error.
int agg_build_lists(vgl_hip_ctx *c, const char *slot, const int64_t *rowptr, int32_t n, vgl_rc_bounds b, int64_t chunk_env, const char *bad_msg, vgl_agg_lists &L)
{
    hipStream_t st = c->stream;
    vgl_dev<unsigned long long> cnt;
    VGL_TRY(vgl_open_counters(c, &cnt, AC_NCNT));
    if (n > 0) {
        vgl_timed_launch tl(c, slot);
        hipLaunchKernelGGL(vgl_k_agg_class_entries, dim3(vgl_grid(n, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, rowptr, (int64_t)n, b, cnt.p + AC_ENT);
    }
    const agg_row_src src{rowptr, b};
    vgl_rc_lists<vgl_rc_bounded> lists;
    VGL_TRY(lists.count(c, slot, slot, src, n, AGG_MAX_GRID, cnt.p, AC_NCNT, AC_ROWS, AC_BAD, AC_WORK, n, bad_msg, "agg: internal error (the row classes do not add up to the rows)"));
    L.entries = c->h_counters[AC_WORK];
    for (int q = 0; q < VGL_RC_N; q++) { L.rows_of[q] = lists.rows[q]; L.entries_of[q] = c->h_counters[AC_ENT + q]; }
    if (L.entries < 0 || L.entries_of[0] + L.entries_of[1] + L.entries_of[2] != L.entries) VGL_FAIL("agg: internal error (the class entries do not add up)");
    VGL_TRY(L.rows.alloc((size_t)n));
    int64_t nwg = 0;
    if (n > 0) {
        VGL_TRY(lists.fill(c, slot, src, n, AGG_MAX_GRID, 1, nullptr, cnt.p + AC_TAIL));
        // ascending inside a class: the order of the lists is a function of the CSR and the switches, not of the order in which the appends arrived
        vgl_scratch tmp;
        int64_t off = 0;
        for (int q = 0; q < VGL_RC_N; q++) {
            if (lists.rows[q] > 0) {
                vgl_timed_launch tl(c, slot);
                VGL_TRY(vgl_sort_keys(c, tmp, (const int32_t *)lists.l[q].rows, L.rows.p + off, (size_t)lists.rows[q], 0, (unsigned)vgl_index_bits(n)));
            }
            off += lists.rows[q];
        }
        nwg = lists.rows[VGL_RC_WG];
    }
    L.n[VGL_RC_SHORT] = lists.rows[VGL_RC_SHORT];
    L.n[VGL_RC_WAVE] = lists.rows[VGL_RC_WAVE];
    // the chunks of the workgroup rows, on the host: few rows are that long
    std::vector<int32_t> rows((size_t)nwg), item_row, item_chunk, hub_row, hub_first, hub_nch;
    std::vector<int64_t> len((size_t)nwg);
    if (nwg > 0) {
        const int32_t *wg_rows = L.rows.p + lists.rows[0] + lists.rows[1];
        vgl_dev<int64_t> d_len;
        VGL_TRY(d_len.alloc(st, (size_t)nwg));
        {
            vgl_timed_launch tl(c, slot);
            hipLaunchKernelGGL(vgl_k_agg_lengths, dim3(vgl_grid(nwg, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, wg_rows, (int32_t)nwg, rowptr, d_len.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_HIP_TRY(hipMemcpyAsync(rows.data(), wg_rows, sizeof(int32_t) * (size_t)nwg, hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipMemcpyAsync(len.data(), d_len.p, sizeof(int64_t) * (size_t)nwg, hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
    }
    int64_t longest = 0;
    for (int64_t i = 0; i < nwg; i++) {
        if (rows[(size_t)i] < 0 || rows[(size_t)i] >= n || len[(size_t)i] <= b.wave) VGL_FAIL("agg: internal error (a workgroup row is none)");
        longest = std::max(longest, len[(size_t)i]);
    }
    L.ch = vgl_rc_chunks::of(chunk_env, longest);
    for (int64_t i = 0; i < nwg; i++) {
        const int64_t nch = L.ch.pieces(len[(size_t)i]);
        if ((int64_t)item_row.size() + nch > INT32_MAX) VGL_FAIL("agg: the rows have more than 2^31 chunks (raise VGL_AGG_CHUNK)");
        if (nch > 1) {
            hub_row.push_back(rows[(size_t)i]);
            hub_first.push_back((int32_t)item_row.size());
            hub_nch.push_back((int32_t)nch);
        }
        for (int64_t j = 0; j < nch; j++) {
            item_row.push_back(rows[(size_t)i]);
            item_chunk.push_back((int32_t)j);
        }
    }
    L.n[VGL_RC_WG] = (int64_t)item_row.size();
    L.nhubs = (int64_t)hub_row.size();
    auto up = [&](vgl_dev<int32_t> &to, const std::vector<int32_t> &from) -> int {
        VGL_TRY(to.alloc(from.size()));
        if (!from.empty()) VGL_HIP_TRY(hipMemcpyAsync(to.p, from.data(), sizeof(int32_t) * from.size(), hipMemcpyHostToDevice, st));
        return 0;
    };
    VGL_TRY(up(L.item_row, item_row));
    VGL_TRY(up(L.item_chunk, item_chunk));
    VGL_TRY(up(L.hub_row, hub_row));
    VGL_TRY(up(L.hub_first, hub_first));
    VGL_TRY(up(L.hub_nch, hub_nch));
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // (the host vectors and the unsorted lists are free again)
    return 0;
}

}  // namespace

// (declared in vgl_agg.h: edge.hip's transposed entry sum builds the transpose on first use as the transposed runs below do)
int agg_build_transpose(vgl_hip_ctx *c, vgl_hip_agg_plan *p)
{
    hipStream_t st = c->stream;
    const int64_t E = p->E;
    VGL_TRY(p->t_rowptr.alloc((size_t)p->n_cols + 1));
    VGL_TRY(p->t_adj.alloc((size_t)E));
    VGL_TRY(p->t_origin.alloc((size_t)E));
    {
        vgl_dev<int32_t> row;
        vgl_dev<int64_t> perm;
        VGL_TRY(row.alloc(st, (size_t)E));
        VGL_TRY(perm.alloc(st, (size_t)E));
        if (E > 0) {
            vgl_timed_launch tl(c, "agg_transpose");
            hipLaunchKernelGGL(vgl_k_agg_entry_rows, dim3(vgl_grid(E, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, p->rowptr, p->n_rows, E, row.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        {
            // stable: the entries of a transposed row keep their order in the CSR, ascending p
            vgl_timed_launch tl(c, "agg_transpose");
            VGL_TRY(vgl_hip_coo_to_csr(c, p->n_cols, E, p->adj, row.p, 0, p->n_cols, p->t_rowptr.p, p->t_adj.p, perm.p, nullptr));
        }
        if (E > 0) {
            vgl_timed_launch tl(c, "agg_transpose");
            hipLaunchKernelGGL(vgl_k_agg_narrow, dim3(vgl_grid(E, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, (const int64_t *)perm.p, E, p->t_origin.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_HIP_TRY(hipStreamSynchronize(st));
    }
    VGL_TRY(agg_build_lists(c, "agg_transpose", p->t_rowptr.p, p->n_cols, p->b, p->chunk_env, "agg: internal error (the transpose's rowptr decreases)", p->tr));
    if (p->tr.entries != E) VGL_FAIL("agg: internal error (the transpose lost entries)");
    p->has_tr = true;
    return 0;
}

namespace {

template <int OP, int VEC, bool TR, bool HEADS = false>
int agg_pass(vgl_hip_ctx *c, const vgl_agg_lists &L, const agg_args &a)
{
    const char *const slot[VGL_RC_N] = {"agg_short", "agg_wave", "agg_wg"};
    const agg_list list[VGL_RC_N] = {{L.rows.p, nullptr}, {L.rows.p + L.n[0], nullptr}, {L.item_row.p, L.item_chunk.p}};
    VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_agg_rows<VGL_RC_SHORT, OP, VEC, TR, HEADS>, vgl_k_agg_rows<VGL_RC_WAVE, OP, VEC, TR, HEADS>,
                               vgl_k_agg_rows<VGL_RC_WG, OP, VEC, TR, HEADS>, list, a));
    if (L.nhubs > 0) {
        const agg_hubs hubs{L.hub_row.p, L.hub_first.p, L.hub_nch.p, (int32_t)L.nhubs};
        vgl_timed_launch tl(c, "agg_hubs");
        hipLaunchKernelGGL(vgl_k_agg_hubs<OP>, dim3(vgl_grid(L.nhubs * a.F, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream, hubs, a);
    }
    VGL_HIP_TRY(hipGetLastError());
    return 0;
}

// what both runs share once their arguments are checked: the pass over L, the stats
int agg_run(vgl_hip_ctx *c, const vgl_agg_lists &L, bool transposed, int op, agg_args a, int vec, int64_t rows, vgl_hip_agg_stats *stats)
{
    hipStream_t st = c->stream;
    const bool ext = !transposed && (op == VGL_HIP_AGG_MAX || op == VGL_HIP_AGG_MIN);
    int32_t tiles[VGL_RC_N];
    agg_shape(a.F, vec, a.lognq, tiles);
    a.chunk = L.ch.chunk;
    vgl_dev<float> cpart;
    vgl_dev<int32_t> cpart_arg;
    if (L.nhubs > 0) {
        VGL_TRY(cpart.alloc(st, (size_t)L.n[VGL_RC_WG] * (size_t)a.F));
        if (ext) VGL_TRY(cpart_arg.alloc(st, (size_t)L.n[VGL_RC_WG] * (size_t)a.F));
    }
    a.cpart = cpart.p; a.cpart_arg = cpart_arg.p;
    if (a.H > 0) {                                                    // the heads form: SUM or MEAN with E x H weights
        if (transposed) {
            if (vec == 4) VGL_TRY((agg_pass<AGG_K_SUM, 4, true, true>(c, L, a)));
            else VGL_TRY((agg_pass<AGG_K_SUM, 1, true, true>(c, L, a)));
        } else {
            if (vec == 4) VGL_TRY((agg_pass<AGG_K_SUM, 4, false, true>(c, L, a)));
            else VGL_TRY((agg_pass<AGG_K_SUM, 1, false, true>(c, L, a)));
        }
    } else if (ext) {
        if (vec == 4) VGL_TRY((agg_pass<AGG_K_EXT, 4, false>(c, L, a)));
        else VGL_TRY((agg_pass<AGG_K_EXT, 1, false>(c, L, a)));
    } else if (transposed) {
        if (vec == 4) VGL_TRY((agg_pass<AGG_K_SUM, 4, true>(c, L, a)));
        else VGL_TRY((agg_pass<AGG_K_SUM, 1, true>(c, L, a)));
    } else {
        if (vec == 4) VGL_TRY((agg_pass<AGG_K_SUM, 4, false>(c, L, a)));
        else VGL_TRY((agg_pass<AGG_K_SUM, 1, false>(c, L, a)));
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // (the partials are free again; the result is there when the call returns)
    if (stats) {
        vgl_hip_agg_stats s;
        memset(&s, 0, sizeof(s));
        s.rows = rows; s.entries = L.entries;
        s.rows_short = L.rows_of[0]; s.rows_wave = L.rows_of[1]; s.rows_wg = L.rows_of[2];
        s.chunks = L.n[VGL_RC_WG]; s.hub_rows = L.nhubs;
        s.transposed = transposed ? 1 : 0; s.vec = vec; s.heads = a.H;
        const int64_t F = a.F;
        // the model (include/vgl_hip.h has the terms)
        int64_t per_entry = 4 + (a.H > 0 ? 4 * (int64_t)a.H : a.weight ? 4 : 0);
        if (transposed) per_entry += 4 + (a.len_rowptr ? 16 : 0);
        int64_t bytes = 0;
        for (int q = 0; q < VGL_RC_N; q++) { s.column_tiles[q] = tiles[q]; bytes += L.entries_of[q] * tiles[q] * per_entry; }
        bytes += L.entries * 4 * F * (transposed && a.arg ? 2 : 1);
        bytes += rows * (8 + 4 * F + (a.oarg ? 4 * F : 0));
        bytes += 4 * (L.rows_of[0] + L.rows_of[1]) + 8 * L.n[VGL_RC_WG];
        s.algorithmic_bytes = bytes;
        *stats = s;
    }
    return 0;
}

int agg_check_call(const char *who, vgl_hip_ctx *c, vgl_hip_agg_plan *p, int op, const float *d_weight, int32_t F)
{
    static thread_local std::string msg;
    auto fail = [&](const char *what) { msg = std::string(who) + ": " + what; return vgl_set_error(__FILE__, __LINE__, msg.c_str()); };
    if (!c || !p) return fail("null argument");
    if (p->c != c) return fail("the plan belongs to another context");
    if (op < VGL_HIP_AGG_SUM || op > VGL_HIP_AGG_MIN) return fail("op must be VGL_HIP_AGG_SUM, _MEAN, _MAX or _MIN");
    if (d_weight && (op == VGL_HIP_AGG_MAX || op == VGL_HIP_AGG_MIN)) return fail("MAX and MIN take no entry weights");
    if (F < 1) return fail("F must be at least 1");
    return 0;
}

// what the two heads runs refuse beside agg_check_call
int agg_check_heads(const char *who, int op, const float *d_weight, int32_t F, int32_t H)
{
    static thread_local std::string msg;
    auto fail = [&](const char *what) { msg = std::string(who) + ": " + what; return vgl_set_error(__FILE__, __LINE__, msg.c_str()); };
    if (op != VGL_HIP_AGG_SUM && op != VGL_HIP_AGG_MEAN) return fail("op must be VGL_HIP_AGG_SUM or _MEAN");
    if (!d_weight) return fail("d_weight must not be NULL");
    if (H < 1) return fail("H must be at least 1");
    if (F % H != 0) return fail("F must be a multiple of H");
    return 0;
}

}  // namespace

extern "C" {

int vgl_hip_agg_plan_create(vgl_hip_ctx *c, const int64_t *d_rowptr, const int32_t *d_adj, int32_t n_rows, int32_t n_cols, vgl_hip_agg_plan **out)
{
    if (!c || !d_rowptr || !d_adj || !out) VGL_FAIL("agg_plan_create: null argument");
    if (n_rows < 0 || n_cols < 0) VGL_FAIL("agg_plan_create: n_rows and n_cols must not be negative");
    VGL_HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    vgl_building<vgl_hip_agg_plan> p(new vgl_hip_agg_plan(), vgl_synced_delete<vgl_hip_agg_plan>{c});
    p->c = c; p->rowptr = d_rowptr; p->adj = d_adj; p->n_rows = n_rows; p->n_cols = n_cols;
    p->b = vgl_rc_env_bounds(c, "VGL_AGG_SHORT", "VGL_AGG_WAVE");
    p->chunk_env = vgl_rc_env_chunk(c, "VGL_AGG_CHUNK");
    if (n_rows == 0) {
        int64_t first = 0;
        VGL_HIP_TRY(hipMemcpyAsync(&first, d_rowptr, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (first != 0) VGL_FAIL("agg_plan_create: rowptr must start at 0 and must not decrease");
    }
    VGL_TRY(agg_build_lists(c, "agg_prepare", d_rowptr, n_rows, p->b, p->chunk_env, "agg_plan_create: rowptr must start at 0 and must not decrease", p->fwd));
    p->E = p->fwd.entries;
    if (p->E > AGG_MAX_ENTRIES) VGL_FAIL("agg_plan_create: at most 2^31 - 16 entries per plan");
    if (p->E > 0) {
        vgl_dev<unsigned long long> bad;
        VGL_TRY(vgl_open_counters(c, &bad, 1));
        {
            vgl_timed_launch tl(c, "agg_prepare");
            hipLaunchKernelGGL(vgl_k_agg_check_adj, dim3(vgl_grid(p->E, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, d_adj, p->E, n_cols, bad.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(vgl_publish_counters(c, "agg_prepare", bad.p, 1));
        if (c->h_counters[0] != 0) VGL_FAIL("agg_plan_create: an entry of adj is outside [0, n_cols)");
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    *out = p.release();
    return 0;
}

int vgl_hip_agg_plan_info(vgl_hip_agg_plan *p, vgl_hip_agg_stats *stats)
{
    if (!p || !stats) VGL_FAIL("agg_plan_info: null argument");
    vgl_hip_agg_stats s;
    memset(&s, 0, sizeof(s));
    s.rows = p->n_rows; s.entries = p->E;
    s.rows_short = p->fwd.rows_of[0]; s.rows_wave = p->fwd.rows_of[1]; s.rows_wg = p->fwd.rows_of[2];
    s.chunks = p->fwd.n[VGL_RC_WG]; s.hub_rows = p->fwd.nhubs;
    s.transposed = p->has_tr ? 1 : 0;
    *stats = s;
    return 0;
}

int vgl_hip_agg_plan_destroy(vgl_hip_ctx *c, vgl_hip_agg_plan *p)
{
    if (!c) VGL_FAIL("agg_plan_destroy: null argument");
    if (!p) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete p;
    return 0;
}

int vgl_hip_agg_run(vgl_hip_ctx *c, vgl_hip_agg_plan *p, int op, const float *d_weight, const float *d_x, int64_t ldx, int32_t F, float *d_out, int64_t ldo, int32_t *d_arg,
                    vgl_hip_agg_stats *stats)
{
    // every refusal comes before the first write to an output
    VGL_TRY(agg_check_call("agg_run", c, p, op, d_weight, F));
    if (!d_x || !d_out) VGL_FAIL("agg_run: d_x and d_out must not be NULL");
    if (ldx < F || ldo < F) VGL_FAIL("agg_run: a leading dimension must not be below F");
    VGL_HIP_TRY(hipSetDevice(c->device));
    const bool ext = op == VGL_HIP_AGG_MAX || op == VGL_HIP_AGG_MIN;
    agg_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->rowptr; a.adj = p->adj;
    a.weight = d_weight;
    a.x = d_x; a.ldx = ldx; a.out = d_out; a.ldo = ldo;
    a.oarg = ext ? d_arg : nullptr;
    a.F = F;
    a.mean = op == VGL_HIP_AGG_MEAN ? 1 : 0;
    a.neg = op == VGL_HIP_AGG_MIN ? 1 : 0;
    const int vec = F % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && agg_aligned16(d_x) && agg_aligned16(d_out) && (!a.oarg || agg_aligned16(a.oarg)) ? 4 : 1;
    return agg_run(c, p->fwd, false, op, a, vec, p->n_rows, stats);
}

int vgl_hip_agg_run_transposed(vgl_hip_ctx *c, vgl_hip_agg_plan *p, int op, const float *d_weight, const int32_t *d_arg, const float *d_g, int64_t ldg, int32_t F, float *d_gx,
                               int64_t ldgx, vgl_hip_agg_stats *stats)
{
    VGL_TRY(agg_check_call("agg_run_transposed", c, p, op, d_weight, F));
    if (!d_g || !d_gx) VGL_FAIL("agg_run_transposed: d_g and d_gx must not be NULL");
    if (ldg < F || ldgx < F) VGL_FAIL("agg_run_transposed: a leading dimension must not be below F");
    const bool ext = op == VGL_HIP_AGG_MAX || op == VGL_HIP_AGG_MIN;
    if (ext && !d_arg) VGL_FAIL("agg_run_transposed: MAX and MIN need the d_arg of the forward run");
    VGL_HIP_TRY(hipSetDevice(c->device));
    if (!p->has_tr) VGL_TRY(agg_build_transpose(c, p));
    agg_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->t_rowptr.p; a.adj = p->t_adj.p; a.origin = p->t_origin.p;
    a.len_rowptr = op == VGL_HIP_AGG_MEAN ? p->rowptr : nullptr;
    a.weight = d_weight;
    a.arg = ext ? d_arg : nullptr;
    a.x = d_g; a.ldx = ldg; a.out = d_gx; a.ldo = ldgx;
    a.F = F;
    const int vec = F % 4 == 0 && ldg % 4 == 0 && ldgx % 4 == 0 && agg_aligned16(d_g) && agg_aligned16(d_gx) && (!a.arg || agg_aligned16(a.arg)) ? 4 : 1;
    return agg_run(c, p->tr, true, op, a, vec, p->n_cols, stats);
}

int vgl_hip_agg_run_heads(vgl_hip_ctx *c, vgl_hip_agg_plan *p, int op, const float *d_weight, int32_t H, const float *d_x, int64_t ldx, int32_t F, float *d_out, int64_t ldo,
                          vgl_hip_agg_stats *stats)
{
    // every refusal comes before the first write to an output
    VGL_TRY(agg_check_call("agg_run_heads", c, p, op, nullptr, F));
    VGL_TRY(agg_check_heads("agg_run_heads", op, d_weight, F, H));
    if (!d_x || !d_out) VGL_FAIL("agg_run_heads: d_x and d_out must not be NULL");
    if (ldx < F || ldo < F) VGL_FAIL("agg_run_heads: a leading dimension must not be below F");
    VGL_HIP_TRY(hipSetDevice(c->device));
    agg_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->rowptr; a.adj = p->adj;
    a.weight = d_weight; a.H = H; a.D = F / H;
    a.x = d_x; a.ldx = ldx; a.out = d_out; a.ldo = ldo;
    a.F = F;
    a.mean = op == VGL_HIP_AGG_MEAN ? 1 : 0;
    const int vec = a.D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && agg_aligned16(d_x) && agg_aligned16(d_out) ? 4 : 1;
    return agg_run(c, p->fwd, false, op, a, vec, p->n_rows, stats);
}

int vgl_hip_agg_run_transposed_heads(vgl_hip_ctx *c, vgl_hip_agg_plan *p, int op, const float *d_weight, int32_t H, const float *d_g, int64_t ldg, int32_t F, float *d_gx,
                                     int64_t ldgx, vgl_hip_agg_stats *stats)
{
    VGL_TRY(agg_check_call("agg_run_transposed_heads", c, p, op, nullptr, F));
    VGL_TRY(agg_check_heads("agg_run_transposed_heads", op, d_weight, F, H));
    if (!d_g || !d_gx) VGL_FAIL("agg_run_transposed_heads: d_g and d_gx must not be NULL");
    if (ldg < F || ldgx < F) VGL_FAIL("agg_run_transposed_heads: a leading dimension must not be below F");
    VGL_HIP_TRY(hipSetDevice(c->device));
    if (!p->has_tr) VGL_TRY(agg_build_transpose(c, p));
    agg_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->t_rowptr.p; a.adj = p->t_adj.p; a.origin = p->t_origin.p;
    a.len_rowptr = op == VGL_HIP_AGG_MEAN ? p->rowptr : nullptr;
    a.weight = d_weight; a.H = H; a.D = F / H;
    a.x = d_g; a.ldx = ldg; a.out = d_gx; a.ldo = ldgx;
    a.F = F;
    const int vec = a.D % 4 == 0 && ldg % 4 == 0 && ldgx % 4 == 0 && agg_aligned16(d_g) && agg_aligned16(d_gx) ? 4 : 1;
    return agg_run(c, p->tr, true, op, a, vec, p->n_cols, stats);
}

}  // extern "C"
