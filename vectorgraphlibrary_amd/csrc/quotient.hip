// quotient.hip -- the quotient graph of a vertex labelling: the vertices of a class merge into one coarse vertex, the stored entries between two
// classes merge into one coarse entry that carries the sum of their weights (their number without weights).  The row merge next to the row filter of
// subgraph.hip.  The contract is written out in include/vgl_hip.h; DESIGN section 25 has the kernels, their bounds and the bytes model.
//
// Vertex side: one validation pass (negative labels, the largest label), a stable radix sort of (label, vertex) over the bits the largest
// label needs, head flags and their inclusive scan (the coarse id = the rank of the label), a scatter (cluster_of, label_of, member_ptr; the sorted
// vertices ARE `members`) and the sizes.  Per planned direction member_off = the exclusive scan of the members' row lengths in member order: flat
// entry j of coarse row c finds its member by a binary search of member_off within the cluster, the row's volume is a difference of two of its values.
//
// Entry side: coarse rows are classified by volume (vgl_rowclass.h bounds, plus a fourth class) and listed per class; rows of volume 0 are no items.
//   short   8 lanes per row: rank-counting among the gathered coarse far ends, a chunk of 8 in registers at a time, shuffles within the team
//   wave    a wavefront per row, table: a workgroup per row: the far ends staged in LDS, a bitonic sort, an in-place compaction of the distinct keys
//           with the team's rank, then (fill) one LDS int64 sum per distinct key, added to with LDS atomics after a binary search of the key
//   sorted  64-bit keys  c << 32 | c(w)  paired with the weight: a radix sort of pairs + a reduce by key (vgl_prim.h) in pieces of consecutive rows under
//           VGL_QUOT_SORT_CAP_MB (a row above the cap is a piece of its own); the runs of row c are placed at the row's start
// FILL = false counts the distinct entries of every row (a scan makes the rowptr), FILL = true writes adj and count.  Every row has one owner; no atomic
// touches an output array; integer sums only.
#include "vgl_rowclass.h"
#include "vgl_prim.h"
#include <cstring>
#include <algorithm>
#include <vector>

namespace {
constexpr int QUOT_SHORT_CAP = 256;              // 32 chunks of 8: the head flags of a lane's entries are one 32-bit mask
constexpr int QUOT_WAVE_CAP = 1024;              // LDS keys and sums per wavefront row
constexpr int QUOT_TABLE_CAP = 4096;             // ... per workgroup row: 4096 x (4 + 8) bytes = 48 KiB, the same as four wavefront rows
constexpr int QUOT_SORTED = 3;                   // the fourth class
constexpr int64_t QUOT_MAX_GRID = 2048;
constexpr uint32_t QUOT_NONE = 0xffffffffu;      // no entry here (past the row's end, or a dropped loop); sorts behind every coarse id
}  // namespace

struct vgl_hip_quotient_plan {
    vgl_hip_graph *g = nullptr;
    int32_t V = 0, Vc = 0;
    int drop = 0;
    bool planned[2] = {false, false};
    vgl_rc_bounds b = {0, 0};
    int32_t table = 0;
    int64_t cap_keys = 0;                        // keys of one sort piece (INT64_MAX: no cap)
    vgl_dev<int32_t> cluster_of, label_of, size, members;
    vgl_dev<int64_t> member_ptr;
    struct dir {
        vgl_dev<int64_t> member_off, rowptr, soff;       // V + 1; V' + 1; sorted rows + 1 (the exclusive scan of their volumes)
        vgl_rc_lists<vgl_rc_bounded> L;                  // short, wave, table
        vgl_dev<int32_t> srows;                          // the sorted rows, ascending
        int64_t nsorted = 0, piece_keys = 0, entries = 0;
        std::vector<int64_t> soff_h, piece;              // host copy of soff; piece k = sorted rows [piece[k], piece[k + 1])
    } d[2];
    vgl_hip_quotient_stats st;
};

namespace {

enum {
    QC_BAD = 0,         // negative labels
    QC_MAXL = 1,        // the largest label
    QC_VC = 2,          // V'
    QC_ROWS = 3,        // + 4 * direction + class: coarse rows per class
    QC_READ = 11,       // + direction: the sum of the volumes
    QC_SKEYS = 13,      // + direction: ... of the sorted rows
    QC_E = 15,          // + direction: E'
    QC_TAIL = 17,       // + 3 * direction + class: rows appended to the class list so far
    QC_NCNT = 23
};
static_assert(QC_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

bool quot_sharded(const vgl_hip_graph *g) { return g->row_begin != 0 || g->row_end != g->V; }
__host__ __device__ inline int quot_class_of(int64_t vol, vgl_rc_bounds b, int32_t table)
{
    if (vol <= 0) return -1;
    const int k = vgl_rc_class_of(vol, b);
    return k == VGL_RC_WG && vol > table ? QUOT_SORTED : k;
}

// ---- vertex side ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_check(int32_t V, const int32_t *label, unsigned long long *cnt)
{
    int64_t bad = 0;
    int32_t mx = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t l = label[v];
        bad += l < 0;
        mx = l > mx ? l : mx;
    }
    vgl_wave_flush_add(cnt + QC_BAD, bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t x = __shfl_xor(mx, o);
        mx = x > mx ? x : mx;
    }
    if (vgl_lane() == 0 && mx > 0) atomicMax(cnt + QC_MAXL, (unsigned long long)mx);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_heads(int32_t V, const uint32_t *sorted_label, int32_t *head)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < V; i += (int64_t)gridDim.x * VGL_BLOCK)
        head[i] = i == 0 || sorted_label[i] != sorted_label[i - 1];
}
// position i of the sorted order: its vertex joins cluster cid[i] - 1; a head names the cluster's label and first member
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_scatter(int32_t V, int32_t Vc, const uint32_t *sorted_label, const int32_t *members, const int32_t *head, const int32_t *cid,
                                                                int32_t *cluster_of, int32_t *label_of, int64_t *member_ptr)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < V; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t c = cid[i] - 1;
        if (c < 0 || c >= Vc) continue;
        cluster_of[members[i]] = c;
        if (head[i]) {
            label_of[c] = (int32_t)sorted_label[i];
            member_ptr[c] = i;
        }
        if (i == V - 1) member_ptr[Vc] = V;
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_sizes(int32_t Vc, const int64_t *member_ptr, int32_t *size)
{
    for (int64_t c = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; c < Vc; c += (int64_t)gridDim.x * VGL_BLOCK) size[c] = (int32_t)(member_ptr[c + 1] - member_ptr[c]);
}
// len[i] = the row length of member i, len[V] = 0
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_member_len(int32_t V, const int32_t *members, const int64_t *rowptr, int64_t *len)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i <= V; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t v = i < V ? members[i] : 0;
        len[i] = i < V ? rowptr[v + 1] - rowptr[v] : 0;
    }
}

// ---- the coarse rows of a direction ----
struct quot_row { int64_t m0, m1, base, vol; int32_t c; };
struct quot_view {
    int32_t Vc;
    int drop;
    const int64_t *rowptr;       // the parent's, of this direction
    const int32_t *adj;
    const int32_t *cluster_of, *members;
    const int64_t *member_ptr, *member_off;
    __device__ __forceinline__ int64_t vol_of(int64_t c) const { return member_off[member_ptr[c + 1]] - member_off[member_ptr[c]]; }
    __device__ __forceinline__ quot_row row_of(int32_t c) const
    {
        const int64_t m0 = member_ptr[c], m1 = member_ptr[c + 1], base = member_off[m0];
        return quot_row{m0, m1, base, member_off[m1] - base, c};
    }
    // the coarse far end of flat entry j < vol of the row (QUOT_NONE for a dropped loop) and its position p in the parent's adjacency
    __device__ __forceinline__ uint32_t key(const quot_row &r, int64_t j, int64_t &p) const
    {
        const int64_t f = r.base + j;
        int64_t lo = r.m0, hi = r.m1;                                 // invariant: member_off[lo] <= f < member_off[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (member_off[mid] <= f) lo = mid; else hi = mid;
        }
        p = rowptr[members[lo]] + (f - member_off[lo]);
        const int32_t k = cluster_of[adj[p]];
        return drop && k == r.c ? QUOT_NONE : (uint32_t)k;
    }
};
struct quot_two { int32_t Vc; const int64_t *member_ptr; const int64_t *member_off[2]; vgl_rc_bounds b; int32_t table; };
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_classify(quot_two s, unsigned long long *cnt)
{
    int64_t rows[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, read[2] = {0, 0}, skeys[2] = {0, 0};
    for (int64_t c = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; c < s.Vc; c += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t m0 = s.member_ptr[c], m1 = s.member_ptr[c + 1];
#pragma unroll
        for (int d = 0; d < 2; d++)
            if (s.member_off[d]) {
                const int64_t vol = s.member_off[d][m1] - s.member_off[d][m0];
                const int k = quot_class_of(vol, s.b, s.table);
#pragma unroll
                for (int q = 0; q < 4; q++) rows[d][q] += k == q;
                read[d] += vol;
                skeys[d] += k == QUOT_SORTED ? vol : 0;
            }
    }
#pragma unroll
    for (int d = 0; d < 2; d++) {
#pragma unroll
        for (int q = 0; q < 4; q++) vgl_wave_flush_add(cnt + QC_ROWS + 4 * d + q, rows[d][q]);
        vgl_wave_flush_add(cnt + QC_READ + d, read[d]);
        vgl_wave_flush_add(cnt + QC_SKEYS + d, skeys[d]);
    }
}
// the class-list builder's source: coarse row i into the short, wave or table list; rows of volume 0 and sorted rows are no items of it
struct quot_src {
    const int64_t *member_ptr, *member_off;
    vgl_rc_bounds b;
    int32_t table;
    __device__ __forceinline__ int cls(int64_t i, int64_t &work) const
    {
        work = member_off[member_ptr[i + 1]] - member_off[member_ptr[i]];
        const int k = quot_class_of(work, b, table);
        return k == QUOT_SORTED ? -1 : k;
    }
};
// the sorted rows in ascending order: flags (V' + 1, the last 0), their exclusive scan, the scatter
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_sorted_flag(quot_src s, int32_t Vc, int32_t *flag)
{
    for (int64_t c = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; c <= Vc; c += (int64_t)gridDim.x * VGL_BLOCK) {
        int64_t vol = 0;
        flag[c] = c < Vc && quot_class_of(vol = s.member_off[s.member_ptr[c + 1]] - s.member_off[s.member_ptr[c]], s.b, s.table) == QUOT_SORTED;
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_sorted_list(quot_src s, int32_t Vc, const int32_t *flag, const int32_t *pos, int64_t nsorted, int32_t *srows, int64_t *svol)
{
    for (int64_t c = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; c < Vc; c += (int64_t)gridDim.x * VGL_BLOCK)
        if (flag[c] && pos[c] >= 0 && pos[c] < nsorted) {
            srows[pos[c]] = (int32_t)c;
            svol[pos[c]] = s.member_off[s.member_ptr[c + 1]] - s.member_off[s.member_ptr[c]];
        }
}

// ---- the LDS classes: FILL = false counts the distinct coarse far ends of every listed row, FILL = true writes them ascending with their sums ----
struct quot_out {
    int64_t *cnt_row;            // counting: by coarse row
    const int64_t *rowptr;       // filling: the coarse row starts; a position at or past the row's end is never stored to
    int32_t *adj;
    int64_t *count;
    const int64_t *weight;       // per stored entry of the direction; nullptr: 1 each
};
template <int CLS>
__device__ __forceinline__ void quot_team_sync()
{
    if constexpr (CLS == VGL_RC_WG) __syncthreads();
    else {                                                            // one wavefront: its LDS operations complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}
template <int CLS, bool FILL>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot(const int32_t *list, int32_t n, quot_view a, quot_out o)
{
    using T = vgl_rc_team<CLS>;
    if constexpr (CLS == VGL_RC_SHORT) {
        for (int64_t at0 = T::begin(); at0 < n; at0 += T::stride()) {
            const int64_t i = T::item(at0);
            const bool has = i < n;
            quot_row r{0, 0, 0, 0, 0};
            if (has) r = a.row_of(list[i]);
            if (r.vol > QUOT_SHORT_CAP) r.vol = 0;                    // (never: the bound is clamped on the host)
            const int nch = (int)((r.vol + T::LANES - 1) / T::LANES);
            // an entry is a head when no equal key sits at an earlier flat position
            uint32_t headmask = 0;
            int heads = 0;
            for (int ca = 0; T::together(ca < nch); ca++) {
                const int64_t j = (int64_t)ca * T::LANES + T::lane();
                int64_t p = 0;
                const uint32_t mine = j < r.vol ? a.key(r, j, p) : QUOT_NONE;
                bool head = mine != QUOT_NONE;
                for (int cb = 0; cb <= ca; cb++) {                    // (uniform over the wave)
                    const int64_t jb = (int64_t)cb * T::LANES + T::lane();
                    const uint32_t kb = cb == ca ? mine : jb < r.vol ? a.key(r, jb, p) : QUOT_NONE;
#pragma unroll
                    for (int l = 0; l < T::LANES; l++) {
                        const uint32_t other = __shfl(kb, l, T::LANES);
                        if (other == mine && (int64_t)cb * T::LANES + l < j) head = false;
                    }
                }
                if (head) headmask |= 1u << ca;
                int tot = 0;
                (void)T::rank(head, &tot);
                heads += tot;
            }
            if (!FILL) {
                if (T::lead() && has) o.cnt_row[r.c] = heads;
                continue;                                             // (uniform over the workgroup)
            }
            // the output position of a head is the number of heads with a smaller key, its count the sum over equal keys
            const int64_t at = has ? o.rowptr[r.c] : 0, end = has ? o.rowptr[r.c + 1] : 0;
            for (int ca = 0; T::together(ca < nch); ca++) {
                const int64_t j = (int64_t)ca * T::LANES + T::lane();
                int64_t p = 0;
                const uint32_t mine = j < r.vol ? a.key(r, j, p) : QUOT_NONE;
                int64_t pos = 0, sum = 0;
                for (int cb = 0; T::together(cb < nch); cb++) {
                    const int64_t jb = (int64_t)cb * T::LANES + T::lane();
                    int64_t pb = 0;
                    const uint32_t kb = jb < r.vol ? a.key(r, jb, pb) : QUOT_NONE;
                    const int64_t wb = kb == QUOT_NONE ? 0 : o.weight ? o.weight[pb] : 1;
                    const int hb = (headmask >> cb) & 1u;
#pragma unroll
                    for (int l = 0; l < T::LANES; l++) {
                        const uint32_t other = __shfl(kb, l, T::LANES);
                        const int oh = __shfl(hb, l, T::LANES);
                        const int64_t ow = __shfl(wb, l, T::LANES);
                        pos += oh && other < mine;
                        sum += other == mine ? ow : 0;
                    }
                }
                if (((headmask >> ca) & 1u) && at + pos < end) {
                    o.adj[at + pos] = (int32_t)mine;
                    o.count[at + pos] = sum;
                }
            }
        }
    } else {
        constexpr int CAP = CLS == VGL_RC_WAVE ? QUOT_WAVE_CAP : QUOT_TABLE_CAP;
        __shared__ uint32_t s_keys[T::ITEMS_PER_WG][CAP];
        __shared__ int64_t s_sum[T::ITEMS_PER_WG][CAP];
        uint32_t *K = s_keys[T::team()];
        int64_t *S = s_sum[T::team()];
        for (int64_t i = T::begin(); i < n; i += T::stride()) {       // (uniform over the team)
            quot_row r = a.row_of(list[i]);
            if (r.vol > CAP) r.vol = 0;                               // (never: the bounds are clamped on the host)
            int P = 1;
            while (P < r.vol) P <<= 1;
            quot_team_sync<CLS>();                                    // the item before has been written out
            for (int x = T::lane(); x < P; x += T::LANES) {
                int64_t p = 0;
                K[x] = x < r.vol ? a.key(r, x, p) : QUOT_NONE;
            }
            quot_team_sync<CLS>();
            for (int k = 2; k <= P; k <<= 1)                          // bitonic sort, ascending: QUOT_NONE ends up behind the coarse ids
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int x = T::lane(); x < P; x += T::LANES) {
                        const int y = x ^ j;
                        if (y > x) {
                            const uint32_t kx = K[x], ky = K[y];
                            if ((kx > ky) == ((x & k) == 0)) { K[x] = ky; K[y] = kx; }
                        }
                    }
                    quot_team_sync<CLS>();
                }
            // the distinct keys move to K[0, d) in order: a head at x goes to a slot <= x, and only to x itself when nothing before it was dropped
            int d = 0;
            for (int x0 = 0; x0 < P; x0 += T::LANES) {                // (uniform over the team)
                const int x = x0 + T::lane();
                const uint32_t kx = x < P ? K[x] : QUOT_NONE;
                const bool head = kx != QUOT_NONE && (x == 0 || K[x - 1] != kx);
                quot_team_sync<CLS>();
                int tot = 0;
                const int rank = T::rank(head, &tot);
                if (head) K[d + rank] = kx;
                d += tot;
                quot_team_sync<CLS>();
            }
            if (!FILL) {
                if (T::lead()) o.cnt_row[r.c] = d;
                continue;                                             // (uniform over the team)
            }
            for (int x = T::lane(); x < d; x += T::LANES) S[x] = 0;
            quot_team_sync<CLS>();
            for (int64_t j = T::lane(); j < r.vol; j += T::LANES) {
                int64_t p = 0;
                const uint32_t kj = a.key(r, j, p);
                if (kj == QUOT_NONE) continue;
                int lo = 0, hi = d;                                   // the first slot whose key is not below kj
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (K[mid] < kj) lo = mid + 1; else hi = mid;
                }
                if (lo < d) atomicAdd(reinterpret_cast<unsigned long long *>(S + lo), (unsigned long long)(o.weight ? o.weight[p] : 1));
            }
            quot_team_sync<CLS>();
            const int64_t at = o.rowptr[r.c], end = o.rowptr[r.c + 1];
            for (int x = T::lane(); x < d; x += T::LANES)
                if (at + x < end) {
                    o.adj[at + x] = (int32_t)K[x];
                    o.count[at + x] = S[x];
                }
        }
    }
}
const int64_t quot_grid_cap[VGL_RC_N] = {4 * QUOT_MAX_GRID, 4 * QUOT_MAX_GRID, 4 * QUOT_MAX_GRID};
template <bool FILL>
int quot_launch(vgl_hip_ctx *c, const vgl_hip_quotient_plan *p, int d, const quot_view &a, const quot_out &o)
{
    const char *const count_slot[VGL_RC_N] = {"quot_count_short", "quot_count_wave", "quot_count_table"};
    const char *const fill_slot[VGL_RC_N] = {"quot_fill_short", "quot_fill_wave", "quot_fill_table"};
    const vgl_rc_lists<vgl_rc_bounded> &L = p->d[d].L;
    const int32_t *const list[VGL_RC_N] = {L.l[0].rows, L.l[1].rows, L.l[2].rows};
    return vgl_rc_launch_trio(c, FILL ? fill_slot : count_slot, L.rows, quot_grid_cap, vgl_k_quot<VGL_RC_SHORT, FILL>, vgl_k_quot<VGL_RC_WAVE, FILL>, vgl_k_quot<VGL_RC_WG, FILL>, list, a,
                              o);
}
quot_view quot_view_of(const vgl_hip_quotient_plan *p, int d)
{
    const vgl_dir_csr &csr = d == 0 ? p->g->out : p->g->in;
    return quot_view{p->Vc, p->drop, csr.rowptr, csr.adj, p->cluster_of.p, p->members.p, p->member_ptr.p, p->d[d].member_off.p};
}

// ---- the sorted class ----
// key t of the piece: flat entry f0 + t of the sorted rows [i0, i1); a dropped loop becomes the key of row V', which no output row has
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_emit(quot_view a, const int32_t *srows, const int64_t *soff, int64_t i0, int64_t i1, int64_t nk, const int64_t *weight,
                                                             uint64_t *keys, int64_t *vals)
{
    const int64_t f0 = soff[i0];
    for (int64_t t = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; t < nk; t += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t f = f0 + t;
        int64_t lo = i0, hi = i1;                                     // invariant: soff[lo] <= f < soff[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (soff[mid] <= f) lo = mid; else hi = mid;
        }
        const quot_row r = a.row_of(srows[lo]);
        int64_t p = 0;
        const uint32_t k = a.key(r, f - soff[lo], p);
        keys[t] = k == QUOT_NONE ? (uint64_t)a.Vc << 32 : ((uint64_t)r.c << 32 | k);
        vals[t] = k == QUOT_NONE ? 0 : weight ? weight[p] : 1;
    }
}
// the distinct keys of a piece, ascending: FILL = false stores the number of keys of every row (by the row's last key), FILL = true every key and sum
template <bool FILL>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_quot_place(const uint64_t *ukeys, const int64_t *usums, const int64_t *n_unique, int64_t nk, int32_t Vc, quot_out o)
{
    const int64_t n = *n_unique < nk ? *n_unique : nk;
    for (int64_t t = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; t < n; t += (int64_t)gridDim.x * VGL_BLOCK) {
        const uint64_t key = ukeys[t];
        const int64_t r = (int64_t)(key >> 32);
        if (r >= Vc) continue;
        if (!FILL && t + 1 < n && (int64_t)(ukeys[t + 1] >> 32) == r) continue;
        int64_t lo = 0, hi = t;                                       // the first key of row r
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if ((int64_t)(ukeys[mid] >> 32) < r) lo = mid + 1; else hi = mid;
        }
        if (!FILL) o.cnt_row[r] = t + 1 - lo;
        else {
            const int64_t pos = o.rowptr[r] + (t - lo);
            if (pos < o.rowptr[r + 1]) {
                o.adj[pos] = (int32_t)(uint32_t)key;
                o.count[pos] = usums[t];
            }
        }
    }
}
template <bool FILL>
int quot_sorted(vgl_hip_ctx *c, const vgl_hip_quotient_plan *p, int d, const quot_out &o)
{
    const vgl_hip_quotient_plan::dir &D = p->d[d];
    if (D.nsorted == 0) return 0;
    hipStream_t st = c->stream;
    const char *slot = FILL ? "quot_fill_sorted" : "quot_count_sorted";
    const size_t cap = (size_t)std::max<int64_t>(D.piece_keys, 1);
    const int end_bit = 32 + vgl_key_bits((uint64_t)p->Vc);         // (the row of a dropped loop's key is V' itself)
    vgl_dev<uint64_t> keys_a, keys_b;
    vgl_dev<int64_t> vals_a, vals_b, n_unique;
    vgl_scratch temp;                                                 // sized for the largest piece here: the loop allocates nothing
    VGL_TRY(keys_a.alloc(st, cap));
    VGL_TRY(keys_b.alloc(st, cap));
    VGL_TRY(vals_a.alloc(st, cap));
    VGL_TRY(vals_b.alloc(st, cap));
    VGL_TRY(n_unique.alloc(st, 1));
    VGL_TRY(vgl_sort_pairs(c, temp, keys_a.p, keys_b.p, vals_a.p, vals_b.p, cap, 0, end_bit, VGL_SIZE_ONLY));
    VGL_TRY(vgl_reduce_by_key(c, temp, keys_b.p, vals_b.p, cap, keys_a.p, vals_a.p, n_unique.p, VGL_SIZE_ONLY));
    const quot_view a = quot_view_of(p, d);
    for (size_t k = 0; k + 1 < D.piece.size(); k++) {
        const int64_t i0 = D.piece[k], i1 = D.piece[k + 1], nk = D.soff_h[(size_t)i1] - D.soff_h[(size_t)i0];
        if (nk <= 0 || nk > (int64_t)cap) VGL_FAIL("quotient: internal error (a sort piece does not fit its buffers)");
        vgl_timed_launch tl(c, slot);
        hipLaunchKernelGGL(vgl_k_quot_emit, dim3(vgl_grid(nk, VGL_BLOCK, 4 * QUOT_MAX_GRID)), dim3(VGL_BLOCK), 0, st, a, (const int32_t *)D.srows.p, (const int64_t *)D.soff.p, i0, i1, nk,
                           o.weight, keys_a.p, vals_a.p);
        VGL_TRY(vgl_sort_pairs(c, temp, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (size_t)nk, 0, end_bit));
        VGL_TRY(vgl_reduce_by_key(c, temp, keys_b.p, vals_b.p, (size_t)nk, keys_a.p, vals_a.p, n_unique.p));
        hipLaunchKernelGGL(vgl_k_quot_place<FILL>, dim3(vgl_grid(nk, VGL_BLOCK, 4 * QUOT_MAX_GRID)), dim3(VGL_BLOCK), 0, st, (const uint64_t *)keys_a.p, (const int64_t *)vals_a.p,
                           (const int64_t *)n_unique.p, nk, p->Vc, o);
        VGL_HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int vgl_hip_quotient_plan_create(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *d_label, int drop_loops, vgl_hip_quotient_plan **out)
{
    if (!c || !g || !d_label || !out) VGL_FAIL("quotient_plan_create: null argument");
    if (quot_sharded(g)) VGL_FAIL("quotient_plan_create: graph handle must own all rows (the quotient has no sharded form)");
    const int32_t V = g->V;
    if (V < 1) VGL_FAIL("quotient_plan_create: the graph has no vertex");
    hipStream_t st = c->stream;
    vgl_building<vgl_hip_quotient_plan> p(new vgl_hip_quotient_plan(), vgl_synced_delete<vgl_hip_quotient_plan>{c});
    p->g = g;
    p->V = V;
    p->drop = drop_loops != 0;
    p->b.shrt = (int32_t)vgl_env_int(c, "VGL_QUOT_SHORT", 32, 0, QUOT_SHORT_CAP);
    p->b.wave = (int32_t)vgl_env_int(c, "VGL_QUOT_WAVE", QUOT_WAVE_CAP, p->b.shrt, QUOT_WAVE_CAP);
    p->table = (int32_t)vgl_env_int(c, "VGL_QUOT_TABLE", QUOT_TABLE_CAP, p->b.wave, QUOT_TABLE_CAP);
    const int64_t cap_mb = vgl_env_int(c, "VGL_QUOT_SORT_CAP_MB", 4096, 0, (int64_t)1 << 24);
    p->cap_keys = cap_mb == 0 ? INT64_MAX : (cap_mb << 20) / 32;      // keys in and out, sums in and out: 32 bytes per key
    p->planned[0] = true;
    p->planned[1] = g->in.rowptr != nullptr;
    memset(&p->st, 0, sizeof(p->st));
    const unsigned grid_v = vgl_grid(V, VGL_BLOCK, QUOT_MAX_GRID);

    vgl_dev<unsigned long long> cnt;
    VGL_TRY(vgl_open_counters(c, &cnt, QC_NCNT));
    {
        vgl_timed_launch tl(c, "quot_check");
        hipLaunchKernelGGL(vgl_k_quot_check, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, d_label, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_publish_counters(c, "quot_publish", cnt, QC_NCNT));
    if (c->h_counters[QC_BAD] != 0) VGL_FAIL("quotient_plan_create: a label is negative");
    const int end_bit = vgl_key_bits((uint64_t)c->h_counters[QC_MAXL]);

    // the stable sort of (label, vertex); the sorted vertices are `members`
    vgl_dev<uint32_t> sorted_label;
    vgl_dev<int32_t> ids, head, cid;
    VGL_TRY(sorted_label.alloc(st, (size_t)V));
    VGL_TRY(ids.alloc(st, (size_t)V));
    VGL_TRY(head.alloc(st, (size_t)V));
    VGL_TRY(cid.alloc(st, (size_t)V));
    VGL_TRY(p->members.alloc(st, (size_t)V));
    VGL_TRY(p->cluster_of.alloc(st, (size_t)V));
    {
        const uint32_t *keys_in = reinterpret_cast<const uint32_t *>(d_label);
        vgl_scratch temp;
        VGL_TRY(vgl_sort_pairs(c, temp, keys_in, sorted_label.p, ids.p, p->members.p, (size_t)V, 0, end_bit, VGL_SIZE_ONLY));
        VGL_TRY(vgl_inclusive_scan(c, temp, head.p, cid.p, (size_t)V, VGL_SIZE_ONLY));
        vgl_timed_launch tl(c, "quot_vertex");
        hipLaunchKernelGGL(vgl_k_iota, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, ids.p);
        VGL_TRY(vgl_sort_pairs(c, temp, keys_in, sorted_label.p, ids.p, p->members.p, (size_t)V, 0, end_bit));
        hipLaunchKernelGGL(vgl_k_quot_heads, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const uint32_t *)sorted_label.p, head.p);
        VGL_TRY(vgl_inclusive_scan(c, temp, head.p, cid.p, (size_t)V));
        VGL_HIP_TRY(hipMemcpyAsync(cnt.p + QC_VC, cid.p + (V - 1), sizeof(int32_t), hipMemcpyDeviceToDevice, st));      // (the slot's upper half stays 0)
        VGL_HIP_TRY(hipGetLastError());
    }
    VGL_TRY(vgl_publish_counters(c, "quot_publish", cnt, QC_NCNT));
    const int64_t Vc = c->h_counters[QC_VC];
    if (Vc < 1 || Vc > V) VGL_FAIL("quotient_plan_create: internal error (the clusters exceed V)");
    p->Vc = (int32_t)Vc;
    const unsigned grid_c = vgl_grid(Vc, VGL_BLOCK, QUOT_MAX_GRID);
    VGL_TRY(p->label_of.alloc(st, (size_t)Vc));
    VGL_TRY(p->size.alloc(st, (size_t)Vc));
    VGL_TRY(p->member_ptr.alloc(st, (size_t)Vc + 1));
    {
        vgl_timed_launch tl(c, "quot_vertex");
        hipLaunchKernelGGL(vgl_k_quot_scatter, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (int32_t)Vc, (const uint32_t *)sorted_label.p, (const int32_t *)p->members.p,
                           (const int32_t *)head.p, (const int32_t *)cid.p, p->cluster_of.p, p->label_of.p, p->member_ptr.p);
        hipLaunchKernelGGL(vgl_k_quot_sizes, dim3(grid_c), dim3(VGL_BLOCK), 0, st, (int32_t)Vc, (const int64_t *)p->member_ptr.p, p->size.p);
    }
    VGL_HIP_TRY(hipGetLastError());

    // member_off per planned direction, then the classes of both directions in one pass
    vgl_dev<int64_t> scratch;                                         // V + 1: row lengths in member order, later the counts per coarse row
    VGL_TRY(scratch.alloc(st, (size_t)V + 1));
    for (int d = 0; d < 2; d++) {
        if (!p->planned[d]) continue;
        const vgl_dir_csr &csr = d == 0 ? g->out : g->in;
        VGL_TRY(p->d[d].member_off.alloc(st, (size_t)V + 1));
        {
            vgl_timed_launch tl(c, "quot_member_off");
            hipLaunchKernelGGL(vgl_k_quot_member_len, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)p->members.p, csr.rowptr, scratch.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        vgl_scratch tmp;
        VGL_TRY(vgl_exclusive_scan(c, tmp, scratch.p, p->d[d].member_off.p, (size_t)V + 1, VGL_SIZE_ONLY));
        vgl_timed_launch tl(c, "quot_member_off");
        VGL_TRY(vgl_exclusive_scan(c, tmp, scratch.p, p->d[d].member_off.p, (size_t)V + 1));
    }
    {
        const quot_two two{(int32_t)Vc, p->member_ptr.p, {p->d[0].member_off.p, p->planned[1] ? p->d[1].member_off.p : nullptr}, p->b, p->table};
        vgl_timed_launch tl(c, "quot_classify");
        hipLaunchKernelGGL(vgl_k_quot_classify, dim3(grid_c), dim3(VGL_BLOCK), 0, st, two, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_publish_counters(c, "quot_publish", cnt, QC_NCNT));
    vgl_hip_quotient_stats &s = p->st;
    s.vertices = Vc;
    int64_t rows[2][4], read[2], skeys[2];
    for (int d = 0; d < 2; d++) {
        for (int q = 0; q < 4; q++) rows[d][q] = c->h_counters[QC_ROWS + 4 * d + q];
        read[d] = c->h_counters[QC_READ + d];
        skeys[d] = c->h_counters[QC_SKEYS + d];
        int64_t total = 0;
        for (int q = 0; q < 4; q++) {
            if (rows[d][q] < 0) VGL_FAIL("quotient_plan_create: internal error (a class count is negative)");
            total += rows[d][q];
        }
        if (total > Vc || (!p->planned[d] && total != 0)) VGL_FAIL("quotient_plan_create: internal error (the classes exceed the coarse rows)");
    }
    s.rows_short_out = rows[0][0]; s.rows_wave_out = rows[0][1]; s.rows_table_out = rows[0][2]; s.rows_sorted_out = rows[0][3];
    s.rows_short_in = rows[1][0]; s.rows_wave_in = rows[1][1]; s.rows_table_in = rows[1][2]; s.rows_sorted_in = rows[1][3];
    s.entries_read_out = read[0]; s.entries_read_in = read[1];
    s.sorted_keys_out = skeys[0]; s.sorted_keys_in = skeys[1];

    for (int d = 0; d < 2; d++) {
        if (!p->planned[d]) continue;
        vgl_hip_quotient_plan::dir &D = p->d[d];
        const quot_src src{p->member_ptr.p, D.member_off.p, p->b, p->table};
        for (int q = 0; q < VGL_RC_N; q++) D.L.rows[q] = rows[d][q];
        VGL_TRY(D.L.fill(c, "quot_lists", src, Vc, QUOT_MAX_GRID, 1, nullptr, cnt + QC_TAIL + 3 * d));
        D.nsorted = rows[d][QUOT_SORTED];
        if (D.nsorted > 0) {
            vgl_dev<int32_t> flag, pos;
            vgl_dev<int64_t> svol;
            VGL_TRY(flag.alloc(st, (size_t)Vc + 1));
            VGL_TRY(pos.alloc(st, (size_t)Vc + 1));
            VGL_TRY(svol.alloc(st, (size_t)D.nsorted + 1));
            VGL_TRY(D.srows.alloc(st, (size_t)D.nsorted));
            VGL_TRY(D.soff.alloc(st, (size_t)D.nsorted + 1));
            {
                vgl_timed_launch tl(c, "quot_lists");
                hipLaunchKernelGGL(vgl_k_quot_sorted_flag, dim3(grid_c), dim3(VGL_BLOCK), 0, st, src, (int32_t)Vc, flag.p);
            }
            {
                vgl_scratch tmp;
                VGL_TRY(vgl_exclusive_scan(c, tmp, flag.p, pos.p, (size_t)Vc + 1, VGL_SIZE_ONLY));
                vgl_timed_launch tl(c, "quot_lists");
                VGL_TRY(vgl_exclusive_scan(c, tmp, flag.p, pos.p, (size_t)Vc + 1));
            }
            VGL_HIP_TRY(hipMemsetAsync(svol.p + D.nsorted, 0, sizeof(int64_t), st));
            {
                vgl_timed_launch tl(c, "quot_lists");
                hipLaunchKernelGGL(vgl_k_quot_sorted_list, dim3(grid_c), dim3(VGL_BLOCK), 0, st, src, (int32_t)Vc, (const int32_t *)flag.p, (const int32_t *)pos.p, D.nsorted, D.srows.p,
                                   svol.p);
            }
            VGL_HIP_TRY(hipGetLastError());
            {
                vgl_scratch tmp;
                VGL_TRY(vgl_exclusive_scan(c, tmp, svol.p, D.soff.p, (size_t)D.nsorted + 1, VGL_SIZE_ONLY));
                vgl_timed_launch tl(c, "quot_lists");
                VGL_TRY(vgl_exclusive_scan(c, tmp, svol.p, D.soff.p, (size_t)D.nsorted + 1));
            }
            // the pieces: consecutive sorted rows under the cap; a row above the cap is a piece of its own
            D.soff_h.assign((size_t)D.nsorted + 1, 0);
            VGL_HIP_TRY(hipMemcpyAsync(D.soff_h.data(), D.soff.p, sizeof(int64_t) * ((size_t)D.nsorted + 1), hipMemcpyDeviceToHost, st));
            VGL_HIP_TRY(hipStreamSynchronize(st));
            if (D.soff_h[(size_t)D.nsorted] != skeys[d]) VGL_FAIL("quotient_plan_create: internal error (the sorted volumes do not add up)");
            D.piece_keys = vgl_plan_pieces(D.nsorted, [&](int64_t i) { return D.soff_h[(size_t)i + 1] - D.soff_h[(size_t)i]; }, p->cap_keys, &D.piece);
        }
        (d == 0 ? s.sort_pieces_out : s.sort_pieces_in) = D.nsorted > 0 ? (int64_t)D.piece.size() - 1 : 0;
        // the distinct entries of every coarse row, then the rowptr
        VGL_TRY(D.rowptr.alloc(st, (size_t)Vc + 1));
        VGL_HIP_TRY(hipMemsetAsync(scratch.p, 0, sizeof(int64_t) * ((size_t)Vc + 1), st));      // (rows of volume 0 have no owner)
        const quot_out o{scratch.p, nullptr, nullptr, nullptr, nullptr};
        VGL_TRY(quot_launch<false>(c, p.get(), d, quot_view_of(p.get(), d), o));
        VGL_TRY(quot_sorted<false>(c, p.get(), d, o));
        {
            vgl_scratch tmp;
            VGL_TRY(vgl_exclusive_scan(c, tmp, scratch.p, D.rowptr.p, (size_t)Vc + 1, VGL_SIZE_ONLY));
            vgl_timed_launch tl(c, "quot_scan");
            VGL_TRY(vgl_exclusive_scan(c, tmp, scratch.p, D.rowptr.p, (size_t)Vc + 1));
        }
        VGL_HIP_TRY(hipMemcpyAsync(cnt.p + QC_E + d, D.rowptr.p + Vc, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    }
    VGL_TRY(vgl_publish_counters(c, "quot_publish", cnt, QC_NCNT));
    for (int d = 0; d < 2; d++) {
        p->d[d].entries = p->planned[d] ? c->h_counters[QC_E + d] : 0;
        if (p->d[d].entries < 0 || p->d[d].entries > read[d]) VGL_FAIL("quotient_plan_create: internal error (more coarse entries than stored entries)");
    }
    s.entries_out = p->d[0].entries;
    s.entries_in = p->d[1].entries;
    s.algorithmic_bytes = 32 * (int64_t)V + 8 * Vc + 8 * (Vc + 1);
    for (int d = 0; d < 2; d++)
        if (p->planned[d]) s.algorithmic_bytes += 28 * (int64_t)V + 40 * (Vc + 1) + 16 * read[d] + 12 * p->d[d].entries;
    VGL_HIP_TRY(hipStreamSynchronize(st));
    *out = p.release();
    return 0;
}

int vgl_hip_quotient_plan_info(vgl_hip_quotient_plan *p, int32_t *vertices, int64_t *out_entries, int64_t *in_entries, vgl_hip_quotient_stats *stats)
{
    if (!p) VGL_FAIL("quotient_plan_info: null argument");
    if (vertices) *vertices = p->Vc;
    if (out_entries) *out_entries = p->d[0].entries;
    if (in_entries) *in_entries = p->planned[1] ? p->d[1].entries : -1;
    if (stats) *stats = p->st;
    return 0;
}

int vgl_hip_quotient_plan_vertex_maps(vgl_hip_ctx *c, vgl_hip_quotient_plan *p, int32_t *d_cluster_of, int32_t *d_label_of, int32_t *d_size)
{
    if (!c || !p) VGL_FAIL("quotient_plan_vertex_maps: null argument");
    if (d_cluster_of) VGL_HIP_TRY(hipMemcpyAsync(d_cluster_of, p->cluster_of.p, sizeof(int32_t) * (size_t)p->V, hipMemcpyDeviceToDevice, c->stream));
    if (d_label_of) VGL_HIP_TRY(hipMemcpyAsync(d_label_of, p->label_of.p, sizeof(int32_t) * (size_t)p->Vc, hipMemcpyDeviceToDevice, c->stream));
    if (d_size) VGL_HIP_TRY(hipMemcpyAsync(d_size, p->size.p, sizeof(int32_t) * (size_t)p->Vc, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int vgl_hip_quotient_plan_members(vgl_hip_ctx *c, vgl_hip_quotient_plan *p, int32_t *d_members, int64_t *d_member_ptr)
{
    if (!c || !p) VGL_FAIL("quotient_plan_members: null argument");
    if (d_members) VGL_HIP_TRY(hipMemcpyAsync(d_members, p->members.p, sizeof(int32_t) * (size_t)p->V, hipMemcpyDeviceToDevice, c->stream));
    if (d_member_ptr) VGL_HIP_TRY(hipMemcpyAsync(d_member_ptr, p->member_ptr.p, sizeof(int64_t) * ((size_t)p->Vc + 1), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int vgl_hip_quotient_plan_fill(vgl_hip_ctx *c, vgl_hip_quotient_plan *p, int direction, const int64_t *d_weight, int64_t *d_rowptr, int32_t *d_adj, int64_t *d_count)
{
    if (!c || !p) VGL_FAIL("quotient_plan_fill: null argument");
    if (direction != 0 && direction != 1) VGL_FAIL("quotient_plan_fill: direction must be 0 (outgoing) or 1 (incoming)");
    if (!p->planned[direction]) VGL_FAIL("quotient_plan_fill: direction 1 needs the incoming CSR");
    const vgl_hip_quotient_plan::dir &D = p->d[direction];
    if (!d_rowptr || (D.entries > 0 && (!d_adj || !d_count))) VGL_FAIL("quotient_plan_fill: d_rowptr, d_adj and d_count must not be NULL");
    VGL_HIP_TRY(hipMemcpyAsync(d_rowptr, D.rowptr.p, sizeof(int64_t) * ((size_t)p->Vc + 1), hipMemcpyDeviceToDevice, c->stream));
    if (D.entries == 0) return 0;
    const quot_out o{nullptr, D.rowptr.p, d_adj, d_count, d_weight};
    VGL_TRY(quot_launch<true>(c, p, direction, quot_view_of(p, direction), o));
    return quot_sorted<true>(c, p, direction, o);
}

int vgl_hip_quotient_plan_destroy(vgl_hip_ctx *c, vgl_hip_quotient_plan *p)
{
    if (!c) VGL_FAIL("quotient_plan_destroy: null argument");
    if (!p) return 0;
    (void)hipStreamSynchronize(c->stream);
    delete p;
    return 0;
}

}  // extern "C"
