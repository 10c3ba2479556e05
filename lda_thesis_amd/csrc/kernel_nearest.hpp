// kernel_nearest.hpp -- llda_nearest_kernel / llda_nearest_merge_kernel: the n best rows of b for every row of a under a bilinear score
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_nearest_rows (include/llda_gibbs.h): score(q, j) = the FMA chain s = fma(a[q][k], b[j][k], s) over k ascending from
// +0.0, one rounding per element; per query the n best rows by (score descending as IEEE values, global row id ascending), NaN scores
// and the query's `exclude` row left out.  No score is ever written to memory.
//
// Pass 1, an fp64 product tiled in LDS and registers with the selection in its epilogue.  A workgroup of 256 lanes owns NEAR_T = 128
// queries and walks one row range of b in tiles of 128 rows.  The lanes form a 16 x 16 grid (dx = lane & 15 over rows, qx = lane >> 4
// over queries) and every lane keeps an 8 x 8 block of accumulators; the k-loop runs in steps of NEAR_KS = 16 columns that are staged
// k-major in LDS (the next step's global loads are in flight while this one is multiplied).  Every accumulator sees k = 0, 1, .., L-1
// in this order and nothing else: a score depends on its two rows only.  Columns past L and rows past the range are staged as +0.0,
// and fma(0, 0, s) = s for every s the chain can hold (it never holds -0.0: it starts at +0.0).
// A lane's eight queries are 2 qx, 2 qx + 1, 32 + 2 qx, ... (near_local): its LDS reads are four 16-byte reads per operand and the
// sixteen lanes of a row read one contiguous 256-byte run.
// Epilogue.  The sixteen lanes that share a query sit in ONE wavefront, so a query's list -- n (score, id) pairs in LDS, best first;
// the n-th is the key to beat -- belongs to one wavefront and needs no barrier.  Every lane compares its 64 scores with the keys of
// its eight queries, one row of its block at a time, so that the keys tighten between rows; almost always none passes and the
// wavefront goes on.  Otherwise, query by query, the lanes that hold a candidate take turns (lowest lane of the sixteen first): the
// candidate is handed to all sixteen lanes, lane p owns place p of the list and keeps its entry, takes the candidate, or takes the
// entry of place p - 1 -- one parallel step per candidate, and a candidate that no longer beats the key changes nothing.  The n best
// under a total order do not depend on the order of arrival.  An empty place is (-inf, INT64_MAX): any candidate beats it.
// Every (query, range) leaves its list and its NaN count in scratch.
//
// Pass 2: one lane per query merges the lists of the ranges (each is sorted: the first entry that fails ends a list), adds the NaN
// counts, and writes the outputs with their padding.
// ---------------------------------------------------------------------------------------------
constexpr int NEAR_T = 128;                               // queries and rows of a tile (both tile edges)
constexpr int NEAR_KS = 16;                               // columns per step of the k-loop
constexpr int NEAR_LD = NEAR_T + 2;                       // LDS row of a staged column: 2 doubles of padding spread the transposing stores
constexpr int NEAR_MAX_N = 16;
constexpr int64_t NEAR_EMPTY = INT64_MAX;

struct NearParams {
    const double *a, *b;
    int64_t Q, D, lda, ldb, row_base;
    const int64_t *exclude;
    int32_t L, n, chunks, reserved;
    double *part_val;                                     // [Q][chunks][n]
    int64_t *part_idx;                                    // [Q][chunks][n]
    int64_t *part_nan;                                    // [Q][chunks]
    int64_t *top_idx;
    double *top_val;
    int64_t *n_nan;
};

// does (s, id) come before (ts, tid)?  IEEE compares: -0 == +0, a NaN s never does
__device__ __forceinline__ bool near_beats(double s, int64_t id, double ts, int64_t tid)
{
    return s > ts || (s == ts && id < tid);
}

// the i-th of a lane's eight rows (or queries) of the tile, for the lane coordinate x in 0 .. 15
__device__ __forceinline__ int near_local(int x, int i) { return (i >> 1) * 32 + x * 2 + (i & 1); }

// first row of range c of D rows cut into C ranges (the first D % C ranges take one row more)
__host__ __device__ inline int64_t near_range_start(int64_t D, int64_t C, int64_t c)
{
    const int64_t base = D / C, rem = D % C;
    return c * base + (c < rem ? c : rem);
}

// one step's share of a lane: 8 doubles of the a tile and 8 of the b tile, +0.0 outside
template <bool VEC>
__device__ __forceinline__ void near_fetch(const NearParams &P, int64_t q0, int64_t r0, int64_t r1, int k0, int tid, double (&ga)[8], double (&gb)[8])
{
    if (VEC) {                                            // 16-byte loads: both bases 16-byte aligned, both ld even
        const int kk = (tid & 7) * 2, row = tid >> 3;
        const int k = k0 + kk;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = q0 + row + 32 * u, r = r0 + row + 32 * u;
            double2 va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
            if (q < P.Q) {
                const double *p = P.a + q * P.lda + k;
                if (k + 1 < P.L) va = *reinterpret_cast<const double2 *>(p);
                else if (k < P.L) va.x = *p;
            }
            if (r < r1) {
                const double *p = P.b + r * P.ldb + k;
                if (k + 1 < P.L) vb = *reinterpret_cast<const double2 *>(p);
                else if (k < P.L) vb.x = *p;
            }
            ga[2 * u] = va.x; ga[2 * u + 1] = va.y;
            gb[2 * u] = vb.x; gb[2 * u + 1] = vb.y;
        }
    } else {
        const int kk = tid & 15, row = tid >> 4;
        const int k = k0 + kk;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t q = q0 + row + 16 * u, r = r0 + row + 16 * u;
            ga[u] = (q < P.Q && k < P.L) ? P.a[q * P.lda + k] : 0.0;
            gb[u] = (r < r1 && k < P.L) ? P.b[r * P.ldb + k] : 0.0;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void near_stage(double *As, double *Bs, int tid, const double (&ga)[8], const double (&gb)[8])
{
    if (VEC) {
        const int kk = (tid & 7) * 2, row = tid >> 3;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            As[kk * NEAR_LD + row + 32 * u] = ga[2 * u];
            As[(kk + 1) * NEAR_LD + row + 32 * u] = ga[2 * u + 1];
            Bs[kk * NEAR_LD + row + 32 * u] = gb[2 * u];
            Bs[(kk + 1) * NEAR_LD + row + 32 * u] = gb[2 * u + 1];
        }
    } else {
        const int kk = tid & 15, row = tid >> 4;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            As[kk * NEAR_LD + row + 16 * u] = ga[u];
            Bs[kk * NEAR_LD + row + 16 * u] = gb[u];
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) llda_nearest_kernel(const NearParams P)
{
    __shared__ __attribute__((aligned(16))) double As[NEAR_KS * NEAR_LD];
    __shared__ __attribute__((aligned(16))) double Bs[NEAR_KS * NEAR_LD];
    __shared__ double list_s[NEAR_T * NEAR_MAX_N];
    __shared__ int64_t list_i[NEAR_T * NEAR_MAX_N];
    __shared__ int64_t excl[NEAR_T];
    __shared__ unsigned long long nan_cnt[NEAR_T];

    const int tid = threadIdx.x, dx = tid & 15, qx = tid >> 4, grp = (tid >> 4) & 3;
    const int n = P.n;
    const int64_t q_tiles = (P.Q + NEAR_T - 1) / NEAR_T;  // (workgroups of one range are neighbours: they read the same rows of b)
    const int64_t c = (int64_t)blockIdx.x / q_tiles;
    const int64_t q0 = ((int64_t)blockIdx.x - c * q_tiles) * NEAR_T;
    const int64_t rs = near_range_start(P.D, P.chunks, c), re = near_range_start(P.D, P.chunks, c + 1);

    for (int e = tid; e < NEAR_T * NEAR_MAX_N; e += 256) { list_s[e] = -INFINITY; list_i[e] = NEAR_EMPTY; }
    if (tid < NEAR_T) {
        excl[tid] = (P.exclude && q0 + tid < P.Q) ? P.exclude[q0 + tid] : -1;
        nan_cnt[tid] = 0;
    }
    __syncthreads();

    double ga[8], gb[8];
    for (int64_t r0 = rs; r0 < re; r0 += NEAR_T) {
        double acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;
        near_fetch<VEC>(P, q0, r0, re, 0, tid, ga, gb);
        for (int k0 = 0; k0 < P.L; k0 += NEAR_KS) {
            __syncthreads();                              // the last step's reads of the tiles are done
            near_stage<VEC>(As, Bs, tid, ga, gb);
            __syncthreads();
            if (k0 + NEAR_KS < P.L) near_fetch<VEC>(P, q0, r0, re, k0 + NEAR_KS, tid, ga, gb);
#pragma unroll 4
            for (int kk = 0; kk < NEAR_KS; ++kk) {
                double2 av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    av[u] = *reinterpret_cast<const double2 *>(&As[kk * NEAR_LD + u * 32 + qx * 2]);
                    bv[u] = *reinterpret_cast<const double2 *>(&Bs[kk * NEAR_LD + u * 32 + dx * 2]);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const double x = (i & 1) ? av[i >> 1].y : av[i >> 1].x;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const double y = (j & 1) ? bv[j >> 1].y : bv[j >> 1].x;
                        acc[i][j] = __builtin_fma(x, y, acc[i][j]);
                    }
                }
            }
        }

        // ---- epilogue: row by row of the lane's block, which scores beat the key of their query?
        double ts[8];
        int64_t ti[8], ex[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ql = near_local(qx, i);
            ts[i] = ((volatile double *)list_s)[ql * NEAR_MAX_N + n - 1];
            ti[i] = ((volatile int64_t *)list_i)[ql * NEAR_MAX_N + n - 1];
            ex[i] = excl[ql];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t r = r0 + near_local(dx, j);
            const int64_t id = P.row_base + r;
            uint32_t pass = 0;
            if (r < re) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (q0 + near_local(qx, i) >= P.Q) continue;
                    const double s = acc[i][j];
                    if (s != s) atomicAdd(&nan_cnt[near_local(qx, i)], 1ull);
                    else if (id != ex[i] && near_beats(s, id, ts[i], ti[i])) pass |= 1u << i;
                }
            }
            if (!__any(pass != 0)) continue;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ql = near_local(qx, i);
                volatile double *ls = list_s + ql * NEAR_MAX_N;
                volatile int64_t *li = list_i + ql * NEAR_MAX_N;
                bool pend = (pass >> i) & 1;
                while (__any(pend)) {                     // (uniform: every lane of the wavefront takes part in the ballot)
                    const uint32_t mine = (uint32_t)(__ballot(pend) >> (16 * grp)) & 0xFFFFu;
                    if (mine) {                           // (the same for the sixteen lanes of a query: they take the branch together)
                        const int leader = __ffs((int)mine) - 1;
                        const double cs = __shfl(acc[i][j], leader, 16);
                        const int64_t ci = __shfl(id, leader, 16);
                        // lane dx owns place dx of the list: it keeps its entry, takes the candidate, or takes its better neighbour's
                        double es = 0.0, ps = 0.0;
                        int64_t ei = 0, pi = 0;
                        if (dx < n) {
                            es = ls[dx]; ei = li[dx];
                            if (dx > 0) { ps = ls[dx - 1]; pi = li[dx - 1]; }
                        }
                        const bool up = dx > 0 && near_beats(cs, ci, ps, pi), in = near_beats(cs, ci, es, ei);
                        if (dx < n && (up || in)) {       // (every lane has read before any lane writes: one instruction stream)
                            ls[dx] = up ? ps : cs;
                            li[dx] = up ? pi : ci;
                        }
                        if (dx == leader) pend = false;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                ts[i] = ls[n - 1];                        // the key as it is now
                ti[i] = li[n - 1];
            }
        }
    }

    __syncthreads();
    for (int e = tid; e < NEAR_T * n; e += 256) {
        const int ql = e / n, p = e - ql * n;
        const int64_t q = q0 + ql;
        if (q < P.Q) {
            const int64_t at = (q * P.chunks + c) * n + p;
            P.part_val[at] = list_s[ql * NEAR_MAX_N + p];
            P.part_idx[at] = list_i[ql * NEAR_MAX_N + p];
        }
    }
    if (tid < NEAR_T && q0 + tid < P.Q) P.part_nan[(q0 + tid) * P.chunks + c] = (int64_t)nan_cnt[tid];
}

// (score, id) as an entry of the merge kernel's TopList (top_list.hpp): the bits of the double, then the id
struct NearOrd {
    static constexpr int Q = 2, W = 0;
    typedef TopEntry<2, 0> E;
    static __device__ __forceinline__ double score(const E &e) { return __longlong_as_double((long long)e.q[0]); }
    static __device__ __forceinline__ int64_t id(const E &e) { return (int64_t)e.q[1]; }
    static __device__ __forceinline__ E entry(double s, int64_t id) { return E{{(uint64_t)__double_as_longlong(s), (uint64_t)id}, {0}}; }
    __device__ __forceinline__ E pad() const { return entry(-INFINITY, NEAR_EMPTY); }
    __device__ __forceinline__ bool before(const E &a, const E &b) const { return near_beats(score(a), id(a), score(b), id(b)); }
    __device__ __forceinline__ bool same(const E &a, const E &b) const { return id(a) == id(b); }
};

__global__ void __launch_bounds__(64) llda_nearest_merge_kernel(const NearParams P)
{
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= P.Q) return;
    const int n = P.n;
    TopList<NEAR_MAX_N, NearOrd> L;
    int64_t nans = 0;
    for (int64_t c = 0; c < P.chunks; ++c) {
        nans += P.part_nan[q * P.chunks + c];
        const double *ps = P.part_val + (q * P.chunks + c) * n;
        const int64_t *pi = P.part_idx + (q * P.chunks + c) * n;
        for (int p = 0; p < n; ++p) {
            const NearOrd::E e = NearOrd::entry(ps[p], pi[p]);
            // (the list is sorted: behind an empty place, or an entry that does not get in, nothing gets in either)
            if (pi[p] == NEAR_EMPTY || !L.admits(e)) break;
            L.insert(e);
        }
    }
#pragma unroll
    for (int j = 0; j < NEAR_MAX_N; ++j)
        if (j < n) {
            const int64_t id = NearOrd::id(L.at(j));
            if (P.top_idx) P.top_idx[q * n + j] = id != NEAR_EMPTY ? id : -1;
            if (P.top_val) P.top_val[q * n + j] = id != NEAR_EMPTY ? NearOrd::score(L.at(j)) : 0.0;
        }
    if (P.n_nan) P.n_nan[q] = nans;
}

}  // namespace
