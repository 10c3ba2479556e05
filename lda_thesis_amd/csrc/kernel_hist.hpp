// kernel_hist.hpp -- llda_count_hist_kernel: counts of counts of n_dk / n_kw for the estimate of the priors
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_count_hist (include/llda_gibbs.h): how many ALLOWED entries of a (rows, KP) count matrix hold the value n, for every n.
// Minka's fixed point for a symmetric Dirichlet prior sees n_dk and n_kw only through these histograms, and a histogram is exact
// and independent of order: the estimate stays bit-identical for every grid and every number of ranks.
//
// A bandwidth pass.  The matrix is walked as one run of 16-byte chunks (KP is a multiple of 8): a workgroup takes tiles of
// 256 * HIST_UNROLL consecutive chunks, so every load instruction of a wavefront reads 1 KB of one row (or of neighbouring rows), and
// all HIST_UNROLL loads of a thread are in flight before the first is looked at.  In the group layout a chunk holds the slots
// 4q .. 4q+3 of ONE lane (T a multiple of 4; q = chunk / G, lane = chunk % G), so its four label bits are one nibble of one mask
// word; rows of one or two slots per lane (K <= 16) hold four / two lanes per chunk.
//
// Most entries are 0 and most of the rest 1 .. 3: those are counted in four registers per thread (an LDS atomic on them would
// serialise the whole wavefront on one address).  Values up to HIST_LDS_BINS go to a histogram of the workgroup in LDS -- spread
// over many addresses, few conflicts --, flushed once at the end with one 64-bit atomic per non-empty bin; larger values below
// n_bins take a global 64-bit atomic each (rare and scattered), and everything outside 0 .. n_bins-1 goes to the overflow list.
// The 32-bit counters hold what ONE thread / ONE workgroup counts: 2^32 entries per workgroup of a 2048-workgroup grid are 32 TB.
// ---------------------------------------------------------------------------------------------
constexpr int HIST_LDS_BINS = 4096;        // 16 KB per workgroup: eight workgroups per CU
constexpr int HIST_REG_BINS = 4;
constexpr int HIST_UNROLL = 4;

struct HParams {
    const int4 *counts;
    int64_t n4;                            // chunks: rows * KP / 4
    const uint16_t *mask;
    int64_t mask_stride;                   // G (a mask row per row) or 0 (one mask row for all)
    int32_t G, cpr;                        // lanes per row, chunks per row (KP / 4)
    uint32_t g_magic;                      // ceil(2^24 / G): chunk / G = chunk * g_magic >> 24 for chunk < 2048, G <= 8192
    uint32_t n_bins;
    int32_t step256_r, step256_c;          // 256 chunks on = so many rows + so many chunks (< cpr) ...
    int32_t tile_c;                        // ... and from the end of one tile of the workgroup to the start of its next one
    int64_t tile_rows;
    unsigned long long *hist;
    int32_t *over_val;
    int64_t over_cap;
    unsigned long long *over_n;
};

// the label bits of the four entries of chunk c of a row (bit j = entry 4c + j is allowed); W = slots of a lane that are contiguous
template <int W>
__device__ __forceinline__ uint32_t hist_allowed(const uint16_t *__restrict__ mrow, int c, int G, uint32_t g_magic)
{
    if constexpr (W == 4) {
        const int q = (int)(((uint32_t)c * g_magic) >> 24), g = c - q * G;
        return ((uint32_t)mrow[g] >> (4 * q)) & 15u;
    } else if constexpr (W == 2) {
        return ((uint32_t)mrow[2 * c] & 3u) | (((uint32_t)mrow[2 * c + 1] & 3u) << 2);
    } else {
        return ((uint32_t)mrow[4 * c] & 1u) | (((uint32_t)mrow[4 * c + 1] & 1u) << 1) | (((uint32_t)mrow[4 * c + 2] & 1u) << 2) |
               (((uint32_t)mrow[4 * c + 3] & 1u) << 3);
    }
}

template <int W>
__global__ void __launch_bounds__(256) llda_count_hist_kernel(const HParams P)
{
    __shared__ uint32_t s_hist[HIST_LDS_BINS];
    const int tid = threadIdx.x;
    for (int b = tid; b < HIST_LDS_BINS; b += 256) s_hist[b] = 0;
    __syncthreads();
    const uint32_t n_bins = P.n_bins;
    const uint32_t reg_bins = min(n_bins, (uint32_t)HIST_REG_BINS), lds_bins = min(n_bins, (uint32_t)HIST_LDS_BINS);
    const int cpr = P.cpr, G = P.G;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;

    auto tally = [&](int32_t v, bool on) {
        const uint32_t u = (uint32_t)v;
        c0 += (on && u == 0u) ? 1u : 0u;
        c1 += (on && u == 1u) ? 1u : 0u;
        c2 += (on && u == 2u) ? 1u : 0u;
        c3 += (on && u == 3u) ? 1u : 0u;
        if (on && u >= reg_bins) {
            if (u < lds_bins) atomicAdd(&s_hist[u], 1u);
            else if (u < n_bins) atomicAdd(P.hist + u, 1ull);
            else {
                const unsigned long long i = atomicAdd(P.over_n, 1ull);
                if (i < (unsigned long long)P.over_cap) P.over_val[i] = v;
            }
        }
    };

    int64_t i = (int64_t)blockIdx.x * (256 * HIST_UNROLL) + tid;
    int64_t r = i / cpr;
    int c = (int)(i - r * cpr);
    while (i < P.n4) {                                      // (uniform per tile up to its ragged end: the guards below)
        int4 v[HIST_UNROLL];
        uint32_t bits[HIST_UNROLL];
#pragma unroll
        for (int k = 0; k < HIST_UNROLL; ++k) {
            const bool in = i < P.n4;
            v[k] = in ? P.counts[i] : make_int4(0, 0, 0, 0);
            bits[k] = in ? hist_allowed<W>(P.mask + r * P.mask_stride, c, G, P.g_magic) : 0u;
            // 256 chunks on (the last step of a tile goes on to the workgroup's next tile)
            i += 256;
            c += P.step256_c;
            r += P.step256_r;
            if (c >= cpr) { c -= cpr; ++r; }
        }
#pragma unroll
        for (int k = 0; k < HIST_UNROLL; ++k) {
            tally(v[k].x, bits[k] & 1u);
            tally(v[k].y, bits[k] & 2u);
            tally(v[k].z, bits[k] & 4u);
            tally(v[k].w, bits[k] & 8u);
        }
        i += (int64_t)(gridDim.x - 1) * (256 * HIST_UNROLL);
        c += P.tile_c;
        r += P.tile_rows;
        if (c >= cpr) { c -= cpr; ++r; }
    }
    if (c0) atomicAdd(&s_hist[0], c0);
    if (c1) atomicAdd(&s_hist[1], c1);
    if (c2) atomicAdd(&s_hist[2], c2);
    if (c3) atomicAdd(&s_hist[3], c3);
    __syncthreads();
    // (bins 1 .. 3 of s_hist hold entries that belong to the overflow list when n_bins < 4: they went there too, see reg_bins)
    for (uint32_t b = tid; b < lds_bins; b += 256) {
        const uint32_t h = s_hist[b];
        if (h) atomicAdd(P.hist + b, (unsigned long long)h);
    }
}

}  // namespace
