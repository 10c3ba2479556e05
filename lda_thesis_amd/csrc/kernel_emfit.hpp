// kernel_emfit.hpp -- llda_wcredit_index / _wave / _lds / _group / _combine kernels, llda_phistep_block / _den / _div kernels:
// the word side of the E-step and the phi M-step (EM training)
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_credit_words (include/llda_gibbs.h): the shares of llda_attribute's E-step added up per WORD, credit_w[v][k], the expected
// n_kw of the corpus under (theta, phi_t).  With llda_phi_step it is the other half of EM training.
//
// Arithmetic (fixed by the header, restated in tests/emref.py): a site's t, p, inv and g are kernel_attr.hpp's, with the factors of
// t the other way round (IEEE multiplication commutes).  The ORDER of the sum is what the header adds: the run of a word is cut
// into chunks of `chunk` sites, a chunk is added in ascending site order from +0.0, the chunk sums in ascending chunk order from
// +0.0.  No floating-point atomics: every sum has one owner.
//
// Geometry: the walks of doc_model.hpp with the roles swapped -- the "document" is a chunk of one word's sites, its "loads" the
// word's row of phi_t (in registers, in global memory beyond K = 1024 with the sums in LDS, one value per lane for K <= 32), the
// "words" of its sites are document ids and the rows that stream in are theta's.  One wavefront (one lane group) per CHUNK: the
// hot words of a Zipf corpus are thousands of chunks, not one serial tail.
//   llda_wcredit_index_kernel (one workgroup): cfirst[v] = chunks of the words before v, pfirst[v] = those of them that belong to
//       words with more than one chunk (their partial rows in the scratch), both exclusive prefix sums over the V words, and
//       cword[c] = the word of chunk c (one load per chunk where a bisection in cfirst would be 17 dependent ones);
//   the chunk kernels: chunk c is chunk c - cfirst[v] of the word v = cword[c].  The only chunk of a word stores 0.0 + its sum
//       straight to credit_w / tok / bad; a chunk of a longer word stores its sum to its partial row;
//   llda_wcredit_combine_kernel: a wavefront per word that has no chunk (a row of +0.0) or more than one (the partial rows added
//       in ascending order).
// What a word gets depends on its own sites and rows and on chunk: a chunk's sum does not know which kernel form or grid ran.
// Offsets that do not fit the caller's S, or partial rows beyond the scratch, are never used as addresses.
// ---------------------------------------------------------------------------------------------
struct WCreditParams : DocModel {                       // word = site_doc, phi_t / ld_phi / V = theta, its stride and its D rows
    const int64_t *word_off;
    const double *wphi;                                 // phi_t [n_words][ld_wphi]
    int64_t n_words, ld_wphi, ld_credit, S, rows_cap, chunks_cap;
    int32_t chunk;
    int64_t *cfirst, *pfirst;                           // [n_words + 1] each; NULL: no word has a site
    int32_t *cword;                                     // [chunks_cap]
    double *part;                                       // [rows_cap][K]
    int64_t *ptok, *pbad;                               // [rows_cap]
    double *credit_w;
    int64_t *tok, *bad;
};

constexpr int WCREDIT_WAVES = 4;                        // wavefronts of a workgroup (wave, group and combine kernels)
constexpr int WCREDIT_INDEX_NT = 1024;                  // threads of the one workgroup of llda_wcredit_index_kernel
constexpr int64_t WCREDIT_LDS_MAX_BLOCKS = 1 << 16;     // workgroups of llda_wcredit_lds_kernel at most: each takes its chunks in turn

__device__ __forceinline__ int64_t wcredit_chunks(const WCreditParams &P, int64_t v)
{
    const int64_t n = P.word_off[v + 1] - P.word_off[v];
    return n > 0 ? (n + P.chunk - 1) / P.chunk : 0;
}

// the two exclusive prefix sums over the words and the word of every chunk: tiles of WCREDIT_INDEX_NT consecutive words, thread t on
// word t of the tile (coalesced), a scan inside every wavefront, the wavefronts' totals through LDS, the running totals in registers
__global__ void __launch_bounds__(WCREDIT_INDEX_NT) llda_wcredit_index_kernel(const WCreditParams P)
{
    constexpr int NW = WCREDIT_INDEX_NT / 64;
    __shared__ int64_t wc[NW], wp[NW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t base_c = 0, base_p = 0;                     // chunks / partial rows of the tiles before this one (every thread alike)
    for (int64_t v0 = 0; v0 < P.n_words; v0 += WCREDIT_INDEX_NT) {
        const int64_t v = v0 + t;
        const int64_t nc = v < P.n_words ? wcredit_chunks(P, v) : 0, np = nc > 1 ? nc : 0;
        int64_t ic = nc, ip = np;                       // inclusive scan over the wavefront
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int64_t a = __shfl_up(ic, s, 64), b = __shfl_up(ip, s, 64);
            if (lane >= s) { ic += a; ip += b; }
        }
        if (lane == 63) { wc[wave] = ic; wp[wave] = ip; }
        __syncthreads();
        int64_t oc = 0, op = 0, tc = 0, tp = 0;         // the wavefronts before this one; the tile
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int64_t x = wc[w], y = wp[w];
            if (w < wave) { oc += x; op += y; }
            tc += x; tp += y;
        }
        __syncthreads();                                // (the next tile writes wc / wp again)
        if (v < P.n_words) {
            const int64_t c = base_c + oc + ic - nc;
            P.cfirst[v] = c;
            P.pfirst[v] = base_p + op + ip - np;
            for (int64_t j = c; j < c + nc && j < P.chunks_cap; ++j) P.cword[j] = (int32_t)v;
        }
        base_c += tc; base_p += tp;
    }
    if (t == 0) { P.cfirst[P.n_words] = base_c; P.pfirst[P.n_words] = base_p; }
}

struct WChunk {
    int64_t v, b, e, row;                               // the word, its sites [b, e) of this chunk, the partial row (-1: none)
    bool single;                                        // the word's only chunk: the sums go straight to the outputs
};

// the chunks there are: what the index pass counted, and never more than the table holds
__device__ __forceinline__ int64_t wcredit_total(const WCreditParams &P)
{
    const int64_t n = P.cfirst[P.n_words];
    return n < P.chunks_cap ? n : P.chunks_cap;
}

// chunk c < wcredit_total -> its word and its sites
__device__ __forceinline__ WChunk wcredit_chunk(const WCreditParams &P, int64_t c)
{
    WChunk w;
    w.v = P.cword[c];
    const int64_t first = P.cfirst[w.v], j = c - first, end = P.word_off[w.v + 1];
    w.single = P.cfirst[w.v + 1] - first == 1;
    w.b = P.word_off[w.v] + j * P.chunk;
    w.e = w.b + P.chunk < end ? w.b + P.chunk : end;
    if (w.b < 0 || w.e > P.S) w.b = w.e = 0;            // (offsets that are not the caller's S sites: nothing is read)
    w.row = w.single ? -1 : P.pfirst[w.v] + j;
    if (w.row >= P.rows_cap) w.row = -1;                // (more partial rows than S allows: nothing is written)
    return w;
}

// where a chunk's sums go: the word's outputs or its partial row; NULL: nowhere
struct WDest {
    double *row;
    int64_t *tok, *bad;
    __device__ __forceinline__ WDest(const WCreditParams &P, const WChunk &w)
    {
        if (w.single) {
            row = P.credit_w ? P.credit_w + w.v * P.ld_credit : nullptr;
            tok = P.tok ? P.tok + w.v : nullptr;
            bad = P.bad ? P.bad + w.v : nullptr;
        } else {
            row = w.row >= 0 ? P.part + w.row * P.K : nullptr;
            tok = w.row >= 0 ? P.ptok + w.row : nullptr;
            bad = w.row >= 0 ? P.pbad + w.row : nullptr;
        }
    }
};

// 32 < K <= 1024: the word's row of phi_t and the chunk's sums in NI registers per lane each
template <int NI, int U>
__global__ void __launch_bounds__(64 * WCREDIT_WAVES) llda_wcredit_wave_kernel(const WCreditParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveCols<NI> C(lane, P.K);
    const int64_t total = wcredit_total(P);
    for (int64_t c = (int64_t)blockIdx.x * WCREDIT_WAVES + wave; c < total; c += (int64_t)gridDim.x * WCREDIT_WAVES) {
        const WChunk w = wcredit_chunk(P, c);
        const double *prow = P.wphi + w.v * P.ld_wphi;
        double ph[NI], acc[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) { ph[i] = prow[C.kc[i]]; acc[i] = 0.0; }
        int64_t tok = 0, bad = 0;
        wave_sites<NI, U>(P, C, ph, lane, w.b, w.e, [&](int64_t, int32_t f, bool ok, double p, const double (&t)[NI]) {
            const bool good = ok && attr_good(p);
            tok += good ? f : 0;
            bad += good ? 0 : f;
            if (!good) return;
            const double inv = 1.0 / p;
            const double g = (double)f * inv;
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] = acc[i] + t[i] * g;
        });
        const WDest dst(P, w);
        if (dst.row) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (C.in >> i & 1u) dst.row[C.kc[i]] = w.single ? 0.0 + acc[i] : acc[i];
        }
        if (lane == 0 && dst.tok) *dst.tok = tok;
        if (lane == 0 && dst.bad) *dst.bad = bad;
    }
}

// K > 1024: the chunk's sums in LDS (dynamic: 8 K bytes), the word's row of phi_t read through its pointer, one wavefront per
// workgroup.  Lane j touches the entries j + 64 i and no other: no barrier.
__global__ void __launch_bounds__(64) llda_wcredit_lds_kernel(const WCreditParams P)
{
    extern __shared__ double wcredit_lds[];
    const int lane = threadIdx.x;
    const int K = P.K;
    double *acc = wcredit_lds;
    const int64_t total = wcredit_total(P);
    for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
        const WChunk w = wcredit_chunk(P, c);
        const double *prow = P.wphi + w.v * P.ld_wphi;
        for (int k = lane; k < K; k += 64) acc[k] = 0.0;
        int64_t tok = 0, bad = 0;
        stream_sites(P, prow, lane, w.b, w.e, [&](int64_t, int32_t f, bool ok, double p, const double *row) {
            const bool good = ok && attr_good(p);
            tok += good ? f : 0;
            bad += good ? 0 : f;
            if (!good) return;
            const double inv = 1.0 / p;
            const double g = (double)f * inv;
#pragma unroll 8
            for (int k = lane; k < K; k += 64) acc[k] = acc[k] + (prow[k] * row[k]) * g;
        });
        const WDest dst(P, w);
        if (dst.row)
            for (int k = lane; k < K; k += 64) dst.row[k] = w.single ? 0.0 + acc[k] : acc[k];
        if (lane == 0 && dst.tok) *dst.tok = tok;
        if (lane == 0 && dst.bad) *dst.bad = bad;
    }
}

// K <= G <= 32: 64 / G chunks per wavefront, the groups of a wavefront walk to their longest chunk
template <int G>
__global__ void __launch_bounds__(64 * WCREDIT_WAVES) llda_wcredit_group_kernel(const WCreditParams P)
{
    constexpr int CPB = 64 * WCREDIT_WAVES / G;         // chunks of a workgroup
    const int64_t total = wcredit_total(P), n_tiles = (total + CPB - 1) / CPB;
    GroupDoc g;
    g.gl = threadIdx.x % G;
    g.mine = g.gl < P.K;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        g.d = tile * CPB + threadIdx.x / G;
        g.active = g.d < total;
        WChunk w;
        w.v = 0; w.b = w.e = 0; w.row = -1; w.single = false;
        if (g.active) w = wcredit_chunk(P, g.d);
        g.b = w.b;
        g.n = w.e - w.b;
        g.n_max = g.n;
#pragma unroll
        for (int s = G; s < 64; s <<= 1) {
            const int64_t o = __shfl_xor(g.n_max, s, 64);
            g.n_max = o > g.n_max ? o : g.n_max;
        }
        g.th = (g.active && g.mine) ? P.wphi[w.v * P.ld_wphi + g.gl] : 0.0;
        double acc = 0.0;
        int64_t tok = 0, bad = 0;
        group_sites<G>(P, g, g.th, [&](int64_t, int32_t f, bool ok, bool, double p, double tk) {
            const bool good = ok && attr_good(p);
            tok += good ? f : 0;                        // (a site past the chunk's end: f = 0)
            bad += good ? 0 : f;
            const double inv = good ? 1.0 / p : 0.0;
            if (good && g.mine) acc = acc + tk * ((double)f * inv);
        });
        if (!g.active) continue;
        const WDest dst(P, w);
        if (dst.row && g.mine) dst.row[g.gl] = w.single ? 0.0 + acc : acc;
        if (g.gl == 0 && dst.tok) *dst.tok = tok;
        if (g.gl == 0 && dst.bad) *dst.bad = bad;
    }
}

// the words without a chunk and the words with more than one: a wavefront per word
__global__ void __launch_bounds__(64 * WCREDIT_WAVES) llda_wcredit_combine_kernel(const WCreditParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t v = (int64_t)blockIdx.x * WCREDIT_WAVES + wave; v < P.n_words; v += (int64_t)gridDim.x * WCREDIT_WAVES) {
        const int64_t nc = P.cfirst ? P.cfirst[v + 1] - P.cfirst[v] : 0;
        if (nc == 1) continue;
        const int64_t r0 = nc ? P.pfirst[v] : 0;
        if (r0 + nc > P.rows_cap) continue;             // (more partial rows than S allows: none was written)
        if (P.credit_w)
            for (int k = lane; k < P.K; k += 64) {
                double acc = 0.0;
                for (int64_t j = 0; j < nc; ++j) acc = acc + P.part[(r0 + j) * P.K + k];
                P.credit_w[v * P.ld_credit + k] = acc;
            }
        if (lane == 0) {
            int64_t tok = 0, bad = 0;
            for (int64_t j = 0; j < nc; ++j) { tok += P.ptok[r0 + j]; bad += P.pbad[r0 + j]; }
            if (P.tok) P.tok[v] = tok;
            if (P.bad) P.bad[v] = bad;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// llda_phi_step (include/llda_gibbs.h): phi_t[v][k] = (cw[v][k] + beta) / (colsum[k] + V beta).  The column sums have a fixed
// order too: blocks of PHISTEP_ROWS words added in ascending order from +0.0 (one thread per column and block), then the block
// sums in ascending order from +0.0 (one thread per column).  The division reads cw[v][k] and writes out[v][k] in the same
// thread, after both sums are complete (stream order): out may be cw.
// ---------------------------------------------------------------------------------------------
struct PhiStepParams {
    const double *cw;
    double *out, *den_out;
    double *bsum, *den;                                 // [n_blocks][K], [K]: the scratch
    int64_t V, ld, ld_out, n_blocks;
    int32_t K;
    double beta, Vb;
};

constexpr int PHISTEP_ROWS = 256;                       // LLDA_COLSUM_ROWS
constexpr int PHISTEP_NT = 256;

__global__ void __launch_bounds__(PHISTEP_NT) llda_phistep_block_kernel(const PhiStepParams P)
{
    const int k = blockIdx.y * PHISTEP_NT + threadIdx.x;
    if (k >= P.K) return;
    const int64_t r0 = (int64_t)blockIdx.x * PHISTEP_ROWS, r1 = r0 + PHISTEP_ROWS < P.V ? r0 + PHISTEP_ROWS : P.V;
    double acc = 0.0;
    for (int64_t r = r0; r < r1; ++r) acc = acc + P.cw[r * P.ld + k];
    P.bsum[(int64_t)blockIdx.x * P.K + k] = acc;
}

__global__ void __launch_bounds__(PHISTEP_NT) llda_phistep_den_kernel(const PhiStepParams P)
{
    const int k = blockIdx.x * PHISTEP_NT + threadIdx.x;
    if (k >= P.K) return;
    double acc = 0.0;
    for (int64_t b = 0; b < P.n_blocks; ++b) acc = acc + P.bsum[b * P.K + k];
    const double den = acc + P.Vb;
    P.den[k] = den;
    if (P.den_out) P.den_out[k] = den;
}

__global__ void __launch_bounds__(PHISTEP_NT) llda_phistep_div_kernel(const PhiStepParams P)
{
    const int64_t n = P.V * P.K, step = (int64_t)gridDim.x * PHISTEP_NT;
    for (int64_t i = (int64_t)blockIdx.x * PHISTEP_NT + threadIdx.x; i < n; i += step) {
        const int64_t v = i / P.K;
        const int k = (int)(i - v * P.K);
        P.out[v * P.ld_out + k] = (P.cw[v * P.ld + k] + P.beta) / P.den[k];
    }
}

}  // namespace
