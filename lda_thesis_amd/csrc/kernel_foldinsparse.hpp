// kernel_foldinsparse.hpp -- llda_foldin_sparse_kernel: the test-time sampler on sparse label sets
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_foldin_sparse (include/llda_gibbs.h): llda_foldin for documents that carry a handful of the K labels, K up
// to LLDA_MAX_K.  The label sets are kernel_docsparse.hpp's CSR (without loads); z, n_dk_s and th_s live per SLOT of the list.
//
// Arithmetic: the header text of llda_foldin (beta_fallback = 0, avg_mode = 0, beta = 0) on the document's compacted problem --
// K' = L_d, ph'[j][v] = phi_t[v][lab[j]] -- in the oracle's layout(L_d): L_d <= 32 is ONE numpy leaf, compacted topic j sits in lane
// j & 7, slot j >> 3 of a group of 8 lanes.  Here a lane holds T = 1, 2 or 4 >= ceil(max_labels / 8) slots; the slots past L_d hold
// +0.0 and are never positive, so the prefixes, the Hillis-Steele scan and the draw are those of the document's own T_d <= T slots.
//   sum      numpy's order for L_d contiguous doubles, per DOCUMENT (documents of different L_d share a wavefront): R = L_d >> 3 full
//            rows on the eight chains (slot s < R of every lane), the xor butterfly 1, 2, 4, then the L_d & 7 tail entries (slot R of
//            the lanes < L_d & 7) in order.  R = 0 is numpy's sequential sum: the chains hold +0.0.
//   start    nothing can be prepared per word, the column sum runs over the document's labels: a first pass over the document finds
//            a column that cannot be normalised (sum 0, or a quotient that is not finite), then every site starts from the uniform
//            row 1 / L_d; else from column / sum.  `while sum > 1: prob /= c_init`, the draw under the sweep word 0xFFFFFFFF.
//   sweep    prob = (n_dk + alpha) * ph'[:, v]; S = sum; prob /= S; `while sum > 1: prob /= c_loop`; draw.  No decided tier: every
//            site takes this pipeline.  The quotients are the hardware's IEEE divisions (v_div_scale / v_div_fmas / v_div_fixup),
//            correctly rounded over the whole range of doubles: no reciprocal shortcut, so no rescale rule.
//   average  every `thinning` sweeps cur = n_dk / n_dk.sum() enters (s-1)/s * avg + (1/s) * cur, each product rounded on its own.
//
// Geometry.  8 lanes per document, 8 documents per wavefront, 32 per workgroup; label ids, counts and the average in registers.
// Everything a group does depends on its own document only: the loops and branches below diverge between groups and are uniform
// inside one, and every cross-lane operation (DPP inside 8 lanes, shuffles of width 8, ballots cut to the group's byte) reads the
// group's own lanes.  A site's row is L_d gathered doubles whatever K is; the row of the next site and the word of the site after
// it are in flight while a site is sampled (the sites are walked cyclically, as llda_foldin_kernel does).
// z is written by lane 0 of the group and read back by all eight one sweep later (one site later in a document of one site: that
// one is carried in a register).
//
// Unfit document (label_slot's rules): z = -1 at its sites, nothing else written, no label id used as an index, status bit 2.
// A word outside [0, V): z = -1, no count, never an index, the site keeps its number n; status bit 1.
// No positive probability at a site (every site of L_d = 0): status bit 0; the site keeps its old slot (slot 0 at the start).
// ---------------------------------------------------------------------------------------------
struct FoldinSparseParams {
    const int64_t *doc_off;
    const int32_t *word;
    const int32_t *freq;
    const double *phi_t;
    const int64_t *doc_ids;
    int32_t *z;
    int32_t *n_dk_s;
    double *th_s;
    int32_t *status;
    LabelSets sets;                                     // (theta_s is not used)
    int64_t D, V, ld_phi, doc_base;
    double alpha, c_init, c_loop;
    uint32_t key0, key1, stream_id;
    int32_t K, iters, thinning;
};

constexpr int FS_THREADS = 256;
constexpr int FS_DOCS = FS_THREADS / 8;                 // documents of a workgroup
constexpr int FS_MAX_STEPS = 1 << 28;                   // of one `while sum > 1` loop (llda_foldin_kernel's bound)

inline int foldin_sparse_slots(int max_labels) { return max_labels <= 8 ? 1 : max_labels <= 16 ? 2 : 4; }

// numpy's sum of the document's L_d = 8 R + tail doubles; every lane of the group returns it
template <int T>
__device__ __forceinline__ double fs_sum(const double (&w)[T], int R, int tail)
{
    double acc = 0.0, tv = 0.0;
#pragma unroll
    for (int s = 0; s < T; ++s) {
        acc = s < R ? acc + w[s] : acc;
        tv = s == R ? w[s] : tv;
    }
    acc = acc + dpp_f64<DPP_XOR1>(acc);
    acc = acc + dpp_f64<DPP_XOR2>(acc);
    acc = acc + dpp_f64<DPP_HALF_MIRROR>(acc);
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const double o = __shfl(tv, t, 8);
        acc = t < tail ? acc + o : acc;
    }
    return acc;
}

// `while prob.sum() > 1: prob /= c`, step by step
template <int T>
__device__ __forceinline__ void fs_shrink(double (&p)[T], double c, int R, int tail)
{
    int steps = 0;
    while (fs_sum<T>(p, R, tail) > 1.0 && steps < FS_MAX_STEPS) {       // (group-uniform)
#pragma unroll
        for (int s = 0; s < T; ++s) p[s] = p[s] / c;
        ++steps;
    }
}

template <int T>
__global__ void __launch_bounds__(FS_THREADS) llda_foldin_sparse_kernel(const FoldinSparseParams P, const int64_t n_tiles)
{
    const int lane = threadIdx.x & 63, j = threadIdx.x & 7;
    const int gbase = lane & ~7;
    const double inf = __builtin_huge_val();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t d = tile * FS_DOCS + (threadIdx.x >> 3);
        if (d >= P.D) continue;                                         // (whole groups)
        const int64_t s0 = P.doc_off[d];
        const int len = (int)(P.doc_off[d + 1] - s0);
        // the label list: slot 8 s + j in register s
        const int64_t lb = P.sets.lab_off[d], L64 = P.sets.lab_off[d + 1] - lb;
        const bool inside = lb >= 0 && L64 >= 0 && L64 <= P.sets.NL && lb <= P.sets.NL - L64;
        const bool range = inside && L64 <= P.sets.max_labels;
        const int L = range ? (int)L64 : 0;
        int k[T];
        bool wrong = false;
#pragma unroll
        for (int s = 0; s < T; ++s) {
            const int i = 8 * s + j;
            const bool slot = i < L;
            k[s] = slot ? P.sets.lab[lb + i] : -1;
            const int left = (slot && i > 0) ? P.sets.lab[lb + i - 1] : -1;
            wrong = wrong || (slot && ((uint32_t)k[s] >= (uint32_t)P.K || k[s] <= left));
        }
        const bool fit = range && !((__ballot(wrong) >> gbase) & 0xFFull);
        if (!fit) {
            for (int n = j; n < len; n += 8) P.z[s0 + n] = -1;
            if (j == 0 && P.status) atomicOr(P.status, 4);
            continue;
        }
        bool mine[T];
#pragma unroll
        for (int s = 0; s < T; ++s) {
            mine[s] = 8 * s + j < L;
            k[s] = mine[s] ? k[s] : 0;
        }
        const int R = L >> 3, tail = L & 7;
        const uint32_t gdoc = P.doc_ids ? (uint32_t)P.doc_ids[d] : (uint32_t)(d + P.doc_base);
        int ndk[T];
        double avg[T];
#pragma unroll
        for (int s = 0; s < T; ++s) { ndk[s] = 0; avg[s] = 0.0; }
        int64_t ntot = 0;
        // the gathered row of a word: ph'[:, v] on the lane's slots, +0.0 where it has none
        auto gather = [&](const int v, const bool ok, double (&b)[T]) {
            const double *row = P.phi_t + (int64_t)(ok ? v : 0) * P.ld_phi;
#pragma unroll
            for (int s = 0; s < T; ++s) b[s] = (ok && mine[s]) ? row[k[s]] : 0.0;
        };
        // ---- first pass: does the document hold a column that cannot be normalised?
        bool uni = false;
        {
            int v_1 = len > 0 ? P.word[s0] : -1;
            for (int n = 0; n < len; ++n) {
                const int v = v_1;
                v_1 = P.word[s0 + (n + 1 < len ? n + 1 : n)];
                const bool ok = word_ok(v, P.V);
                if (!ok) continue;                                      // (group-uniform)
                double a[T];
                gather(v, true, a);
                const double cs = fs_sum<T>(a, R, tail);
                bool bad = cs == 0.0;
#pragma unroll
                for (int s = 0; s < T; ++s) {
                    const double q = a[s] / cs;
                    bad = bad || (mine[s] && !(__builtin_fabs(q) < inf));
                }
                uni = uni || ((__ballot(bad) >> gbase) & 0xFFull) != 0;
            }
        }
        const double flat = 1.0 / (double)L;                            // (L = 0: no slot takes it)
        // ---- sweep -1: the initial assignments; then `iters` sweeps.  ._1: the next site, ._2: the one after it
        if (len > 0) {
            int v_1 = P.word[s0], f_1 = P.freq[s0];
            const int n2 = len > 1 ? 1 : 0;
            int v_2 = P.word[s0 + n2], f_2 = P.freq[s0 + n2];
            double b_1[T];
            gather(v_1, word_ok(v_1, P.V), b_1);
            int zo_1 = 0;
            int nn = n2;                                                // the site whose scalars are in ._2
            uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
            for (int sweep = -1; sweep < P.iters; ++sweep) {
                for (int n = 0; n < len; ++n) {
                    const int v = v_1, f = f_1, zo = zo_1;
                    double b[T];
#pragma unroll
                    for (int s = 0; s < T; ++s) b[s] = b_1[s];
                    v_1 = v_2; f_1 = f_2;
                    gather(v_1, word_ok(v_1, P.V), b_1);
                    if (len > 1) zo_1 = P.z[s0 + nn];                   // (written a sweep ago; not read in sweep -1)
                    nn = nn + 1 < len ? nn + 1 : 0;
                    v_2 = P.word[s0 + nn]; f_2 = P.freq[s0 + nn];
                    if ((n & 15) == 0) {                                // a Philox block serves two sites: 16 sites per group
                        r0 = (uint32_t)(n >> 1) + (uint32_t)j; r1 = gdoc; r2 = P.stream_id; r3 = (uint32_t)sweep;
                        philox4x32_10(r0, r1, r2, r3, P.key0, P.key1);
                    }
                    const int holder = (n >> 1) & 7;
                    const uint32_t ra = (uint32_t)__shfl((int)((n & 1) ? r2 : r0), holder, 8);
                    const uint32_t rb = (uint32_t)__shfl((int)((n & 1) ? r3 : r1), holder, 8);
                    const double u = ((double)(ra >> 5) * 67108864.0 + (double)(rb >> 6)) * (1.0 / 9007199254740992.0);
                    if (!word_ok(v, P.V)) {                             // (group-uniform)
                        if (sweep < 0 && j == 0) {
                            P.z[s0 + n] = -1;
                            if (P.status) atomicOr(P.status, 2);
                        }
                        continue;
                    }
                    double w[T];
                    if (sweep < 0) {
                        const double cs = uni ? 1.0 : fs_sum<T>(b, R, tail);
#pragma unroll
                        for (int s = 0; s < T; ++s) w[s] = mine[s] ? (uni ? flat : b[s] / cs) : 0.0;
                        fs_shrink<T>(w, P.c_init, R, tail);
                        ntot += f;
                    } else {
                        const int go = zo & 7, so = zo >> 3;
#pragma unroll
                        for (int s = 0; s < T; ++s) ndk[s] -= (j == go && s == so) ? f : 0;       // n_dk[z] -= f
#pragma unroll
                        for (int s = 0; s < T; ++s) w[s] = mine[s] ? ((double)ndk[s] + P.alpha) * b[s] : 0.0;
                        const double S = fs_sum<T>(w, R, tail);
#pragma unroll
                        for (int s = 0; s < T; ++s) w[s] = mine[s] ? w[s] / S : 0.0;
                        fs_shrink<T>(w, P.c_loop, R, tail);
                    }
                    const int pos = draw_position<8, T, false>(w, u, 0u, true, j, lane);          // lane * T + slot, or -1
                    int zn;
                    if (pos < 0) {                                      // the reference's draw raises here
                        zn = sweep < 0 ? 0 : zo;
                        if (j == 0 && P.status) atomicOr(P.status, 1);
                    } else {
                        zn = (pos % T) * 8 + pos / T;
                    }
                    const int gn = zn & 7, sn = zn >> 3;
#pragma unroll
                    for (int s = 0; s < T; ++s) ndk[s] += (j == gn && s == sn) ? f : 0;           // n_dk[new_z] += f
                    if (j == 0) P.z[s0 + n] = zn;
                    if (len == 1) zo_1 = zn;
                }
                if (sweep >= 0 && (sweep + 1) % P.thinning == 0) {
                    const int s2 = (sweep + 1) / P.thinning;
                    const double tot = (double)ntot;
                    const double f_old = (double)(s2 - 1) / (double)s2, f_new = 1.0 / (double)s2;
#pragma unroll
                    for (int s = 0; s < T; ++s) {
                        const double cur = (double)ndk[s] / tot;
                        const double old_part = f_old * avg[s];
                        const double new_part = f_new * cur;
                        avg[s] = s2 == 1 ? cur : old_part + new_part;
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < T; ++s)
            if (mine[s]) {
                P.n_dk_s[lb + 8 * s + j] = ndk[s];
                P.th_s[lb + 8 * s + j] = avg[s];
            }
    }
}

}  // namespace
