// kernel_lrsparse.hpp -- llda_leftright_sparse_kernel: the left-to-right estimate of p(w_d | labels_d) on sparse label sets
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_left_to_right_sparse (include/llda_gibbs.h): llda_left_to_right for documents that carry a handful of the K
// labels, K up to LLDA_MAX_K.  The label sets are kernel_docsparse.hpp's CSR (label_slot, without loads).
//
// Arithmetic: the header text of llda_left_to_right on the document's compacted problem -- K' = L_d, phi_t'[w][j] = phi_t[w][lab[j]],
// every topic allowed, A = L_d, the same doc ids, stream_id + r, seed and u(n, r, m).  Compacted topic j sits in lane j, slot 0 of
// the plain 64-lane layout.  Here lane j of a group of G = 8, 16 or 32 >= max_labels lanes holds it, and the bits are the same:
//   draw64   the lanes >= L_d hold x = +0.0 and x is never -0.0.  A Hillis-Steele step d adds X[j - d] to X[j] for j >= d: the
//            steps d >= G do not reach the lanes < G, so the scan over G lanes (group_scan<G>) gives the 64-lane prefixes of the
//            lanes < G.  X[63] of 64 lanes is X[31] + (lanes 32 .. 63) = X[31] + 0.0, X[31] is X[15] + 0.0 for G <= 16, and so
//            on: X[63] = X[G-1].  The lanes >= G have x = 0 and are never drawn.
//   sum64    doc_tree<G>: the steps s >= G of the tree add +0.0 to a sum that is never -0.0 (doc_model.hpp).
// So the kernel equals llda_left_to_right on the compacted problem bit for bit, and for the prefix label sets {0 .. L_d - 1} also
// llda_left_to_right at full K with the prefix as the allowed row.
//
// Geometry.  One workgroup per document.  Particle r is the lane group threadIdx.x / G: a wavefront carries 64 / G particles, the
// workgroup has ceil(R G / 64) <= 8 wavefronts and the groups past R sit out.  A lane holds ONE count, that of its slot.  The
// document's words (32 bits) and every particle's assignments (the slot, 8 bits, 0xFF = NONE) stay in LDS, sized by
// max_doc_tokens.  The word at position m is uniform over the workgroup: every group gathers the same L_d doubles of phi_t[w_m],
// a site costs L_d * 8 bytes whatever K is, and the loading of position m + 1 is fetched while position m is drawn.
// Whether a position holds an assignment and whether 0 < S_r < inf are properties of the PARTICLE: what llda_leftright_kernel
// decides by a wavefront-uniform branch is a per-group predicate (act, draw) here, and every cross-lane operation (doc_tree,
// group_scan, the ballots, the shuffles) is executed by all 64 lanes at every m: the loops run 0 .. n in every lane, and only the
// updates of c, assigned and z are predicated.  The Philox blocks of a group come from its own G lanes, 2 G positions m per batch,
// under the group's stream_id + r.  One barrier per position: the groups leave pred_r in LDS (two buffers, by the parity of n),
// wavefront 0 adds them in increasing r and multiplies the pair.  N and the document's fitness are uniform over the workgroup, so
// every wavefront reaches every barrier.
// An unfit document: every token is bad, nothing is drawn and no label id is used as an index.  L_d = 0: A = 0, x = 0 everywhere,
// pred = 0 / 0 = NaN: every token is bad.
// ---------------------------------------------------------------------------------------------
struct LrSparseParams : LrParams {                      // allowed / ld_allowed are not used: the label lists take their place
    LabelSets sets;                                     // (theta_s is not used)
};

constexpr int LRS_NONE = 0xFF;                          // no assignment (a slot is < 32)
constexpr int LRS_MAX_THREADS = 512;                    // 16 particles of 32 lanes

// bytes of dynamic LDS: pred[2][16] doubles, word[cap] int32, z[R][cap] uint8: at most 82 176
inline size_t lrs_lds_bytes(int R, int cap) { return LR_PRED_BYTES + (size_t)cap * 4 + (size_t)R * cap; }

template <int G>
__global__ void __launch_bounds__(LRS_MAX_THREADS) llda_leftright_sparse_kernel(const LrSparseParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lrs_lds[];
    const int lane = threadIdx.x & 63, gl = threadIdx.x % G, r = threadIdx.x / G;
    const int cap = P.cap, R = P.R;
    const bool particle = r < R;                                        // the group holds one
    const int shift = lane & ~(G - 1);                                  // the group's first lane
    const uint32_t gmask = G == 32 ? ~0u : (1u << G) - 1u;
    double *s_pred = (double *)lrs_lds;                                 // [2][LR_MAX_PARTICLES]
    int32_t *s_word = (int32_t *)(lrs_lds + LR_PRED_BYTES);             // [cap]
    uint8_t *s_z = (uint8_t *)(s_word + cap) + (size_t)(particle ? r : 0) * cap;      // [cap], this particle's
    const double alpha = P.alpha, inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const uint32_t stream = P.stream_id + (uint32_t)r;
    for (int64_t d = blockIdx.x; d < P.D; d += gridDim.x) {
        const int64_t b = P.doc_off[d], len = P.doc_off[d + 1] - b;
        const bool over = len > (int64_t)cap;
        const int N = (len < 0 || over) ? 0 : (int)len;
        const LabelSlot ls = label_slot<G, false>(P.sets, d, true, gl, P.K);      // (every group reads the same list)
        __syncthreads();                                                // the previous document's words and predictions are done with
        for (int i = threadIdx.x; i < N; i += blockDim.x) s_word[i] = P.word[b + i];
        __syncthreads();
        if (!ls.fit) {                                                  // (uniform over the workgroup)
            if (threadIdx.x == 0) {
                if (over && P.status) atomicOr(P.status, 1);
                P.mant[d] = 0.5; P.expo[d] = 1; P.tok[d] = 0; P.bad[d] = N;
            }
            continue;
        }
        const double a_alpha = (double)(int)ls.L * alpha;               // A = L_d
        const uint32_t gdoc = P.doc_ids ? (uint32_t)P.doc_ids[d] : (uint32_t)(d + P.doc_base);
        const double *pcol = P.phi_t + ls.k;                            // the lane's column (column 0 where it has none: not read)
        auto loading = [&](const int w, const bool ok) { return (ok && ls.mine) ? pcol[(int64_t)w * P.ld_phi] : 0.0; };
        int c = 0, assigned = 0;                                        // the count of the lane's slot; the particle's assignments
        double dm = 0.5;                                                // the document's pair and counters (N <= 4096: 32 bits do)
        int de = 1, dtok = 0, dbad = 0;
        for (int n = 0; n < N; ++n) {
            uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
            int batch = -1;                                             // the 2 G positions m whose Philox blocks the group's lanes hold
            double pred = nan;
            int w = s_word[0];
            bool ok = word_ok(w, P.V);
            double v = loading(w, ok);
            // m < n: resampling of the earlier positions that hold an assignment, in order; m == n: prediction and extension
            for (int m = 0; m <= n; ++m) {
                const bool last = m == n;
                const int wn = s_word[last ? m : m + 1];                // the next position's loading, in flight during this draw
                const bool okn = word_ok(wn, P.V);
                const double vn = loading(wn, okn);
                if ((m / (2 * G)) != batch) {                           // (uniform over the workgroup)
                    batch = m / (2 * G);
                    r0 = (uint32_t)(batch * G + gl); r1 = gdoc; r2 = stream; r3 = (uint32_t)n;
                    philox4x32_10(r0, r1, r2, r3, P.key0, P.key1);
                }
                const int holder = (m >> 1) & (G - 1);
                const uint32_t ra = (uint32_t)__shfl((int)((m & 1) ? r2 : r0), holder, G);
                const uint32_t rb = (uint32_t)__shfl((int)((m & 1) ? r3 : r1), holder, G);
                const double u = ((double)(ra >> 5) * 67108864.0 + (double)(rb >> 6)) * (1.0 / 9007199254740992.0);
                const int zo = (particle && !last) ? (int)s_z[m] : LRS_NONE;
                const bool act = particle && (last || zo != LRS_NONE);  // (m < n: the position was assigned, so its word is ok)
                c -= (gl == zo) ? 1 : 0;                                // (NONE is no lane)
                const double x = ls.mine ? ((double)c + alpha) * v : 0.0;
                bool draw = act;
                if (last) {
                    const double sum = doc_tree<G>(0.0 + x);
                    const double S = ok ? sum : nan;
                    pred = S / ((double)assigned + a_alpha);
                    draw = act && S > 0.0 && S < inf;
                }
                // draw64 over the group's lanes: one slot per lane, so a lane's own prefix is x
                const double X = group_scan<G>(x, gl);
                const double t = u * bcast_last<G>(X, lane);
                const double prev = __shfl_up(X, 1, 64);
                const double tg = t - (gl ? prev : 0.0);
                const bool pos = x > 0.0;
                const uint32_t gf = (uint32_t)(__ballot(pos && x > tg) >> shift) & gmask;
                const uint32_t gp = (uint32_t)(__ballot(pos) >> shift) & gmask;
                const int hit = gf ? (int)__ffs((int)gf) - 1 : 31 - (int)__clz((int)(gp | 1u));
                const int zn = (draw && gp != 0) ? hit : zo;            // (m < n: the old slot; m == n: none)
                if (act && zn != LRS_NONE) {
                    c += (gl == zn) ? 1 : 0;
                    assigned += last ? 1 : 0;
                }
                if (act) s_z[m] = (uint8_t)zn;                          // (every lane of the group the same value)
                w = wn; ok = okn; v = vn;
            }
            double *pr = s_pred + (n & 1) * LR_MAX_PARTICLES;
            if (particle) pr[r] = pred;                                 // (every lane of the group the same value)
            __syncthreads();
            if (threadIdx.x < 64) {
                double acc = 0.0;
                for (int i = 0; i < R; ++i) acc = acc + pr[i];
                const double p = acc / (double)R;
                const bool good = p > 0.0 && p < inf;
                dtok += good ? 1 : 0;
                dbad += good ? 0 : 1;
                if (good) pair_mul_frexp(dm, de, p);
            }
        }
        if (threadIdx.x == 0) {
            if (over && P.status) atomicOr(P.status, 1);
            P.mant[d] = dm; P.expo[d] = de; P.tok[d] = dtok; P.bad[d] = dbad;
        }
    }
}

}  // namespace
