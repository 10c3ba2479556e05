// quad_doc_map.hpp -- the lane-to-position mapping of quad_tier1_doc (kernel_quad.hpp), which plays ONE document on all 64 lanes of
// the wavefront, as plain constexpr functions.
// No HIP in here: tests/test_quad_doc_map.py compiles this file with the host compiler and walks every (lane, term).
#pragma once

// LB = log2(lanes per document) of the quad kernel: 4 / 3 / 2 for K = 512 / 256 / 128; KP = 32 << LB positions, G = 2 << LB lanes of the
// standard layout (llda_layout), device position = i << (3 + LB) | quad lane << 3 | e << 2 | c  (kernel_quad.hpp, Geometry)

// One document on 64 lanes: lane s takes the n = KP / 64 consecutive positions o = s n + t (t < n) of the document's DRAW order.
// The draw order is (standard lane g, slot a), g = 2 * quad lane + e -- quad lane, then chain A / B, then element a:  o = g << 4 | a.
constexpr int quad_doc_terms(int LB) { return 1 << (LB - 1); }                     // n: 8, 4, 2
constexpr int quad_doc_order(int LB, int s, int t) { return s * quad_doc_terms(LB) + t; }
constexpr int quad_doc_std_lane(int o) { return o >> 4; }                          // g: P.lab_mask[d * G + g] is the validity word ...
constexpr int quad_doc_std_slot(int o) { return o & 15; }                          // ... and a its bit
constexpr int quad_doc_lane(int o) { return o >> 5; }                              // quad lane: thread tbase + it holds the counts
constexpr int quad_doc_chain(int o) { return (o >> 4) & 1; }                       // e
constexpr int quad_doc_rho(int o) { return 8 * ((o & 15) >> 2) + 2 * (o & 3) + ((o >> 4) & 1); }
constexpr int quad_doc_pos(int LB, int o) { return ((o & 15) >> 2) << (3 + LB) | (o >> 5) << 3 | ((o >> 4) & 1) << 2 | (o & 3); }
// byte of the word's row in the 16-bit image (llda_pack_rows16_all: piece (j = a >> 3, e) of quad lane lq is the 16-byte unit
// (2 j + e) * LPD + lq, the counts of slots 8 j .. 8 j + 7 in order): a lane's n counts are 2 n contiguous, 2 n-aligned bytes
constexpr int quad_doc_image_byte(int LB, int o)
{
    return (2 * ((o & 15) >> 3) + ((o >> 4) & 1)) * (16 << LB) + 16 * (o >> 5) + 2 * (o & 7);
}
