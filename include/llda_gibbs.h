/* llda_gibbs.h -- C ABI of the MI355X-native collapsed-Gibbs sweep for Labeled LDA / CascadeLDA.
 *
 * The reference (KenHBS/LDA_thesis) is pure Python and has no FFI boundary of its own; the hot path
 * is the method  LabeledLDA.training_iteration  (/root/reference/LabeledLDA.py:101-125), byte-for-byte
 * the same body as  SubLDA.training_iteration  (/root/reference/CascadeLDA.py:397-421).  This header
 * is the boundary a maintainer binds (ctypes stub in INTEGRATION.md) to replace those two methods,
 * the count initialisation loops (LabeledLDA.py:89-92, CascadeLDA.py:382-385) and the thinning
 * read-outs (LabeledLDA.py:231-239, :256-265).  ABI 22 adds what the reference does not have: llda_count_hist, the counts of
 * counts from which alpha and beta (0.001 there: CascadeLDA's constants and the defaults of train_it) are estimated while training.
 *
 * Conventions
 *   - every pointer marked [dev] is a DEVICE pointer (HBM of the current HIP device); the library
 *     allocates nothing persistent and owns none of the buffers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all entry points only
 *     ENQUEUE work and return without synchronising unless stated otherwise;
 *   - return value 0 = success, negative = LLDA_E_* (see llda_strerror); HIP failures are returned
 *     as LLDA_E_HIP and the hipError_t is available from llda_last_hip_error(); nothing throws;
 *   - one host thread per device; entry points are re-entrant across devices.
 *
 * Device layout ("group layout")
 *   The K topics of a document are spread over G lanes x T slots; per-topic arrays are stored in
 *   device order with padded row length KP = G*T.  The position of (lane, slot) in a row is
 *       pos = ((slot / 4) * G + lane) * 4 + slot % 4      when T is a multiple of 4
 *       pos = lane * T + slot                               when T is 1 or 2
 *   i.e. the 16-byte chunk `slot / 4` of ALL lanes is contiguous, so that every vector load of a wavefront reads
 *   one contiguous run of the row (llda_layout.pos_lane / pos_slot / topic_pos hold the permutation):
 *       n_kw  [V][KP] int32   word-major  (the reference's n_k_v (K,V) transposed + permuted)
 *       n_dk  [D][KP] int32   (the reference's n_d_k (D,K) permuted)
 *       n_k   [KP]    int32   (the reference's n_zk permuted)
 *       z     [S]     int32   topic of every site, stored as device POSITION (not topic id)
 *       lab_mask [D][G] uint16   bit s of [d][g] = labs[d][topic at (g,s)]
 *   llda_layout() returns the permutation so the host can convert to and from reference order.
 */
#ifndef LLDA_GIBBS_H
#define LLDA_GIBBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLDA_ABI_VERSION 22
#define LLDA_MAX_K 7688          /* every K up to here splits into <= 64 pairwise leaves                       */
#define LLDA_MAX_KP 8192         /* longest padded row: 64 leaves x 128                                        */
#define LLDA_MAX_LEAVES 8        /* "narrow" layouts: one lane group of <= 64 lanes x <= 16 slots per document  */
#define LLDA_MAX_WIDE_LEAVES 64  /* "wide" layouts (more than 8 leaves: some K in 969..1023, every K > 1024)    */
#define LLDA_MAX_ROUNDS 4

enum {
    LLDA_OK = 0,
    LLDA_E_BAD_K = -1,      /* K outside 1..LLDA_MAX_K, or an entry point that only takes narrow layouts */
    LLDA_E_BAD_ARG = -2,    /* NULL pointer, negative size, layout fields do not match K   */
    LLDA_E_HIP = -3,        /* a HIP runtime call failed (see llda_last_hip_error)          */
    LLDA_E_NO_DEVICE = -4   /* no gfx950 device visible                                     */
};

/* Layout of K topics over the lanes of a wavefront (host-side description).
 * Narrow layouts (n_leaves <= 8): G = 8 * (leaves rounded up to a power of two) <= 64 lanes per document, 64/G documents
 * per wavefront.  Wide layouts (wide = 1; ABI 13): G = 8 * (leaves rounded up to a multiple of 8) = 64 * tiers; the G
 * "lanes" of the formulas above are VIRTUAL lanes, virtual lane gv = 64 * tier + physical lane of the one wavefront that
 * walks the document; T is 8, 12 or 16.  The leaf totals of a wide layout are combined along numpy's recursion tree by
 * n_leaves - 1 in-place adds  total[comb_dst[i]] += total[comb_src[i]]  (post-order; total[0] is the sum).  Every entry
 * point takes wide layouts except llda_sweep_batch (its problems have at most 128 topics). */
typedef struct llda_layout {
    int32_t K;                       /* number of topics (labels incl. 'root')                */
    int32_t n_leaves;                /* numpy pairwise-sum leaves                             */
    int32_t G;                       /* lanes per document: 8, 16, 32, 64; wide: 64 * tiers   */
    int32_t T;                       /* slots per lane: 1, 2, 4, 8, 12 or 16                  */
    int32_t KP;                      /* G*T                                                   */
    int32_t tail;                    /* K % 8 of the last leaf                                */
    int32_t tail_row;                /* slot that holds the tail topics                       */
    int32_t n_rounds;                /* leaf-combine rounds (narrow)                          */
    int32_t wide;                    /* 1: more than 8 leaves                                 */
    int32_t tiers;                   /* wide: G / 64; narrow: 0                               */
    int32_t leaf_start[LLDA_MAX_WIDE_LEAVES];
    int32_t leaf_len[LLDA_MAX_WIDE_LEAVES];
    int32_t rounds[LLDA_MAX_ROUNDS][LLDA_MAX_LEAVES];   /* narrow: partner leaf per round (self = idle) */
    int32_t comb_dst[LLDA_MAX_WIDE_LEAVES];             /* numpy's recursion tree, post-order (n_leaves - 1 entries) */
    int32_t comb_src[LLDA_MAX_WIDE_LEAVES];
    int32_t topic_pos[LLDA_MAX_KP];  /* topic id -> device position                           */
    int32_t pos_topic[LLDA_MAX_KP];  /* device position -> topic id, -1 in the padding        */
    int32_t pos_lane[LLDA_MAX_KP];   /* device position -> (virtual) lane that holds it        */
    int32_t pos_slot[LLDA_MAX_KP];   /* device position -> slot of that lane (bit of lab_mask) */
} llda_layout;

/* Arguments of one sweep over a shard of documents.
 * Replaces the loop body of LabeledLDA.training_iteration (LabeledLDA.py:106-125) for documents
 * [doc_base, doc_base + D) under per-document snapshot semantics: every document reads the
 * sweep-start n_kw / n_k plus its own changes; count changes are accumulated into the *_delta
 * buffers with integer atomics (order independent => deterministic). */
typedef struct llda_sweep_args {
    const int64_t  *doc_off;     /* [dev] [D+1] site offsets                                  */
    const int32_t  *doc_order;   /* [dev] [D] processing order (local doc ids) or NULL        */
    const int32_t  *word;        /* [dev] [S] word id of every site (unique, ascending per doc) */
    const int32_t  *freq;        /* [dev] [S] frequency f of every site, 0 <= f < 2^23 (not checked on the device) */
    int32_t        *z;           /* [dev] [S] in/out: device position of the site's topic      */
    const uint16_t *lab_mask;    /* [dev] [D*G] lane masks                                     */
    int32_t        *n_dk;        /* [dev] [D*KP] in/out                                        */
    const int32_t  *n_kw;        /* [dev] [V*KP] sweep-start snapshot (read only)              */
    int32_t        *n_kw_delta;  /* [dev] [V*KP] += sweep changes                              */
    const int32_t  *n_k;         /* [dev] [KP] sweep-start snapshot (read only)                */
    int32_t        *n_k_delta;   /* [dev] [KP] += sweep changes                                */
    int32_t        *status;      /* [dev] optional (may be NULL), int32[4]: word 0 bit 0 is set when a site had no
                                    topic with positive probability (the reference would raise);
                                    bit 1 (informational) when some site took the exact tier;
                                    bit 2 when llda_pack_rows16 met a count outside 0 .. 65535 in a flagged row, or the
                                    four-wave 16-bit-row kernel an entry of n_dk above 65535 (max_doc_tokens was not a bound);
                                    word 1 += sites the fp32 tier was unsure about, word 2 += sites that
                                    reached the exact tier (statistics)                           */
    int64_t  D;                  /* local documents                                            */
    int64_t  V;                  /* vocabulary size (rows of n_kw; also enters den = n_k + V*beta) */
    int32_t  K;                  /* topics                                                     */
    int32_t  docs_per_group;     /* documents a lane group walks per workgroup (>=1; 0 = auto) */
    int32_t  dense_mask;         /* 1 = lab_mask allows every topic in every document (the kernel may
                                    then skip applying it); 0 = general                            */
    int32_t  debug_margin;       /* 0 in production.  Test hook of the tiered draw (dm below; csrc/sweep_plan.hpp is the one place
                                    that reads it, tests/test_sweep_plan_host.py checks this table).  Results never depend on it.
                                    Margins every kernel family starts from:
                                      tier 1 (fp64)  2^-40 of the total score for dm == 0 and -8 <= dm <= -2; 2^-dm for dm > 0 (wider:
                                                     more sites take the exact tier); off (every site exact) for dm == -1, dm <= -9
                                      tier 0 (fp32)  production for dm in {0, -8}; 2^-dm for 1 <= dm <= 15; off otherwise
                                    Sparse label sets (live_off / live_pos): any dm < 0 sends every site through the exact pipeline.
                                    Wide layouts with a dense or general mask:
                                      dm >= -1  the fp32-tiered kernel (tier 0: production margin at 0, 2^-dm for 1 .. 15, else off);
                                                like -6 and -7 it needs 0 < max_doc_tokens < 32768, the register kernel runs otherwise
                                      -2, -5    the fp64 register kernel without the fp32 tier
                                      -3        the same decision on the kernel that keeps nothing of the row in registers
                                      -4        the register kernel with LDS copies of the counts whatever max_doc_tokens says
                                      -6        the fp32-tiered kernel with fp64 factors in LDS even when scratch is there
                                      -7        the fp32-tiered kernel with fp32 factors only whenever scratch is there
                                      <= -8     the fp64 register kernel (-8: production tier 1; below: every site exact)
                                    With n_kw16 and site_row:  -8  production margins on the three-wave form of the 16-bit-row kernel.
                                    With row16 (the quad kernel; tier 1 in production for -9 ... -18):
                                      0           its data-dependent tier-0 margin
                                      -9          the constant tier-0 margin 104 * 2^-24 of the total instead
                                      -10 .. -18  the data-dependent margin scaled by 1 / 1.05 (the derived error bound itself), 1/2, 1/4 ...
                                                  1/256: tests/neartie.py measures how much of it the worst planted tie needs
                                      other dm    the margins every family starts from                                        */
    double   alpha, beta;        /* priors (LabeledLDA.py:55-56)                               */
    uint64_t seed;               /* RNG key                                                    */
    uint32_t sweep;              /* RNG counter word 3                                         */
    uint32_t stream_id;          /* RNG counter word 2 (sub-problem id for CascadeLDA)         */
    int64_t  doc_base;           /* global id of local document 0 (RNG counter word 1)         */
    /* optional sparse-label path (live_off, live_pos non-NULL and live_max <= 64): one lane per allowed
     * topic instead of one lane per 16 topics */
    const int64_t *live_off;     /* [dev] [D+1] offsets into live_pos                              */
    const int32_t *live_pos;     /* [dev] device positions of the topics every document allows, in DRAW order:
                                  * ascending (lane, slot) of the layout -- llda_layout.pos_lane / pos_slot --,
                                  * which for layouts with T >= 8 is not ascending memory position          */
    void          *scratch;      /* [dev] optional (ABI 14) work space: llda_sweep_scratch_bytes(K, D) bytes, contents irrelevant.
                                    Wide layouts of three or four tiers (K = 1 929 ... 3 848) with a dense or general label mask
                                    keep fp32 factors only in LDS when it is there (more wavefronts per CU) and run the rare
                                    fp64 / exact tiers on it.  NULL or too small: the same result from the kernel that keeps
                                    fp64 factors in LDS (14 % slower there)                                                 */
    int64_t  scratch_bytes;      /* size of scratch                                                        */
    int32_t  live_max;           /* largest number of allowed topics of any document                  */
    int32_t  max_doc_tokens;     /* (ABI 13) optional hint, 0 = unknown: an upper bound of every entry of n_dk of the call --
                                    the tokens (sum of freq, plus any phantom counts) of its largest document.  Wide layouts:
                                    below 32 768 the kernel keeps the document's count CHANGES as int16 in LDS instead of copies
                                    of the counts (more wavefronts per CU).  With n_kw16: below 65 536 the kernel packs n_dk with
                                    its sweep-start value into one LDS word and runs FOUR waves per SIMD instead of three
                                    (debug_margin -8: three regardless); an entry above the bound sets status bit 2         */
    /* optional commit log (both non-NULL): instead of two int32 atomics on n_kw_delta per changed site the
     * kernels store ONE word (old position | new position << 16) at the site's place in WORD-major order;
     * llda_commit_log then folds the log into the counts word by word without global atomics.  (No-return
     * global atomics saturate at ~27 G/s on MI355X, scattered 4-byte stores at ~88 G/s: tools/atomic_ubench.hip.)
     * n_kw_delta is not touched in this mode. */
    const int32_t *csc_pos;      /* [dev] [S] index of every site in word-major (stable) order; with row16 (the
                                    kernels of four and more documents per wavefront) every index below 2^30       */
    uint32_t      *commit_log;   /* [dev] [S] out, word-major                                         */
    int64_t  n_sites;            /* doc_off[D] - doc_off[0], the sites this call spans: must be < 2^30 (the hot
                                    kernel addresses word / freq / z / csc_pos as base + 32-bit byte offset from
                                    the first document of the call).  Larger shards: one call per document
                                    range -- pass doc_off + d0, D = d1 - d0, n_dk + d0*KP, lab_mask + d0*G,
                                    doc_base + d0 (and live_off + d0); every other pointer stays as it is. */
    const int32_t *site_rec;     /* [dev] [S][4] optional (ABI 12), with the commit log: {word, freq, csc_pos, 0} of
                                    every site as one 16-byte record.  Layouts with 8 or 16 lanes per document (K <= 256)
                                    read it instead of the three arrays: a wavefront then walks 8 / 4 documents and
                                    every scalar load touches that many cache lines, which makes the vector-memory
                                    address pipeline the bound.  A call that passes it with such a layout may span at
                                    most 2^28 - 1 sites. */
    const uint16_t *n_kw16;      /* [dev] [V*KP] optional (ABI 15): the 16-bit image of n_kw written by llda_pack_rows16 for THIS
                                    sweep's n_kw.  Sites whose csc_pos has bit 31 set read their word's row from it (half the
                                    bytes for the rows that miss the L2); the caller sets the bit for the sites of flagged
                                    words only.  Taken by the dense 16-slot kernel with the commit log (llda_rows16_ok(K),
                                    dense_mask = 1, alpha, beta >= 1e-6); LLDA_E_BAD_ARG on any other path.  Results do
                                    not depend on it. */
    const int32_t *site_row;     /* [dev] [S] with n_kw16 (ABI 16; LLDA_E_BAD_ARG when one comes without the other): where the
                                    row of a site's word starts, in 16-byte units from n_kw --  word * KP / 4  for an int32 row,
                                    ((char *)n_kw16 - (char *)n_kw) / 16 + word * KP / 8  for a 16-bit one (int32 offsets: the caller
                                    carves both arrays out of ONE allocation, so the distance is a constant of V and KP).  Static: which words are flagged never changes.  The kernel reads it
                                    INSTEAD of word -- the choice between the two images costs it no instruction. */
    const void    *n_kw_img;     /* [dev] [V*KP] optional (ABI 18), sparse label sets only (live_off / live_pos; LLDA_E_BAD_ARG on
                                    any other path): the narrow image of THIS sweep's n_kw written by llda_pack_image -- one
                                    byte (img_bits 8) or one 16-bit word (img_bits 16) per count, SATURATING at 255 / 65535.
                                    The sparse-label kernel gathers its counts from the image (a row spans a quarter / half
                                    as many cache lines; that kernel is bound by L2 line fills) and re-reads an entry that
                                    shows the saturation value from n_kw itself, so any count is legal and the results do not
                                    depend on the image.  Needs alpha, beta >= 1e-6 like the sparse-label kernel itself. */
    int32_t  img_bits;           /* 0 (no image), 8 or 16                                                    */
    int32_t  reserved_img;       /* 0                                                                         */
    const uint8_t *row16;        /* [dev] [V] optional (ABI 19), with n_kw16 and WITHOUT site_row: the per-word flags llda_pack_rows16_all
                                    wrote for THIS sweep's n_kw (1 = every count of the row fits 16 bits; n_kw16 then holds EVERY
                                    row).  K with llda_quad_ok (512; ABI 21: the layouts of 16 slots per lane with 8, 16 or 32 lanes), dense_mask = 1, the commit log,
                                    alpha, beta >= 1e-6, 0 < max_doc_tokens < 65 536 and, for K = 128 and 256, site_rec (LLDA_E_BAD_ARG otherwise): the kernel that
                                    walks a document with K / 32 lanes x 32 slots (kernel_quad.hpp), FOUR documents per wavefront at
                                    K = 512, eight at 256, sixteen at 128 -- the per-iteration work of scan, search, pick and count
                                    update is shared by that many sites.  A site whose row is not flagged
                                    reads the int32 row (no prefetch: meant to be rare).  Bit 31 of csc_pos is ignored.  The kernel
                                    forms 32-bit byte offsets into n_kw16 and into the commit log: V < 2^22 (LLDA_E_BAD_ARG
                                    otherwise), and every csc_pos below 2^30 -- a bound on the sites of the whole LOG, which a shard
                                    cut into several calls shares; llda_sweep sees one call's n_sites and cannot check it.  Results
                                    do not depend on it. */
    const int32_t *img_col;      /* [dev] [KP] optional (ABI 20), with n_kw_img: the image column that holds the count of every device
                                    position -- the inverse of the col_src handed to llda_pack_image_cols.  The sparse-label kernel is
                                    bound by the L2's line fills: an image whose columns are ordered so that topics which are allowed
                                    TOGETHER sit in one 128-byte line costs a site fewer fills.  NULL: column = position
                                    (llda_pack_image).  Results do not depend on it. */
} llda_sweep_args;

/* ---- host-only (no device needed) ---- */
int         llda_abi_version(void);
/* 0 for the production build.  Otherwise one bit per compile-time switch the library was built with (ABI 17): overrides of the
 * draw margins / occupancy bound, and the ablation switches of tools/ that delete work from the kernels.  A number measured
 * with a non-zero build is not a measurement of the product: bench.py refuses to print one. */
#define LLDA_BUILD_MARGIN0            0x001   /* -DLLDA_MARGIN0=...       tier-0 margin of the narrow kernels            */
#define LLDA_BUILD_WAVES              0x002   /* -DLLDA_WAVES=...         waves per SIMD the narrow kernels are bounded to */
#define LLDA_BUILD_MARGIN0_WIDE       0x004   /* -DLLDA_MARGIN0_WIDE=...                                                */
#define LLDA_BUILD_ABL_NOLOAD         0x008   /* -DABL_NOLOAD             no n_kw row loads                               */
#define LLDA_BUILD_ABL_NOCOMMIT       0x010   /* -DABL_NOCOMMIT           no count updates                                */
#define LLDA_BUILD_ABL_WIDE_NOROW     0x020   /* -DABL_WIDE_NOROW                                                         */
#define LLDA_BUILD_ABL_WIDE_NOADDLOAD 0x040   /* -DABL_WIDE_NOADDLOAD                                                     */
#define LLDA_BUILD_ABL_NOFMA          0x080   /* -DABL_NOFMA                                                              */
#define LLDA_BUILD_ABL_EXTRA_LDS      0x100   /* -DABL_EXTRA_LDS_BYTES=n  unused dynamic LDS (occupancy ablation)          */
#define LLDA_BUILD_QUAD_PROFILE       0x200   /* -DQUAD_PROFILE           shader-clock stamps in the quad kernel (status[8..]) */
#define LLDA_BUILD_BUDGET_MARKS       0x400   /* -DLLDA_BUDGET_MARKS      class marks in the assembly of the site loops (counting only) */
#define LLDA_BUILD_QUAD_PRIO          0x800   /* -DLLDA_QUAD_PRIO=tdb     issue priorities of the quad kernels' phases (experiments)     */
int         llda_build_info(void);
const char *llda_strerror(int code);
int         llda_last_hip_error(void);
/* sizeof of the argument structs as the library was compiled (0 llda_layout, 1 llda_sweep_args, 2 llda_batch_args,
 * 3 llda_foldin_args, 4 llda_rank_args, 5 llda_heldout_args, 6 llda_attr_args): a binding checks its own struct definitions against it once, at load time. */
int         llda_struct_size(int which);
/* Fill *out for K topics.  Mirrors numpy's pairwise-sum recursion (np.sum at LabeledLDA.py:117). */
int         llda_layout_init(int32_t K, llda_layout *out);

/* Bytes of llda_sweep_args.scratch that let llda_sweep(K, D documents per call) run its fastest kernel (0 for layouts that
 * need none: every narrow layout).  Host only. */
int64_t     llda_sweep_scratch_bytes(int32_t K, int64_t D);
/* 1 when llda_sweep can read 16-bit rows for K topics (narrow layout, 16 slots per lane, 32 or 64 lanes, no padded slot:
 * K = 512 and K = 1024).  Host only. */
int         llda_rows16_ok(int32_t K);
/* 1 when llda_sweep takes llda_sweep_args.row16 for K topics (ABI 21; narrow layout of 16 slots per lane whose 8, 16 or 32 lanes all
 * belong to a leaf of numpy's pairwise sum: K = 97 .. 128 (one leaf), 185 .. 248 without 192 and 256 (two), 361 .. 488 without 368,
 * 376, 384 and 496, 504, 512 (four) -- K = 100, 120, 200, 240, 400, 480 as well as 128, 256, 512; not 250 (three leaves in a four-leaf
 * layout) or 500 (five leaves).  Positions without a topic
 * keep the factor 0, the exact tier sums in numpy's order for K.  Host only. */
int         llda_quad_ok(int32_t K);

/* ---- device entry points (enqueue on `stream`) ---- */
/* One Gibbs sweep over the shard: LabeledLDA.py:101-125 / CascadeLDA.py:397-421. */
int llda_sweep(const llda_sweep_args *args, void *stream);

/* One Gibbs sweep over MANY independent small problems in ONE launch: the ensemble of per-node sub-problems of
 * CascadeLDA.go_down_tree (/root/reference/CascadeLDA.py:135-184; each is SubLDA.training_iteration,
 * CascadeLDA.py:397-421).  A "document instance" is a document as a member of one sub-problem.  All problems
 * share the vocabulary (V) and the priors; problem p keeps its fused [n_kw (V x KP_p) | n_k (KP_p)] counts at
 * counts + kw_off[p] / counts + nk_off[p], and its changes are added (int32 atomics) at the same offsets of
 * `delta`; the caller folds with llda_apply_delta(counts, delta, total) after the launch(es) of a sweep.
 * The draw key is (seed; sweep, stream = prob_stream[inst_prob[i]], doc = inst_doc[i], site) -- what llda_sweep uses
 * with that stream_id and doc_base = 0 on the problem alone, so both paths leave identical states.
 * Arithmetic: one lane per ALLOWED topic (every instance of a launch has <= `lanes` allowed topics, lanes in
 * {8, 16, 32, 64}); the draw is decided from unnormalised fp64 prefix sums with a 2^-40 margin (it then equals the
 * reference pipeline's choice); a site that cannot be decided that way (~1e-11 per site) goes through
 * the reference's exact fp64 pipeline inside the kernel (status word 2 counts them).  An instance without an allowed
 * topic (live_off[i+1] == live_off[i]) is legal: each of its sites has total 0, takes the exact tier, finds no topic with
 * a positive probability and keeps its z -- bit 0 of status word 0 is set, n_dk and delta get nothing from it.
 * Needs alpha, beta >= 1e-6,
 * V*beta < 2^40 (LLDA_E_BAD_ARG otherwise) and K_p <= 128 for every problem (the caller's responsibility). */
typedef struct llda_batch_args {
    const int64_t *inst_off;     /* [dev] [I+1] site offsets of all document instances               */
    const int32_t *order;        /* [dev] [n_inst] the instances this launch samples                  */
    int64_t        n_inst;
    const int32_t *word;         /* [dev] [S] word id per instance site                               */
    const int32_t *freq;         /* [dev] [S]                                                         */
    int32_t       *z;            /* [dev] [S] in/out device positions (layout of the instance's problem) */
    const int32_t *inst_prob;    /* [dev] [I] problem of every instance                               */
    const int32_t *inst_doc;     /* [dev] [I] index of the document inside its problem (RNG word 1)   */
    const int64_t *live_off;     /* [dev] [I+1] offsets into live_pos                                 */
    const int32_t *live_pos;     /* [dev] allowed device positions of every instance, in DRAW order
                                  * (ascending (lane, slot) of the instance's layout, see llda_sweep_args) */
    const int64_t *ndk_off;      /* [dev] [I] offset of the instance's n_dk row (KP_p entries) in n_dk */
    int32_t       *n_dk;         /* [dev] in/out                                                      */
    const int64_t *kw_off;       /* [dev] [P] offset of problem p's n_kw in counts / delta            */
    const int64_t *nk_off;       /* [dev] [P] offset of problem p's n_k                               */
    const int32_t *kp;           /* [dev] [P] KP_p                                                    */
    const int32_t *prob_stream;  /* [dev] [P] RNG counter word 2 of problem p                         */
    const int32_t *k;            /* [dev] [P] topics of problem p: 1 <= K_p <= 128 (one numpy pairwise leaf)  */
    const int32_t *counts;       /* [dev] sweep-start snapshot (read only)                            */
    int32_t       *delta;        /* [dev] += sweep changes                                            */
    int32_t       *status;       /* [dev] optional int32[4] as in llda_sweep_args                       */
    int64_t  V;
    int32_t  lanes;              /* lanes per instance: 8, 16, 32 or 64                               */
    int32_t  debug_margin;       /* 0 in production; n > 0 widens the margin to 2^-n; < 0: every site through the exact pipeline */
    double   alpha, beta;
    uint64_t seed;
    uint32_t sweep, reserved;
} llda_batch_args;
int llda_sweep_batch(const llda_batch_args *args, void *stream);

/* n_kw[i] += delta[i]; delta[i] = 0  for i < n   (end-of-sweep fold, after the all-reduce of delta).  Any n >= 0 and any 4-byte
 * aligned pointers are taken; 16-byte aligned ones are folded four counts per access, and a group of four whose deltas are all zero
 * is not written. */
int llda_apply_delta(int32_t *counts, int32_t *delta, int64_t n, void *stream);

/* Fold a commit log into word-major counts (the deferred `+= f` / `-= f` of LabeledLDA.py:109-111,123-125).
 * The log is cut into ITEMS of consecutive entries of ONE word: item i covers log[item_begin[i] ..
 * item_begin[i] + item_len[i]) and belongs to word item_word[i] & 0x7fffffff; bit 31 of item_word is set when
 * the word is spread over several items (their rows are then combined with atomics, all others with plain
 * read-modify-writes).  One wavefront per item accumulates a KP-entry histogram in LDS and adds it to
 * target[word*KP ..].  target = n_kw (single device: counts updated in place) or n_kw_delta (zeroed; then
 * all-reduced and applied).  If n_k is not NULL the call also folds n_k += n_k_delta; n_k_delta = 0.
 * freq_csc[j] is the frequency of the site logged at j. */
int llda_commit_log(const int64_t *item_begin, const int32_t *item_len, const int32_t *item_word, int64_t n_items,
                    const uint32_t *commit_log, const int32_t *freq_csc, int32_t K, const int64_t *row_off,
                    int32_t *target, int32_t *n_k, int32_t *n_k_delta, void *stream);
/* row_off (dev, may be NULL = row v at target + v*KP): where the row of every word lives in `target`, for the
 * exchange between ranks.  row_off[v] >= 0: KP int32 at target + row_off[v].  row_off[v] < 0: KP/2 int32 at
 * target + ~row_off[v], each holding the counts of positions 2j (low half) and 2j+1 (high half) as int16 PAIRS;
 * counts are added as f * 65536^(p & 1), so words of several ranks can be summed with a plain int32 all-reduce
 * and decoded afterwards -- exact when the frequency mass of the word over ALL ranks and sites is <= 32767 (the
 * caller decides per word from that static bound; hot words stay int32).  Halves the bytes of the all-reduce.
 *
 * llda_apply_rows: counts[r*KP ..] += row r (pairs decoded), row zeroed, for r < n_rows.  With n_rows = V + 1
 * and counts = the fused [n_kw | n_k] buffer, row V is the n_k delta the sweep kernels wrote.  counts 8-byte aligned (the two counts
 * of a pair word are updated with one access; LLDA_E_BAD_ARG otherwise); n_rows == 0 is a no-op. */
int llda_apply_rows(const int64_t *row_off, int32_t *rows, int64_t n_rows, int32_t K, int32_t *counts, void *stream);

/* The 16-bit image of n_kw for llda_sweep_args.n_kw16 (ABI 15; K with llda_rows16_ok).  row16[v] != 0 flags the words whose
 * rows are packed: those whose counts can never leave 0 .. 65535 -- e.g. the words whose total over all topics, which Gibbs
 * sampling conserves, is at most 65535 (the reference's counts, LabeledLDA.py:109-111,123-125, only move a site's frequency
 * between two topics of one word).  Call it once per sweep, after the counts of the previous sweep were folded in and before
 * the first llda_sweep; unflagged rows of n_kw16 are not written.  A flagged row with a count outside the range sets bit 2
 * of status word 0 (status may be NULL: nothing is reported then).  n_kw and n_kw16 16-byte aligned (LLDA_E_BAD_ARG otherwise). */
int llda_pack_rows16(const int32_t *n_kw, const uint8_t *row16, int64_t V, int32_t K, uint16_t *n_kw16, int32_t *status,
                     void *stream);

/* llda_pack_image with the image's columns in an order of the caller's (ABI 20): img[v][c] = min(n_kw[v][col_src[c]], 255 | 65535)
 * for c < KP; col_src (dev, int32[KP], 16-byte aligned) is a permutation of the device positions.  For llda_sweep_args.n_kw_img + img_col.
 * PRECONDITION, not checked on the host (the table lives on the device): col_src is a permutation of 0 .. KP-1 and img_col its inverse.
 * An entry outside 0 .. KP-1 is clamped to KP-1 by the kernels (no out-of-bounds access), a table that is not a permutation gives an
 * image that is not a copy of n_kw: the sweep's results are then undefined (no status bit reports it). */
int llda_pack_image_cols(const int32_t *n_kw, int64_t V, int32_t K, int32_t bits, const int32_t *col_src, void *img, void *stream);

/* The 16-bit image of EVERY row of n_kw plus, per word, whether all counts of its row fit 16 bits in this sweep's n_kw
 * (row16[v] = 1; ABI 19) -- for llda_sweep_args.row16.  K with llda_quad_ok (LLDA_E_BAD_K otherwise); n_kw and n_kw16 16-byte aligned.
 * Call it once per sweep, after the counts of the previous sweep were folded in and before the first llda_sweep.  The image of an
 * unflagged row holds the low halves of its counts and is never read. */
int llda_pack_rows16_all(const int32_t *n_kw, int64_t V, int32_t K, uint16_t *n_kw16, uint8_t *row16, void *stream);

/* The saturating narrow image of n counts for llda_sweep_args.n_kw_img (ABI 18): img[i] = min(n_kw[i], 255) as uint8_t
 * (bits 8) or min(n_kw[i], 65535) as uint16_t (bits 16); a negative count saturates as well.  n = V*KP, a multiple of 4;
 * n_kw 16-byte aligned, img 4-byte (bits 8) / 8-byte (bits 16) aligned -- llda_sweep asks the same of llda_sweep_args.n_kw_img.  Call it once per sweep, after the counts of the previous sweep were folded in and
 * before the first llda_sweep. */
int llda_pack_image(const int32_t *n_kw, int64_t n, int32_t bits, void *img, void *stream);

/* Count initialisation from assignments: LabeledLDA.py:89-92.  n_dk, n_kw, n_k must be zeroed by the
 * caller; z holds device positions.  (The SubLDA phantom-column quirk, CascadeLDA.py:382-385, is a
 * host-side initialisation and is uploaded as data.) */
int llda_count_init(const int64_t *doc_off, const int32_t *word, const int32_t *freq,
                    const int32_t *z, int64_t D, int32_t K,
                    int32_t *n_dk, int32_t *n_kw, int32_t *n_k, void *stream);

/* Counts of counts (ABI 22): hist[n] += the number of ALLOWED entries of a (rows, KP) count matrix in device order that hold the
 * value n.  Minka's fixed point for a symmetric Dirichlet prior depends on n_dk and n_kw only through these histograms
 * (lda_thesis_amd/priors.py); they are exact, independent of order, and summed over ranks with an integer all-reduce.
 * For every row r and every position p < KP whose (lane, slot) bit -- llda_layout.pos_lane / pos_slot -- is set in the row's
 * mask, v = counts[r*KP + p]:  (uint32_t)v < n_bins: hist[v] += 1 (zeros go to hist[0]); otherwise i = (*over_n)++ and
 * over_val[i] = v when i < over_cap (nothing is ever written past over_cap; over_n still counts every such value; the order of
 * over_val is unspecified).  Masked-off entries are not counted whatever they hold, and the masks lane_masks() builds have no bit
 * in the padding.  hist and over_n ACCUMULATE (the caller zeroes them), so a matrix may be passed as several row ranges.
 *   mask_per_row 1: lab_mask is [rows*G], row r uses mask row r (n_dk with llda_sweep_args.lab_mask);
 *   mask_per_row 0: lab_mask is [G], one mask row for every row (n_kw with the all-topics row).
 * rows == 0 is a no-op; n_bins >= 1, over_cap >= 0 (0 with a non-NULL buffer is legal), counts 16-byte aligned.  Every layout is
 * taken (narrow and wide); indices are 64-bit (rows * KP may exceed 2^31). */
int llda_count_hist(const int32_t *counts, int64_t rows, int32_t K, const uint16_t *lab_mask, int32_t mask_per_row,
                    int32_t n_bins, unsigned long long *hist, int32_t *over_val, int64_t over_cap,
                    unsigned long long *over_n, void *stream);

/* log-likelihood read-out (LabeledLDA.py:256-265): out_doc[d] (dev, double[D]) = sum over the sites
 * of document d of  -log( sum_k phi[k][w] * theta[d][k] ),  phi/theta as get_phi/get_theta
 * (LabeledLDA.py:231-239); sites are NOT weighted by frequency (reference quirk).
 * perplexity = exp( sum_d out_doc[d] / S ). */
int llda_loglik(const int64_t *doc_off, const int32_t *word, const uint16_t *lab_mask,
                const int32_t *n_dk, const int32_t *n_kw, const int32_t *n_k,
                int64_t D, int64_t V, int32_t K, double alpha, double beta,
                double *out_doc, void *stream);

/* Thinning read-outs with their running means, on the device (LabeledLDA.py:131-153, 231-239;
 * CascadeLDA.py:394-395, 423-434).  Outputs are in the REFERENCE's layout (row-major (K, V) and (D, K)
 * doubles), not the device permutation, so they can be handed to the caller as they are.
 *
 * llda_readout_phi:   cur[k][v] = (n_kw[v][k] + beta) / den[k]
 *     den == NULL: den[k] = n_k[k] + V*beta           -> get_phi   (LabeledLDA.py:231-234)
 *     den != NULL: double[KP] in device order, beta=0 -> SubLDA.get_ph with den = row sums of n_k_v
 *                                                        (CascadeLDA.py:394-395; 0/0 gives NaN as numpy does)
 * llda_readout_theta: num = n_dk[d] + labs[d]*alpha; cur[d] = num / np.sum(num)   (LabeledLDA.py:236-239;
 *     the row sum in numpy's pairwise order, bit for bit)
 * Both: mode 0: out = cur; mode 1: out = keep*out + share*cur, each product and the sum rounded
 * separately, as `factor*self.ph_hat + (1/s * cur_ph)` (LabeledLDA.py:144-145) and
 * `m * self.ph + (1-m) * cur_ph` (CascadeLDA.py:432) round -- the caller passes the two coefficients.
 * flags (dev int32[1], OR-ed, may be NULL; phi only) report the guards of LabeledLDA.py:146-153 on `out`:
 *   bit 0 an entry < 0, bit 1 a NaN, bit 2 a word whose column is all zero.
 * Padding (positions p < KP with llda_layout.pos_topic[p] < 0): llda_readout_phi uses n_kw, n_k and den at the K positions that
 * hold a topic only -- the padding may hold anything and changes neither out nor flags.  llda_readout_theta (and llda_loglik)
 * sum a row of n_dk over all KP positions: the padding of n_dk must be 0, as every producer of counts leaves it, and lab_mask has
 * no bit there (lane_masks).  Nothing is written outside out[0 .. K*V) / out[0 .. D*K) and flags[0]. */
#define LLDA_READOUT_NEGATIVE 1
#define LLDA_READOUT_NAN      2
#define LLDA_READOUT_NO_LOAD  4
int llda_readout_phi(const int32_t *n_kw, const int32_t *n_k, const double *den, int64_t V, int32_t K,
                     double beta, int32_t mode, double keep, double share, double *out, int32_t *flags,
                     void *stream);
int llda_readout_theta(const int32_t *n_dk, const uint16_t *lab_mask, int64_t D, int32_t K, double alpha,
                       int32_t mode, double keep, double share, double *out, void *stream);

/* Test-time fold-in sampler for held-out documents: one lane group per document, the topic-word
 * loadings are fixed and only the document's n_dk moves.  Covers
 *   LabeledLDA.prep4test + run_test        (LabeledLDA.py:155-212)
 *   CascadeLDA.prep4test + cascade_test    (CascadeLDA.py:186-247)
 *   CascadeLDA.prep4test + run_test        (CascadeLDA.py:299-344)
 * Per document: initial assignments drawn from the rows init_rows[init_idx[site]] (probabilities
 * prepared by the host exactly as the reference's prep4test does; RNG sweep word 0xFFFFFFFF) after
 * `while prob.sum() > 1: prob /= c_init`; then `iters` sweeps of
 *     prob = (n_dk + alpha) * ph[:, v];  prob /= prob.sum();
 *     [beta_fallback: if prob.sum() == 0 (0/0 raises in the reference): prob = (n_dk+alpha)*(ph[:,v]+beta), renormalise]
 *     while prob.sum() > 1: prob /= c_loop;   draw
 * Every `thinning` sweeps n_dk / sum(n_dk) enters a running average (avg_mode 0:
 * (s-1)/s*avg + (1/s)*cur; 1: m*avg + (1-m)*cur, m = (s-1)/s), written to th (D, KP); th = 0 when no sweep
 * reaches a multiple of `thinning`.  z and n_dk (D, KP) receive the final state (iters = 0: the prep4test
 * start state).
 * Order of the topics.  The five matrices ph, init_rows, slot_valid, n_dk and th are LANE-MAJOR: topic k sits at
 *   pos_lane[p] * T + pos_slot[p],  p = topic_pos[k]  (llda_layout)
 * of its row of KP = G * T entries -- NOT at p, the group-layout position the sweep's arrays use; the two orders
 * differ whenever T >= 8 (every K above 32).  Entries that hold no topic (slot_valid = 0) are 0 in ph and init_rows
 * and come back 0 in n_dk and th.  Only z is in group-layout positions: z[site] = topic_pos[topic].
 * The RNG of document d is keyed by the low 32 bits of doc_ids[d] (or of doc_base + d) and by doc_stream[d] (or stream_id).
 * An empty document (doc_off[d] == doc_off[d+1]) gets n_dk = 0 and th = 0 on every path.
 * Refused with LLDA_E_BAD_ARG before anything touches the device: a NULL args, doc_off, word, init_idx, freq, ph,
 * init_rows, slot_valid, z, n_dk or th; D < 0; iters < 0; thinning < 1; c_init or c_loop that is not > 1 (1, less, NaN:
 * the division loops above would not end).  K outside 1 .. LLDA_MAX_K: LLDA_E_BAD_K.  D == 0 is a no-op.
 * alpha < 0 or c_loop - 1 < 1e-9 are legal: every site then takes the exact pipeline, as with exact_only.
 * Domain of the loadings.  ph holds doubles >= 0 of ANY magnitude, init_rows probabilities.  z, n_dk and th are numpy's for every
 * site whose products (n_dk + alpha) * ph[k][v] and whose sum S of them are finite and S > 0 -- from a subnormal S (products that
 * underflow gradually, as numpy's do) up to the overflow threshold: a site with S < 2^-960 is never decided from prefix sums, and
 * outside 2^-500 <= S <= 2^500 the products are multiplied by an exact power of two before they are summed and divided, so the
 * quotients are those of numpy's true division.  What cannot equal numpy: a product or a sum that overflows (inf / inf = NaN in the
 * reference, whose draw raises) and S == 0 without beta_fallback (0 / 0) -- both set bit 0 of status. */
typedef struct llda_foldin_args {
    const int64_t *doc_off;     /* [dev] [D+1]                                                  */
    const int32_t *word;        /* [dev] [S]                                                    */
    const int32_t *init_idx;    /* [dev] [S] row of init_rows for every site                     */
    const int32_t *freq;        /* [dev] [S]                                                    */
    const double  *ph;          /* [dev] [V*KP] loadings, word-major, lane-major rows, 0 in padding */
    const double  *init_rows;   /* [dev] [R*KP] initial probabilities, lane-major rows, 0 in padding */
    const uint8_t *slot_valid;  /* [dev] [KP] lane-major: 1 where an entry holds a topic         */
    int32_t *z;                 /* [dev] [S] out: group-layout positions                         */
    int32_t *n_dk;              /* [dev] [D*KP] out, lane-major rows (n_sites > 0: zeroed by the caller) */
    double  *th;                /* [dev] [D*KP] out, lane-major rows                             */
    int32_t *status;            /* [dev] optional: bit 0 = a site had no positive probability    */
    int64_t D;
    int64_t doc_base;           /* RNG counter word 1 of document 0                              */
    int32_t K, iters, thinning, beta_fallback, avg_mode;
    int32_t exact_only;         /* 0 in production.  Test hook: 1 = every site through the reference's pipeline (numpy-ordered
                                   sum, IEEE divisions, shrink loop, keyed inverse-CDF draw) instead of deciding the draw from
                                   unnormalised prefix sums with a 2^-40 margin where that is provably the same topic */
    double alpha, beta, c_init, c_loop;
    uint64_t seed;
    uint32_t stream_id, reserved2;
    const int64_t *doc_ids;     /* [dev] [D] optional: RNG counter word 1 of every document (its low 32 bits);
                                   NULL = doc_base + d.  Lets documents with unrelated ids share one launch. */
    int64_t n_sites;            /* doc_off[D] (ABI 11).  > 0: the initial assignments are drawn by a separate launch with
                                   one lane group per SITE (they are independent of one another, and the reference's
                                   `while prob.sum() > 1: prob /= c` can run tens of thousands of times for one site);
                                   n_dk must then be zeroed by the caller, doc_off[0] must be 0 and n_sites == doc_off[D].
                                   0: inside the per-document launch, narrow and wide layouts alike; z and n_dk are then pure
                                   outputs (whatever they hold is ignored).  Both give the same z, n_dk and th. */
    const int64_t  *ph_base;    /* [dev] [D] optional (ABI 11): element offset of document d's loadings inside `ph` ...  */
    const uint32_t *doc_stream; /* [dev] [D] optional: ... and its RNG stream id (instead of stream_id): documents that are
                                   sampled against DIFFERENT label subsets of the same size (the nodes of one level of
                                   CascadeLDA.test_down_tree) share one launch                                        */
} llda_foldin_args;

int llda_foldin(const llda_foldin_args *args, void *stream);

/* Rank the label scores of D documents and return the top-n labels plus the per-document ingredients of every metric the
 * reference's harness prints: what LabeledLDA.get_pred / get_preds (/root/reference/LabeledLDA.py:214-229) and one_roc, rates,
 * macro_auc_roc, n_error and get_f1 (/root/reference/evaluate_LabeledLDA.py:8-93) compute on the host, from ONE sort per document
 * (DESIGN.md 4.4b).  Additive to ABI 22.
 *   score [D][ld] doubles, row-major, in REFERENCE topic order (column = topic id), ld >= K the row stride -- not a group layout;
 *   truth [D][K] uint8 or NULL, non-zero = the document carries the label.
 * Only the columns first .. K-1 are ranked (the harness passes 1: 'root' is in no label set); L = K - first.  No other column of
 * score or truth is ever read.  Scores compare as IEEE values (-0 == +0, +-inf ordinary).  Per document:
 *   order    score descending, then topic id ascending: np.argsort(-row, kind="stable")
 *   top_idx  [D][top_n] int32, top_val [D][top_n] double: the first top_n of the order, padded with -1 / 0.0 when L < top_n
 *   n_thr    T, the number of distinct scores (the thresholds of one_roc, highest first: a label is predicted when its score is >=
 *            the threshold; tp_i / fp_i = predicted labels with / without truth, P / N = ranked labels with / without truth)
 *   auc      (double)A / (double)(2 P N),  A = sum_{i=1..T-1} (fp_i - fp_{i-1}) (tp_i + tp_{i-1}): the trapezoid of macro_auc_roc over
 *            (fp / N, tp / P) in exact arithmetic with one rounding (the curve starts at the first threshold, as the reference's);
 *            NaN when P = 0, N = 0 or T < 2
 *   f1       the largest 2 tp_i / (2 tp_i + fp_i + P - tp_i) over the thresholds with tp_i > 0, chosen by integer
 *            cross-multiplication, then one IEEE division (get_f1: its nan thresholds are those with tp = 0); NaN when there is none
 *   hit_rank 1-based rank in the order of the best-ranked true label, 0 when there is none: n_error(n) is the share of documents
 *            with 0 < hit_rank <= n.  (numpy's default argsort in n_error leaves the order of tied scores open; here it is the order above.)
 *   flags    bit 1: P = 0, 2: N = 0, 4: T < 2, 8: every ranked score equals 0 (the documents evaluate_LabeledLDA.py's report drops),
 *            16: a NaN among the ranked scores -- then flags = 16, n_thr = 0, auc = f1 = NaN, hit_rank = 0, top_idx = -1, top_val = 0.
 * Every output pointer may be NULL on its own; with truth == NULL auc, f1 and hit_rank are not written and bits 1 and 2 never set.
 * Every output is an integer or one correctly rounded division of two exact integers: bit-identical whatever the geometry.
 * D == 0 is a no-op; K in 1 .. LLDA_MAX_K (LLDA_E_BAD_K otherwise), 0 <= first < K, ld >= K, 0 <= top_n <= 16. */
typedef struct llda_rank_args {
    const double  *score;        /* [dev] [D][ld]                                                */
    const uint8_t *truth;        /* [dev] [D][K] or NULL                                         */
    int64_t  D;
    int64_t  ld;
    int32_t  K, first, top_n, reserved;
    int32_t *top_idx;            /* [dev] [D][top_n] or NULL                                     */
    double  *top_val;            /* [dev] [D][top_n] or NULL                                     */
    int32_t *n_thr;              /* [dev] [D] or NULL                                            */
    double  *auc;                /* [dev] [D] or NULL                                            */
    double  *f1;                 /* [dev] [D] or NULL                                            */
    int32_t *hit_rank;           /* [dev] [D] or NULL                                            */
    int32_t *flags;              /* [dev] [D] or NULL                                            */
} llda_rank_args;
#define LLDA_RANK_NO_POSITIVE 1
#define LLDA_RANK_NO_NEGATIVE 2
#define LLDA_RANK_ONE_THRESHOLD 4
#define LLDA_RANK_ALL_ZERO 8
#define LLDA_RANK_NAN 16
int llda_rank_labels(const llda_rank_args *args, void *stream);

/* The n best words of every topic from the counts (additive to ABI 22): what topwords_per_topic (LabeledLDA.py:241-254) asks of
 * phi, without phi.  phi[k][v] = (n_kw[v][k] + beta) / den[k] is strictly increasing in the integer count for a fixed topic and two
 * different counts never round to one double (V*beta < 2^40), so the order of a topic's words by phi is their order by count, and
 * equal phi means equal counts.
 *   n_kw [V][KP] int32, word-major, device (group-layout) order, 16-byte aligned; 1 <= V <= 2^31 - 1; every layout is taken.
 *   order    for topic k: n_kw[v][topic_pos[k]] descending, compared as SIGNED int32, then word id ascending --
 *            np.argsort(-get_phi()[k], kind="stable")
 *   top_idx  [K][n] int32 word ids, top_cnt [K][n] int32 their counts, both in REFERENCE topic order; entries i >= min(n, V) are
 *            -1 / 0.  Either may be NULL.
 * Positions of the padding (pos_topic == -1) are never emitted and influence nothing, whatever they hold.  One bandwidth pass over
 * V*KP*4 bytes in row chunks of LLDA_TOPW_CHUNK_ROWS words leaves partial lists in `scratch` (device memory, 8-byte aligned, at
 * least llda_top_words_scratch_bytes(V, K, n) bytes, contents irrelevant before and after), a second small launch merges them per
 * topic.  Everything is an integer: the outputs do not depend on the geometry.
 * LLDA_E_BAD_ARG: a NULL n_kw or scratch, n outside 1 .. 16, V < 1, a misaligned pointer, scratch_bytes too small;
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K; both before anything touches HIP.
 * llda_top_words_scratch_bytes is host only (needs no device) and returns the same codes for the same bad arguments. */
#define LLDA_TOPW_CHUNK_ROWS 256
int64_t llda_top_words_scratch_bytes(int64_t V, int32_t K, int32_t n);
int llda_top_words(const int32_t *n_kw, int64_t V, int32_t K, int32_t n, int32_t *top_idx, int32_t *top_cnt, void *scratch,
                   int64_t scratch_bytes, void *stream);

/* Document and co-document frequencies of listed words (additive to ABI 22): the integers of UMass coherence (Mimno et al. 2011)
 * and of NPMI, over a corpus CSR.
 *   doc_off [D+1] int64, word [S] int32 with ids in [0, V): a site counts whatever its frequency, a word may repeat in a document.
 *            doc_off may point into the middle of a longer array (a document range); its entries index `word` as they are.
 *   memb_off [V+1] int32, memb [M] int32, M = memb_off[V] <= K*n: the entries memb_off[w] .. memb_off[w+1]-1 say which topics list
 *            word w, each as topic*16 + rank with topic in REFERENCE order and rank < n; their order is unspecified, a word may be
 *            listed by several topics (entries with topic >= K or rank >= n are ignored).
 *   co       [K][n][n] unsigned 64-bit.  With R(d, k) = the ranks r for which some site of document d carries a word listed as
 *            (k, r):  co[k][i][j] += 1 for all i >= j in R(d, k), for every document and topic.  The diagonal is the document
 *            frequency; entries with j > i are never written.  co ACCUMULATES (the caller zeroes it), so a corpus may be passed
 *            as several document ranges.  Integer atomics: exact and independent of order and geometry.
 * One wavefront per document.  A call of fewer than LLDA_COOC_AGG_MIN_DOCS documents launches at most LLDA_COOC_MAX_WAVES
 * wavefronts, wavefront i takes the documents i, i + LLDA_COOC_MAX_WAVES, ... in turn (its rank masks are cleared in between) and
 * every set bit and pair is one global atomic.  A larger call counts in LDS per slice of topics and adds every workgroup's counters
 * to co once, when at most eight slices cover K (else it takes the first form); the integers are the same.
 * D == 0 is a no-op.  LLDA_E_BAD_ARG: D < 0, V < 1, n outside 1 .. 16, a NULL or misaligned pointer (D > 0);
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K; both before anything touches HIP. */
#define LLDA_COOC_MAX_WAVES 8192
#define LLDA_COOC_AGG_MIN_DOCS 32768
int llda_word_cooc(const int64_t *doc_off, const int32_t *word, int64_t D, int64_t V, int32_t K, int32_t n,
                   const int32_t *memb_off, const int32_t *memb, unsigned long long *co, void *stream);

/* Sliding-window co-occurrence of listed words (additive to ABI 22): the integers of C_V, C_UCI and C_NPMI (Roeder, Both and
 * Hinneburg, WSDM 2015), over documents given as token sequences in reading order.
 *   tok_off [D+1] int64, tok [S] int32: the tokens of document d are tok[tok_off[d]] .. tok[tok_off[d+1]-1].  An id outside [0, V)
 *            (-1) is a position without a dictionary word: it matches nothing and keeps its place in the window.  tok_off may point
 *            into the middle of a longer array; a document holds fewer than 2^32 tokens.
 *   memb_off, memb, co [K][n][n]: as in llda_word_cooc; a word's entries name every (topic, rank) at most once.
 *   window   s, 0 <= s <= LLDA_WINDOW_MAX.  A document of L tokens has no window (L = 0), one window, the whole document (s = 0
 *            or L <= s), or the L - s + 1 windows [w, w + s), w = 0 .. L - s.
 *   For every window and topic k, with R = the ranks r for which some position of the window carries the word listed as (k, r):
 *   co[k][i][j] += 1 for all i >= j in R.  co ACCUMULATES; entries with j > i are never written.  s = 0 gives what llda_word_cooc
 *   gives on the same arrays; with s = 1 the diagonal is the token frequency of every listed word and the rest stays 0.
 * One wavefront walks a document's windows and adds run lengths: a topic's pairs receive, in one add each, the number of
 * consecutive windows over which its set R did not change.  Wavefront i takes the documents i, i + LLDA_WINDOW_MAX_WAVES, ... in a
 * call of fewer than LLDA_WINDOW_AGG_MIN_DOCS documents, and every add is a 64-bit global atomic; a larger call adds to 64-bit LDS
 * counters per slice of topics first and to co once per workgroup, when at most eight slices cover K.  Per-wavefront state is kept
 * per slice of topics as well, so every K and n is taken.  All adds are integers: the result is independent of the form, the
 * geometry and the order.
 * D == 0 is a no-op.  LLDA_E_BAD_ARG: D < 0, V < 1, n outside 1 .. 16, window outside 0 .. LLDA_WINDOW_MAX, a NULL or misaligned
 * pointer (D > 0); LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K; both before anything touches HIP. */
#define LLDA_WINDOW_MAX 65535
#define LLDA_WINDOW_MAX_WAVES 8192
#define LLDA_WINDOW_AGG_MIN_DOCS 32768
int llda_window_cooc(const int64_t *tok_off, const int32_t *tok, int64_t D, int64_t V, int32_t K, int32_t n, int32_t window,
                     const int32_t *memb_off, const int32_t *memb, unsigned long long *co, void *stream);

/* Per-document likelihood of held-out sites (additive to ABI 22): the scored half of document completion.
 *   doc_off [D+1] int64, word [S] int32, freq [S] int32 or NULL (= all 1; 0 <= f < 2^23): the sites to score, a CSR;
 *   theta [D][ld_theta] doubles, phi_t [V][ld_phi] doubles, word-major; both row-major in REFERENCE topic order (column = topic id,
 *   not a group layout), ld_* >= K the row strides.  Columns >= K are never read.
 * A value is a pair (m, e), m in [0.5, 1), meaning m * 2^e; 1.0 is (0.5, 1).  mul((a, ea), (b, eb)): c = a*b; c < 0.5: c = 2c and the
 * exponent drops by one; result (c, ea + eb [- 1]).  Every operation is one IEEE float64 operation, rounded on its own.
 *   site     64 partial sums part[j] = sum_{i = 0, 1, ...; j + 64i < K} theta[d][j+64i] * phi_t[w][j+64i], each product rounded, added
 *            in increasing i from +0.0; then for s = 1, 2, 4, 8, 16, 32: part[j] = part[j] + part[j xor s] for every j at once;
 *            p = part[0].  (m, e) = frexp(p); p^f by right-to-left binary exponentiation: acc = (0.5, 1), base = (m, e); for every
 *            bit of f from the lowest: bit set: acc = mul(acc, base); then base = mul(base, base).
 *   document start from (0.5, 1) and mul the sites' p^f in ascending site index; tok += f.  A site whose p is not a finite positive
 *            number (or whose word id is outside [0, V): it is never used as an index) is left out of the product and of tok and
 *            adds f to bad.
 *   mant [D] double, expo [D] int64: the document's likelihood mant * 2^expo; tok [D] int64, bad [D] int64.  Each may be NULL.
 * The host takes the logarithm: log(mant) + expo * ln 2.  A document's outputs depend on its own inputs only -- not on D, its place
 * in the batch or the geometry -- and equal the restatement in tests/heldoutref.py bit for bit.
 * One wavefront per document for K > 32 (theta in registers up to K = 1024, re-read beyond), a group of 8, 16 or 32 >= K lanes for
 * K <= 32 (zero partials add exactly: the same bits).  D == 0 is a no-op.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: D < 0, V outside 1 .. 2^31 - 1, ld < K, a NULL doc_off, word, theta or
 * phi_t (D > 0), a misaligned pointer.  Both before anything touches HIP. */
typedef struct llda_heldout_args {
    const int64_t *doc_off;      /* [dev] [D+1]                                                  */
    const int32_t *word;         /* [dev] [S]                                                    */
    const int32_t *freq;         /* [dev] [S] or NULL                                            */
    const double  *theta;        /* [dev] [D][ld_theta]                                          */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    int64_t  D, V, ld_theta, ld_phi;
    int32_t  K, reserved;
    double  *mant;               /* [dev] [D] or NULL                                            */
    int64_t *expo;               /* [dev] [D] or NULL                                            */
    int64_t *tok;                /* [dev] [D] or NULL                                            */
    int64_t *bad;                /* [dev] [D] or NULL                                            */
} llda_heldout_args;
#define LLDA_HELDOUT_MAX_FREQ 8388607
int llda_heldout_loglik(const llda_heldout_args *args, void *stream);

/* Credit attribution and the deterministic EM fold-in (additive to ABI 22): the E-step of the document model.
 * With theta fixed (iters = 0) it says which share of every word belongs to which label; iterated with the matching M-step it is a
 * fold-in without random numbers.
 *   doc_off [D+1] int64, word [S] int32, freq [S] int32 or NULL (= all 1; 0 <= f < 2^23): the sites, a CSR;
 *   theta [D][ld_theta] doubles: the start loads; phi_t [V][ld_phi] doubles, word-major; both row-major in REFERENCE topic order,
 *   ld_* >= K the row strides.  Columns >= K are never read.  iters >= 0 EM steps; alpha >= 0 is read only when iters > 0.
 * Every operation is one IEEE float64 operation, rounded on its own.  sum64(x): 64 partial sums part[j] = x[j] + x[j+64] + ... in
 * increasing index from +0.0; then for s = 1, 2, 4, 8, 16, 32: part[j] = part[j] + part[j xor s] for every j at once; the sum is
 * part[0] (the rule of llda_heldout_loglik).
 *   site (w, f)  t[k] = theta[k] * phi_t[w][k];  p = sum64(t).  The site is GOOD when w is in [0, V) and LLDA_ATTR_MIN_P <= p < inf
 *            (below 2^-960, 1/p or f/p can overflow, and 0 * inf would poison labels the document does not have).  A site that is
 *            not good adds f to bad and nothing else (a word id outside [0, V) is never used as an index).  A good site adds f to
 *            tok; inv = 1.0 / p (the one division per site); g = (double)f * inv; credit[k] = credit[k] + t[k] * g for every k.
 *            The sites are added in ascending order, credit from +0.0.
 *   step     (iters times, for a document with at least one site; a document without sites keeps its loads)
 *            num[k] = theta[k] > 0.0 ? credit[k] + alpha : 0.0;  den = sum64(num);  0 < den < inf: theta[k] = num[k] / den for every
 *            k, else theta stays.  Then credit, tok and bad are computed again from zero against the new loads.  A label whose load
 *            is 0 stays 0: that is how a label set is expressed (a uniform row means "any label").
 *   after the last step: credit is the credit against the final loads.  For a good site r[k] = t[k] * inv; the labels with
 *            r[k] > 0, ordered by r[k] descending (the rounded r, not t), then topic id ascending; the first top_m of them go to
 *            site_idx / site_val, padded with -1 / 0.0.  A site that is not good gets all -1 / 0.0.
 *   theta_out [D][ld_out] doubles: the loads after iters steps (iters = 0: the bits of theta);  credit [D][ld_credit] doubles;
 *   site_idx [S][top_m] int32 and site_val [S][top_m] double (top_m in 0 .. 4);  tok [D], bad [D] int64.  Each may be NULL on its
 *   own; with top_m > 0 site_idx and site_val are given or left out together.  Columns >= K of the outputs are not written.
 * A document's outputs depend on its own inputs only -- not on D, its place in the batch or the geometry -- and equal the
 * restatement in tests/attrref.py bit for bit.  An empty document gets theta_out = theta, credit = 0, tok = bad = 0.
 * One wavefront per document for K > 32 (theta and credit in registers up to K = 1024, in LDS beyond: 16 K bytes, one wavefront
 * per workgroup), a group of 8, 16 or 32 >= K lanes for K <= 32.  All steps of a document run inside one launch.  The whole row of
 * phi_t is read even where theta is 0.  D == 0 is a no-op.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args; D < 0; V outside 1 .. 2^31 - 1; an ld < K; iters < 0; alpha
 * negative or NaN; top_m outside 0 .. 4; top_m > 0 with exactly one of site_idx / site_val NULL; a NULL doc_off, word, theta or
 * phi_t (D > 0); a misaligned pointer.  All before anything touches HIP. */
typedef struct llda_attr_args {
    const int64_t *doc_off;      /* [dev] [D+1]                                                  */
    const int32_t *word;         /* [dev] [S]                                                    */
    const int32_t *freq;         /* [dev] [S] or NULL                                            */
    const double  *theta;        /* [dev] [D][ld_theta]                                          */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    int64_t  D, V, ld_theta, ld_phi, ld_out, ld_credit;
    int32_t  K, iters, top_m, reserved;
    double   alpha;
    double  *theta_out;          /* [dev] [D][ld_out] or NULL                                    */
    double  *credit;             /* [dev] [D][ld_credit] or NULL                                 */
    int32_t *site_idx;           /* [dev] [S][top_m] or NULL                                     */
    double  *site_val;           /* [dev] [S][top_m] or NULL                                     */
    int64_t *tok;                /* [dev] [D] or NULL                                            */
    int64_t *bad;                /* [dev] [D] or NULL                                            */
} llda_attr_args;
#define LLDA_ATTR_MIN_P 0x1p-960
#define LLDA_ATTR_MAX_TOP 4
int llda_attribute(const llda_attr_args *args, void *stream);

/* Left-to-right estimate of a document's likelihood p(w_d | phi, alpha) (additive to ABI 22): Wallach, Murray, Salakhutdinov and
 * Mimno, "Evaluation methods for topic models" (ICML 2009), Algorithm 3, with R particles per document.
 *   doc_off [D+1] int64, word [S] int32: TOKENS, one entry per occurrence, in the caller's order;
 *   phi_t [V][ld_phi] doubles, word-major, REFERENCE topic order, ld_phi >= K.  Columns >= K are never read;
 *   allowed [D][ld_allowed] uint8 or NULL: non-zero = document d may use topic k (NULL: every topic); A = how many it may use;
 *   doc_ids [D] int64 or NULL (= doc_base + d): the document's id, whose low 32 bits key its random numbers.
 * Every operation is one IEEE float64 operation, rounded on its own.  Topic k belongs to lane k mod 64, slot k / 64.
 *   x(c, w)      x[k] = ((double)c[k] + alpha) * phi_t[w][k] for the allowed k, +0.0 for the others.
 *   draw64(x, u) lane j owns x[j + 64 i]; q[j][i] = the lane's sequential inclusive prefix over i; X = the Hillis-Steele inclusive
 *                scan of the lane totals (d = 1, 2, .., 32: X[j] = X[j-d] + X[j] for j >= d); t = u * X[63]; t_j = t - X[j-1],
 *                X[-1] = 0; the draw is the first (j, i), lanes first, with x > 0 and q[j][i] > t_j, else the last (j, i) with x > 0,
 *                else NONE.  The weights are not normalised (no division); a topic whose weight is 0 is never drawn.
 *   sum64(x)     64 partials part[j] = x[j] + x[j+64] + ... in increasing k from +0.0; then part[j] = part[j] + part[j xor s] for
 *                s = 1, 2, 4, 8, 16, 32, every j at once; the sum is part[0] (the rule of llda_heldout_loglik).
 *   u(n, r, m)   the keyed uniform of the Philox4x32-10 counter (m >> 1, low 32 bits of the document id, stream_id + r mod 2^32, n)
 *                under the key seed: words (0, 1) = (a, b) for an even m, words (2, 3) for an odd m,
 *                u = ((a >> 5) * 2^26 + (b >> 6)) / 2^53.
 *   document     particle r = 0 .. R-1 holds the counts c_r[k] = 0 and the assignments z_r[n] = NONE.  For the position
 *                n = 0, 1, .., N-1 with the word w_n, every particle:
 *                  resampling   for m = 0 .. n-1 in order, skipping the m with z_r[m] = NONE:  c_r[z_r[m]] -= 1;
 *                               z = draw64(x(c_r, w_m), u(n, r, m)); z_r[m] = z (kept as it was when z is NONE); c_r[z_r[m]] += 1.
 *                  prediction   x = x(c_r, w_n); S_r = sum64(x); pred_r = S_r / ((double)assigned_r + A_alpha), assigned_r = the
 *                               number of m < n with z_r[m] != NONE, A_alpha = (double)A * alpha (rounded before the sum).
 *                  extension    0 < S_r < inf: z_r[n] = draw64(x, u(n, r, n)) and, unless it is NONE, c_r[z_r[n]] += 1.
 *                               Otherwise z_r[n] stays NONE.
 *                A word outside [0, V) is never used as an index: the resampling runs all the same, S_r and pred_r are NaN and
 *                z_r[n] stays NONE.
 *                p_n = (pred_0 + pred_1 + ... + pred_{R-1}) / (double)R, added in increasing r from +0.0.  0 < p_n < inf: tok += 1
 *                and the document's pair is multiplied by frexp(p_n) -- mul of llda_heldout_loglik, from (0.5, 1); else bad += 1.
 *   mant [D] double, expo [D] int64, tok [D] int64, bad [D] int64: as llda_heldout_loglik's (all four required);
 *   status [1] int32 or NULL: bit 0 is OR-ed in when a document holds more than max_doc_tokens tokens.  Such a document is not
 *   scored: its outputs are (0.5, 1, 0, 0).  So are those of an empty document, without the bit.
 * A document's outputs depend on its own tokens, its id, its allowed row and the scalars -- not on D, its place in the batch or the
 * geometry -- and equal the restatement in tests/leftrightref.py bit for bit.  Cost: R * N * (N + 1) / 2 draws over K topics.
 * One workgroup per document, one wavefront per particle (counts in registers, assignments and words in LDS sized by
 * max_doc_tokens: pass the longest document, not the limit).  D == 0 is a no-op.
 * LLDA_E_BAD_K: K outside 1 .. 1024 (the counts of a particle stay in registers: a narrow-layout entry point).  LLDA_E_BAD_ARG: a
 * NULL args or a struct_bytes other than sizeof(llda_leftright_args); D < 0; V outside 1 .. 2^31 - 1; ld_phi < K, or ld_allowed < K
 * with allowed; R outside 1 .. LLDA_LR_MAX_PARTICLES; alpha not a finite number > 0; max_doc_tokens outside 1 .. LLDA_LR_MAX_TOKENS
 * (the estimator is quadratic in N); with D > 0 a NULL doc_off, word, phi_t, mant, expo, tok or bad, or a misaligned pointer.  All
 * before anything touches HIP.  llda_leftright_struct_bytes (host only) lets a binding check its definition at load time. */
#define LLDA_LR_MAX_PARTICLES 16
#define LLDA_LR_MAX_TOKENS 4096
typedef struct llda_leftright_args {
    uint32_t struct_bytes;       /* sizeof(llda_leftright_args)                                  */
    int32_t  K, R, max_doc_tokens;
    const int64_t *doc_off;      /* [dev] [D+1]                                                  */
    const int32_t *word;         /* [dev] [S]                                                    */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    const uint8_t *allowed;      /* [dev] [D][ld_allowed] or NULL                                */
    const int64_t *doc_ids;      /* [dev] [D] or NULL                                            */
    int64_t  D, V, ld_phi, ld_allowed, doc_base;
    double   alpha;
    uint64_t seed;
    uint32_t stream_id, reserved;
    double  *mant;               /* [dev] [D]                                                    */
    int64_t *expo;               /* [dev] [D]                                                    */
    int64_t *tok;                /* [dev] [D]                                                    */
    int64_t *bad;                /* [dev] [D]                                                    */
    int32_t *status;             /* [dev] [1] or NULL                                            */
} llda_leftright_args;
int llda_leftright_struct_bytes(void);
int llda_left_to_right(const llda_leftright_args *args, void *stream);

/* The n best rows of a matrix b for every row of a matrix a under a bilinear score (additive to ABI 22): similar
 * documents (rows = sqrt(theta): the score is the Bhattacharyya coefficient, Hellinger distance = sqrt(1 - score)), similar labels
 * (rows = sqrt(phi), L = V), nearest-neighbour prediction.
 *   a [Q][lda], b [D][ldb] doubles, row-major; lda, ldb >= L; columns >= L are never read.  L in 1 .. 2^31 - 1 (not bound by
 *   LLDA_MAX_K); n in 1 .. LLDA_NEAREST_MAX_N; row_base >= 0 = the global id of row 0 of b (row_base + D must fit an int64);
 *   exclude [Q] int64 or NULL: a global row id that query q must not return (-1, or any id outside the range: none).
 * Score of the pair (q, j): s = +0.0, then for k = 0, 1, .., L-1 in this order s = fma(a[q][k], b[j][k], s) -- one fused multiply-add,
 * one rounding per element.  It depends on the two rows only: not on Q, D, the tiles, `chunks` or which call holds the row.
 * Order per query: score descending, compared as IEEE values (-0 == +0, +-inf ordinary), then global row id ascending.  A NaN score is
 * not a candidate (it is counted), and neither is the exclude row.
 *   top_idx [Q][n] int64 global row ids, top_val [Q][n] double, n_nan [Q] int64 = the NaN scores left out; each may be NULL.
 *   Entries beyond the number of candidates are -1 / 0.0.
 *   chunks: 0 = the library chooses; > 0 = b is walked as exactly min(chunks, D) row ranges.  A geometry knob: no output depends on it.
 *   scratch: at least llda_nearest_scratch_bytes(Q, D, n, chunks) bytes, contents irrelevant before and after.  One partial list per
 *   (query, range) is left there and a second small launch merges them; no score is written to memory.
 * Alignment: every pointer 8-byte aligned, and that is all the kernel needs (odd lda / ldb included).  When a and b are both 16-byte
 * aligned and lda and ldb are both even, the rows are fetched with 16-byte loads (the fast path); the results are the same bits.
 * Q == 0 is a no-op; D == 0 launches only the padding.  LLDA_E_BAD_ARG, before anything touches HIP: a NULL args, a struct_bytes
 * other than sizeof(llda_nearest_args), a NULL a, b or scratch; n outside 1 .. 16; L < 1; lda or ldb < L; negative Q, D, chunks or
 * row_base; sizes whose products leave an int64 or a grid of 2^31 - 1 workgroups; a misaligned pointer; scratch_bytes too small.
 * llda_nearest_scratch_bytes and llda_nearest_struct_bytes are host only; the former returns LLDA_E_BAD_ARG for the same bad sizes. */
#define LLDA_NEAREST_MAX_N 16
#define LLDA_NEAREST_TILE 128    /* queries and rows of a tile */
#define LLDA_NEAREST_KSTEP 16    /* columns per step of the k-loop */
typedef struct llda_nearest_args {
    uint32_t struct_bytes;       /* sizeof(llda_nearest_args)                                    */
    int32_t  L, n, chunks;
    const double  *a;            /* [dev] [Q][lda]                                               */
    const double  *b;            /* [dev] [D][ldb]                                               */
    const int64_t *exclude;      /* [dev] [Q] or NULL                                            */
    int64_t  Q, D, lda, ldb, row_base;
    int64_t *top_idx;            /* [dev] [Q][n] or NULL                                         */
    double  *top_val;            /* [dev] [Q][n] or NULL                                         */
    int64_t *n_nan;              /* [dev] [Q] or NULL                                            */
    void    *scratch;            /* [dev]                                                        */
    int64_t  scratch_bytes;
} llda_nearest_args;
int llda_nearest_struct_bytes(void);
int64_t llda_nearest_scratch_bytes(int64_t Q, int64_t D, int32_t n, int32_t chunks);
int llda_nearest_rows(const llda_nearest_args *args, void *stream);

/* Label-wise evaluation (additive to ABI 22): for every ranked label the D documents ordered by that label's score,
 * and from the ordered row the label's AUC, its best F1 and the threshold that reaches it (SCut).  llda_rank_labels ranks the K labels
 * of a document; this is the other sort: D keys for each of n_labels segments, 64-bit keys, the document id as payload.
 *   score [D][ld] doubles in REFERENCE topic order, ld >= K; truth [D][K] uint8, REQUIRED here, non-zero = the document carries the label.
 * The ranked columns are first .. first + n_labels - 1 <= K - 1; output row l belongs to column first + l, and no other column is read:
 * a caller short of scratch walks the labels in batches and gets the same bits.  1 <= D <= 2^30 (the payload doc << 1 | truth keeps
 * 32 bits and every product below 64); D == 0 or n_labels == 0 is a no-op.  Scores compare as IEEE values (-0 == +0, +-inf ordinary).
 * Per ranked label:
 *   order    [n_labels][D] int32: the document ids by score descending, then document id ascending: np.argsort(-col, kind="stable")
 *   A tie group is a maximal run of equal scores in the order; its end is a threshold: a document is predicted when its score is >=
 *   the group's.  tp_g / fp_g = predicted documents with / without the label, cumulative; tp_0 = fp_0 = 0.
 *   n_pos    P, documents with the label (N = D - P);  n_thr  T, the number of distinct scores; both int64
 *   auc_num  uint64 A = sum_{g=1..T} (fp_g - fp_{g-1}) (tp_g + tp_{g-1}) = 2 #(positive above negative) + #(positive tied with negative),
 *            the Mann-Whitney count; A <= 2 P N < 2^61
 *   auc      (double)A / (double)(2 P N), one IEEE division; NaN when P = 0 or N = 0.  The curve starts at (0, 0): the standard
 *            label-wise AUC.  This is deliberately NOT llda_rank_labels's per-document auc, which starts at the first threshold as the
 *            reference's macro_auc_roc does; that quirk stays where the reference has it.  (T = 1 with P, N > 0 gives 0.5 here.)
 *   f1       the largest 2 tp_g / (tp_g + fp_g + P) over the groups with tp_g > 0, chosen by integer cross-multiplication; equal
 *            rationals go to the highest threshold (the earliest group); then one IEEE division.  thr_tp, thr_fp (int64) are that
 *            group's tp_g and fp_g, thr (double) the score BITS of the group's first document in the order (its lowest document id:
 *            a -0.0 stays one).  No group with tp > 0 (P = 0): f1 = thr = NaN, thr_tp = thr_fp = 0.
 *   flags    int32, the bits of llda_rank_labels: 1: P = 0, 2: N = 0, 4: T < 2, 8: every score of the column equals 0,
 *            16: a NaN in the column -- then flags = 16, the five integers are 0, auc = f1 = thr = NaN and the order row is -1.
 * Every output pointer may be NULL on its own.  Every output is an integer, a copy of an input or one correctly rounded division of
 * two exact integers: bit-identical whatever the chunk, the batches or the geometry.
 *   chunk    0 = LLDA_LABEL_CHUNK pairs are sorted by one workgroup in LDS before the merge levels; 256 = the one other value, for tests
 *            (a deep merge tree at a few thousand documents).  Anything else: LLDA_E_BAD_ARG.
 *   scratch  at least llda_label_scratch_bytes(D, n_labels, chunk) bytes = 2 x 12 x Dp x n_labels + 16, Dp = D rounded up to the chunk;
 *            contents irrelevant before and after.  (D = 100 000, 511 labels: 1.26 GB.)
 * Alignment: score, scratch and the 8-byte outputs 8-byte aligned, flags and order 4-byte aligned.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG, before anything touches HIP: a NULL args; a struct_bytes other than
 * sizeof(llda_label_args); first < 0, n_labels < 0 or first + n_labels > K; ld < K; D < 0 or D > 2^30; a chunk other than 0 and 256;
 * and with D > 0 and n_labels > 0: a NULL score, truth or scratch, a misaligned pointer, scratch_bytes too small.
 * llda_label_scratch_bytes and llda_label_struct_bytes are host only; the former returns LLDA_E_BAD_ARG for the same bad sizes. */
#define LLDA_LABEL_CHUNK 4096        /* pairs one workgroup sorts in LDS: 48 KB, three workgroups per compute unit */
#define LLDA_LABEL_TEST_CHUNK 256
#define LLDA_LABEL_MAX_D (1 << 30)
typedef struct llda_label_args {
    uint32_t struct_bytes;       /* sizeof(llda_label_args)                                      */
    int32_t  K, first, n_labels;
    int32_t  chunk, reserved;
    const double  *score;        /* [dev] [D][ld]                                                */
    const uint8_t *truth;        /* [dev] [D][K]                                                 */
    int64_t  D, ld;
    int64_t  *n_pos;             /* [dev] [n_labels] or NULL                                     */
    int64_t  *n_thr;             /* [dev] [n_labels] or NULL                                     */
    uint64_t *auc_num;           /* [dev] [n_labels] or NULL                                     */
    double   *auc;               /* [dev] [n_labels] or NULL                                     */
    int64_t  *thr_tp;            /* [dev] [n_labels] or NULL                                     */
    int64_t  *thr_fp;            /* [dev] [n_labels] or NULL                                     */
    double   *f1;                /* [dev] [n_labels] or NULL                                     */
    double   *thr;               /* [dev] [n_labels] or NULL                                     */
    int32_t  *flags;             /* [dev] [n_labels] or NULL                                     */
    int32_t  *order;             /* [dev] [n_labels][D] or NULL                                  */
    void     *scratch;           /* [dev]                                                        */
    int64_t  scratch_bytes;
} llda_label_args;
int llda_label_struct_bytes(void);
int64_t llda_label_scratch_bytes(int64_t D, int32_t n_labels, int32_t chunk);
int llda_label_metrics(const llda_label_args *args, void *stream);

/* Label SETS from per-label thresholds (additive to ABI 22): document d predicts label k when score[d][k] >= thr[k],
 * an IEEE compare (so a NaN threshold means "never", and -0 >= +0).
 *   score [D][ld] doubles, ld >= K; thr [K] doubles; truth [D][K] uint8 or NULL; columns below `first` are never predicted, never
 *   counted and, like the padding bits of a mask row, always 0.  A column first .. K-1 whose thr is not a NaN is ELIGIBLE.
 *   mask    [D][W] uint32, W = (K + 31) / 32: bit k & 31 of word k >> 5 = label k is predicted
 *   n_pred  [D] int32: the number of predicted labels
 *   at_least_one = 1: a document whose mask would be empty predicts its best eligible label: the first by (score descending as IEEE
 *           values, topic id ascending) -- the order of llda_rank_labels.  That bit counts as predicted in every output.  (No eligible
 *           column: the mask stays empty.)
 *   A document with a NaN score in an eligible column predicts nothing, with or without at_least_one, and gets n_pred = -1.
 *   With truth: n_hit [D] int32 = predicted and true, n_true [D] int32 = true labels among first .. K-1, and tp, fp, fn [K] int64:
 *   the documents that predict and carry / predict and do not carry / carry and do not predict label k.  tp, fp and fn are ADDED to
 *   (integer atomics: the sums do not depend on the order): THE CALLER ZEROES THEM, and may accumulate several calls.
 * Every output pointer may be NULL on its own; without truth n_hit, n_true, tp, fp and fn are not written.  D == 0 is a no-op.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG, before anything touches HIP: a NULL args; a struct_bytes other than
 * sizeof(llda_sets_args); first outside 0 .. K; ld < K; D < 0 or D x ld beyond an int64; at_least_one other than 0 and 1; and with
 * D > 0: a NULL score or thr, a misaligned pointer (8 bytes: score, thr, tp, fp, fn; 4: mask, n_pred, n_hit, n_true). */
typedef struct llda_sets_args {
    uint32_t struct_bytes;       /* sizeof(llda_sets_args)                                       */
    int32_t  K, first, at_least_one;
    const double  *score;        /* [dev] [D][ld]                                                */
    const double  *thr;          /* [dev] [K]                                                    */
    const uint8_t *truth;        /* [dev] [D][K] or NULL                                         */
    int64_t  D, ld;
    uint32_t *mask;              /* [dev] [D][(K + 31) / 32] or NULL                             */
    int32_t  *n_pred;            /* [dev] [D] or NULL                                            */
    int32_t  *n_hit;             /* [dev] [D] or NULL                                            */
    int32_t  *n_true;            /* [dev] [D] or NULL                                            */
    int64_t  *tp;                /* [dev] [K] or NULL, added to                                  */
    int64_t  *fp;                /* [dev] [K] or NULL, added to                                  */
    int64_t  *fn;                /* [dev] [K] or NULL, added to                                  */
} llda_sets_args;
int llda_sets_struct_bytes(void);
int llda_label_sets(const llda_sets_args *args, void *stream);

/* The n best words of every topic by a float64 SCORE (additive to ABI 22): the distinctive words of a label --
 * relevance (Sievert and Shirley 2014), lift -- and the ranking of a float64 matrix such as the running mean ph_hat.
 *   score[w][k] = P_a(x[w][k]) / wdiv[w]
 *   power    P_a(x) = x for a = 1, else ((x * x) * x) ...: a - 1 multiplications, left to right, each rounded, never contracted;
 *            1 <= a <= 8.
 *   divisor  wdiv [V] doubles or NULL (= every wdiv[w] is 1.0, nothing is divided).  The division is ONE IEEE division.
 *            A word with wdiv[w] == 0 (either sign) is not ranked for any topic.
 *   NaN      a NaN score is skipped and counted in n_nan[k].
 *   order    score descending, compared as IEEE values (-0 == +0, +-inf ordinary), then word id ascending:
 *            np.argsort(-score[cand, k], kind="stable") over the candidate words in id order.
 *   x        two sources; exactly one of n_kw and mat is non-NULL:
 *     counts   n_kw [V][KP] int32, word-major, device (group-layout) order, 16-byte aligned -- what llda_top_words takes.
 *              x = ((double)c + beta) / den[k], the count converted as signed int32; den [KP] doubles in device order, or NULL:
 *              den[k] = (double)n_k[k] + (double)V * beta with n_k [KP] int32 -- exactly llda_readout_phi, so x has the bits of
 *              get_phi()[k][w].  Positions of the padding (pos_topic == -1) of n_kw, n_k and den influence nothing, whatever they
 *              hold.  The conversion, the add and the division happen in the pass: it reads V*KP*4 bytes once, and wdiv.
 *     matrix   mat [V][ld] doubles, ld >= K, columns in REFERENCE topic order, 8-byte aligned; x is the entry.
 *   outputs  in REFERENCE topic order, each may be NULL on its own: top_idx [K][n] int32 word ids; top_score [K][n] doubles, the
 *            bits as computed (a -0.0 stays one); n_nan [K] int32.  Entries beyond the number of ranked words of a topic are -1 and
 *            the quiet NaN 0x7ff8000000000000.
 * With lam = s / t the order of relevance lam * log(phi) + (1 - lam) * log(phi / p) within a topic is the order of
 * phi^t / p^(t - s): a = t and wdiv = P_(t-s)(p); lam = 1 is phi itself (a = 1, no wdiv), lam = 0 is lift (a = 1, wdiv = p).
 * Every output is a copy of an input, a count, or the result of the stated IEEE operations on one element: the result does not
 * depend on chunking or geometry.  The key of a list entry is 96 bits, (score, word).  One bandwidth pass over the source in row
 * chunks of LLDA_TOPW_CHUNK_ROWS words leaves partial lists in `scratch` (device memory, 8-byte aligned, at least
 * llda_scored_words_scratch_bytes(V, K, n) bytes -- enough for either source --, contents irrelevant before and after); a second
 * small launch merges them per topic.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG, before anything touches HIP: a NULL args; a struct_bytes other than
 * sizeof(llda_scored_args); both of n_kw and mat, or neither; n outside 1 .. 16; a outside 1 .. 8; V < 1 or V > 2^31 - 1; ld < K
 * or V x ld beyond an int64 (matrix); neither n_k nor den (counts); a NULL or too small scratch; a misaligned pointer (16 bytes:
 * n_kw; 8: den, mat, wdiv, top_score, scratch; 4: n_k, top_idx, n_nan).
 * llda_scored_struct_bytes and llda_scored_words_scratch_bytes are host only; the latter returns the same codes for a bad V, K, n. */
typedef struct llda_scored_args {
    uint32_t struct_bytes;       /* sizeof(llda_scored_args)                                     */
    int32_t  K, n, a;
    const int32_t *n_kw;         /* [dev] counts: [V][KP], else NULL                             */
    const int32_t *n_k;          /* [dev] counts: [KP] or NULL (then den)                        */
    const double  *den;          /* [dev] counts: [KP] or NULL (then n_k)                        */
    const double  *mat;          /* [dev] matrix: [V][ld], else NULL                             */
    const double  *wdiv;         /* [dev] [V] or NULL                                            */
    int64_t  V, ld;              /* ld: matrix only                                              */
    double   beta;               /* counts only                                                  */
    int32_t *top_idx;            /* [dev] [K][n] or NULL                                         */
    double  *top_score;          /* [dev] [K][n] or NULL                                         */
    int32_t *n_nan;              /* [dev] [K] or NULL                                            */
    void    *scratch;            /* [dev] work space                                             */
    int64_t  scratch_bytes;
} llda_scored_args;
int llda_scored_struct_bytes(void);
int64_t llda_scored_words_scratch_bytes(int64_t V, int32_t K, int32_t n);
int llda_scored_words(const llda_scored_args *args, void *stream);

/* ECDF ranks of every word within every topic (additive to ABI 22): the integers FREX (Bischof and Airoldi 2012)
 * and topic exclusivity are made of.  llda_scored_words ranks one float score; a rank-based score needs every topic's whole
 * empirical distribution over the vocabulary: a sort of V keys per topic, done by the engine of llda_label_metrics.
 *   mat [V][ld] doubles, word-major, columns in REFERENCE topic order, ld >= K; columns >= K are never read.
 *   tot[w]   sum64(mat[w][0 .. K-1]) -- the fixed-order sum of llda_heldout_loglik (64 partials from +0.0, then the xor tree) -- over
 *            ALL K columns, whatever the ranked range.
 *   cand [V] uint8 or NULL (= every word).  A word is a CANDIDATE iff cand[w] != 0 and 0 < tot[w] < inf, in both modes: the same set
 *            for every column, and every entry of a candidate's row is finite.  Vc, the number of candidates, goes to n_cand[0].
 *   value    mode 0: v[w][k] = mat[w][k];  mode 1: v[w][k] = mat[w][k] / tot[w], ONE IEEE division: the exclusivity.
 *   rank     [n_labels][V] int32, row l for column first + l <= K - 1 (no other column is ranked: a caller short of scratch walks the
 *            columns in batches and gets the same bits).  For a candidate #{candidates u : v[u][k] <= v[w][k]}, compared as IEEE
 *            values (-0 == +0): the column's ECDF times Vc, np.searchsorted(np.sort(v[cand, k]), v[w, k], side="right"), in 1 .. Vc;
 *            equal values share the rank of the group's last member.  For any other word 0.
 *   value    [n_labels][V] doubles or NULL: the bits of v (a -0.0 stays one); any other word gets the quiet NaN 0x7ff8000000000000.
 * 1 <= V <= 2^30 (the payload word << 1 keeps 32 bits); n_labels == 0 is a no-op that writes nothing, not even n_cand.
 * Every output is an integer or the result of one stated IEEE operation on one element: bit-identical whatever the chunk, the batches
 * or the geometry.
 *   chunk    as in llda_label_args: 0, or 256 for tests.
 *   scratch  at least llda_ecdf_scratch_bytes(V, n_labels, chunk) bytes = 2 x 12 x Vp x n_labels + 8 x V + 16, Vp = V rounded up to
 *            the chunk; contents irrelevant before and after.
 * Alignment: mat, value, n_cand and scratch 8-byte aligned, rank 4-byte aligned.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG, before anything touches HIP: a NULL args; a struct_bytes other than
 * sizeof(llda_ecdf_args); first < 0, n_labels < 0 or first + n_labels > K; ld < K; V < 1 or V > 2^30; a chunk other than 0 and 256; a
 * mode other than 0 and 1; and with n_labels > 0: a NULL mat, rank or scratch, V x ld beyond an int64, a misaligned pointer,
 * scratch_bytes too small.
 * llda_ecdf_scratch_bytes and llda_ecdf_struct_bytes are host only; the former returns LLDA_E_BAD_ARG for the same bad sizes. */
#define LLDA_ECDF_MAX_V (1 << 30)
typedef struct llda_ecdf_args {
    uint32_t struct_bytes;       /* sizeof(llda_ecdf_args)                                       */
    int32_t  K, first, n_labels;
    int32_t  chunk, mode;
    const double  *mat;          /* [dev] [V][ld]                                                */
    const uint8_t *cand;         /* [dev] [V] or NULL                                            */
    int64_t  V, ld;
    int32_t  *rank;              /* [dev] [n_labels][V]                                          */
    double   *value;             /* [dev] [n_labels][V] or NULL                                  */
    int64_t  *n_cand;            /* [dev] [1] or NULL                                            */
    void     *scratch;           /* [dev]                                                        */
    int64_t  scratch_bytes;
} llda_ecdf_args;
int llda_ecdf_struct_bytes(void);
int64_t llda_ecdf_scratch_bytes(int64_t V, int32_t n_labels, int32_t chunk);
int llda_ecdf_ranks(const llda_ecdf_args *args, void *stream);

/* The n best words of every topic by TWO ranks (additive to ABI 22): FREX, the harmonic mean of a word's frequency
 * rank and its exclusivity rank within the topic,  FREX = 1 / (omega / F_e + (1 - omega) / F_f),  F = rank / Vc,  omega = s / t.
 *   rank_f, rank_e [n_labels][V] int32: what llda_ecdf_ranks wrote in mode 0 and mode 1 -- or any numbers in 0 .. Vc.  A word is
 *            RANKED in column l iff both of its ranks are in 1 .. Vc (anything else counts as 0: not ranked).
 *   cost     c = s / re + (t - s) / rf = A / B with the integers A = s rf + (t - s) re <= 2^36 and B = re rf <= 2^60; FREX = t / (Vc c).
 *   order    c ascending -- FREX descending --, compared EXACTLY: A B' against A' B as 96-bit integer products, never through a
 *            floating-point number (two costs at ranks near 2^30 differ by less than a double resolves); equal costs by word id
 *            ascending.  sorted((Fraction(A, B), w)) over the ranked words.
 *   weight   0 <= s <= t, 1 <= t <= LLDA_FREX_MAX_T: s = 0 orders by rf alone, s = t by re alone.
 *   outputs  top_idx, top_rank_f, top_rank_e [n_labels][n] int32: the word ids and their two ranks; entries beyond the number of
 *            ranked words are -1 / 0 / 0.  1 <= n <= LLDA_FREX_MAX_N.
 *   probe    [n_labels][m] int32 word ids or NULL, 0 <= m <= LLDA_FREX_MAX_N: probe_rank_f, probe_rank_e [n_labels][m] get the two
 *            ranks of those words in that column; a probe outside 0 .. V-1 (-1: no word) or a word that is not ranked gives 0 / 0.
 * Every output pointer may be NULL on its own.  All outputs are copies of inputs chosen by integer comparisons: bit-identical whatever
 * the geometry.  The double a caller reports is computed on the host, (double)t * (double)B / ((double)Vc * (double)A), each step
 * rounded; it is a report, never the key.
 * One coalesced pass along the rank rows in chunks of LLDA_FREX_CHUNK words leaves partial lists in `scratch` (at least
 * llda_frex_scratch_bytes(V, n_labels, n) = 12 x n x ceil(V / LLDA_FREX_CHUNK) x n_labels + 16 bytes, 8-byte aligned, contents
 * irrelevant before and after); a second small launch merges them per column.  n_labels == 0 is a no-op.
 * LLDA_E_BAD_ARG, before anything touches HIP: a NULL args; a struct_bytes other than sizeof(llda_frex_args); n_labels < 0 or
 * > LLDA_MAX_K; V or Vc outside 1 .. 2^30; t outside 1 .. 64 or s outside 0 .. t; n outside 1 .. 16; m outside 0 .. 16; and with
 * n_labels > 0: a NULL rank_f, rank_e or scratch, a misaligned pointer (8 bytes: scratch; 4: every other), scratch_bytes too small.
 * llda_frex_scratch_bytes and llda_frex_struct_bytes are host only; the former returns LLDA_E_BAD_ARG for the same bad sizes. */
#define LLDA_FREX_MAX_N 16
#define LLDA_FREX_MAX_T 64
#define LLDA_FREX_CHUNK 16384
typedef struct llda_frex_args {
    uint32_t struct_bytes;       /* sizeof(llda_frex_args)                                       */
    int32_t  n_labels, n, m;
    int32_t  s, t;
    const int32_t *rank_f;       /* [dev] [n_labels][V]                                          */
    const int32_t *rank_e;       /* [dev] [n_labels][V]                                          */
    const int32_t *probe;        /* [dev] [n_labels][m] or NULL                                  */
    int64_t  V, Vc;
    int32_t *top_idx;            /* [dev] [n_labels][n] or NULL                                  */
    int32_t *top_rank_f;         /* [dev] [n_labels][n] or NULL                                  */
    int32_t *top_rank_e;         /* [dev] [n_labels][n] or NULL                                  */
    int32_t *probe_rank_f;       /* [dev] [n_labels][m] or NULL                                  */
    int32_t *probe_rank_e;       /* [dev] [n_labels][m] or NULL                                  */
    void    *scratch;            /* [dev] work space                                             */
    int64_t  scratch_bytes;
} llda_frex_args;
int llda_frex_struct_bytes(void);
int64_t llda_frex_scratch_bytes(int64_t V, int32_t n_labels, int32_t n);
int llda_frex_select(const llda_frex_args *args, void *stream);

/* EM training, the word side (additive to ABI 22): llda_attribute's E-step adds a site's label shares to its DOCUMENT; this adds
 * the same shares to its WORD.  credit_w[v][k] is the expected n_kw of the corpus under (theta, phi_t); with llda_phi_step below it
 * is the other half of an EM fit of Labeled LDA without random numbers.
 *   word_off [V+1] int64, site_doc [S] int32, freq [S] int32 or NULL (= all 1; 0 <= f < 2^23): the sites in WORD-major order, a
 *   CSR over the words: the sites of word v are word_off[v] .. word_off[v+1], site_doc their documents.  S = word_off[V], the
 *   caller states it (0 <= S <= LLDA_WCREDIT_MAX_SITES); offsets outside [0, S] are not used as addresses;
 *   theta [D][ld_theta] and phi_t [V][ld_phi] doubles, REFERENCE topic order, ld_* >= K.  Columns >= K are never read;
 *   chunk >= 1: how many consecutive sites of a word are added up by one wavefront.
 * A site (d, f) of word v, in the arithmetic of llda_attribute (every operation one IEEE float64 operation, rounded on its own;
 * sum64 as defined there):  ok = d in [0, D) (a document id outside is never used as an index);  t[k] = theta[d][k] * phi_t[v][k];
 * p = sum64(t).  The site is GOOD when it is ok and LLDA_ATTR_MIN_P <= p < inf.  A site that is not good adds f to bad[v] and
 * nothing else.  A good site adds f to tok[v]; inv = 1.0 / p; g = (double)f * inv; acc[k] = acc[k] + t[k] * g.  (Multiplication
 * commutes: t, p, inv and g carry the bits they have in llda_attribute.)
 * The order of the sum: the sites of word v are cut into chunks of `chunk` consecutive sites, the last may be shorter.  A chunk is
 * added in ascending site order from +0.0; credit_w[v][k] is the chunk sums added in ascending chunk order from +0.0.  A word
 * without sites gets a row of +0.0 and tok = bad = 0.
 *   credit_w [V][ld_credit] doubles, tok [V], bad [V] int64: each may be NULL.  Columns >= K of credit_w are not written.
 * A word's outputs depend on its own sites, its own row of phi_t, the rows of theta they name and chunk -- not on V, the word's
 * place in the batch, the grid or the kernel form -- and equal the restatement in tests/emref.py bit for bit.  No floating-point
 * atomics: one wavefront (for K <= 32 a group of 8, 16 or 32 lanes) per chunk, phi_t's row in registers up to K = 1024 and read
 * through its pointer beyond, with the sums in LDS; the only chunk of a word stores straight to the outputs, the chunks of a longer
 * word store partial rows to the scratch, which a second pass adds.  A wavefront finds its chunk in a table (the word of every chunk,
 * next to a prefix sum of the words' chunk counts) that a first one-workgroup pass leaves in the scratch.
 *   scratch: llda_credit_words_scratch_bytes(V, S, K, chunk) bytes = 16 (V + 1) + 2 floor(S / chunk) (8 K + 16) + 4 C rounded up to
 *   a multiple of 8 + 16, C = min(S, floor(S / chunk) + V) the chunks at most.
 * S == 0 still writes the zero rows and needs no input and no scratch; with every output NULL nothing is launched.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args or a struct_bytes that is not the struct's; D < 0; V outside
 * 1 .. 2^31 - 1; S outside 0 .. LLDA_WCREDIT_MAX_SITES; an ld < K; chunk < 1; with S > 0 a NULL word_off, site_doc, phi_t or
 * scratch, a NULL theta (D > 0), or scratch_bytes below the query; a misaligned pointer.  All before anything touches HIP. */
#define LLDA_WCREDIT_MAX_SITES (1LL << 40)
typedef struct llda_wcredit_args {
    uint32_t struct_bytes;       /* sizeof(llda_wcredit_args)                                    */
    int32_t  K, chunk, reserved;
    const int64_t *word_off;     /* [dev] [V+1]                                                  */
    const int32_t *site_doc;     /* [dev] [S]                                                    */
    const int32_t *freq;         /* [dev] [S] or NULL                                            */
    const double  *theta;        /* [dev] [D][ld_theta]                                          */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    int64_t  D, V, S, ld_theta, ld_phi, ld_credit;
    double  *credit_w;           /* [dev] [V][ld_credit] or NULL                                 */
    int64_t *tok;                /* [dev] [V] or NULL                                            */
    int64_t *bad;                /* [dev] [V] or NULL                                            */
    void    *scratch;            /* [dev] work space                                             */
    int64_t  scratch_bytes;
} llda_wcredit_args;
int llda_wcredit_struct_bytes(void);
int64_t llda_credit_words_scratch_bytes(int64_t V, int64_t S, int32_t K, int32_t chunk);
int llda_credit_words(const llda_wcredit_args *args, void *stream);

/* EM training, the phi M-step (additive to ABI 22): the shape of the reference's get_phi, (n + b) / (n_k + V b), on expected counts.
 *   cw [V][ld] doubles: the word credit (non-negative, finite); beta > 0, finite.
 *   colsum[k]: the rows are cut into blocks of LLDA_COLSUM_ROWS consecutive words; a block is added in ascending word order from
 *   +0.0, the block sums in ascending block order from +0.0.  Vb = (double)V * beta, rounded once; den[k] = colsum[k] + Vb;
 *   phi_t_out[v][k] = (cw[v][k] + beta) / den[k].  Every operation one IEEE float64 operation; tests/emref.py restates it.
 *   phi_t_out [V][ld_out] doubles: may be cw itself with ld_out = ld (an entry is read and written by one thread, after the sums);
 *   den [K] doubles or NULL.  Columns >= K are neither read nor written.
 *   scratch: llda_phi_step_scratch_bytes(V, K) bytes = (ceil(V / 256) + 1) 8 K + 16, the block sums and den.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args or a wrong struct_bytes; V outside 1 .. 2^31 - 1; an ld < K;
 * beta not a finite number > 0; a NULL cw, phi_t_out or scratch; scratch_bytes below the query; a misaligned pointer.  All before
 * anything touches HIP. */
#define LLDA_COLSUM_ROWS 256
typedef struct llda_phistep_args {
    uint32_t struct_bytes;       /* sizeof(llda_phistep_args)                                    */
    int32_t  K;
    const double *cw;            /* [dev] [V][ld]                                                */
    double  *phi_t_out;          /* [dev] [V][ld_out]                                            */
    double  *den;                /* [dev] [K] or NULL                                            */
    int64_t  V, ld, ld_out;
    double   beta;
    void    *scratch;            /* [dev] work space                                             */
    int64_t  scratch_bytes;
} llda_phistep_args;
int llda_phistep_struct_bytes(void);
int64_t llda_phi_step_scratch_bytes(int64_t V, int32_t K);
int llda_phi_step(const llda_phistep_args *args, void *stream);

/* The document model on sparse label sets (additive to ABI 22): llda_attribute and llda_credit_words for documents that carry a
 * handful of the K labels.  A site gathers L_d entries of its word's row of phi_t where the dense entry points read K.
 *   lab_off [D+1] int64, lab [NL] int32: the label sets, a CSR next to the sites: the labels of document d are
 *   lab[lab_off[d]] .. lab[lab_off[d+1] - 1], strictly ascending, in [0, K).  L_d = lab_off[d+1] - lab_off[d].  NL = lab_off[D], the
 *   caller states it.  lab_off must not descend (two documents never share a slot);
 *   theta_s [NL] doubles: the loads, one per SLOT of lab; theta_out [NL] and credit [NL] live per slot too;
 *   max_labels in 1 .. LLDA_SPARSE_MAX_LABELS: the longest list of the call.  The lane group is the smallest of 8, 16, 32 that is
 *   >= max_labels, one value per call.
 * A document is UNFIT when L_d > max_labels, when its offsets do not lie in [0, NL], when a label id is outside [0, K) or when its
 * list is not strictly ascending (the kernel compares every id with its left neighbour's inside the group).  The label ids of an
 * unfit document are never used as an index.  A document with L_d = 0 is fit: every site has p = 0.
 * Arithmetic: that of llda_attribute word for word (every operation one IEEE float64 operation, rounded on its own; sum64,
 * LLDA_ATTR_MIN_P, one division per site, g = (double)f * inv, num / den and the theta > 0 rule, ties by topic id) on the
 * one-document problem with K' = L_d, theta' = the document's slots and phi_t'[w][j] = phi_t[w][lab[j]]:
 *   site (w, f)  t[j] = theta_s[j] * phi_t[w][lab[j]];  p = sum64(t), over the L_d products in slot order.
 * With the prefix 0 .. L_d - 1 as every label set and dense rows that are 0 elsewhere both entry points below give the bits of the
 * dense entry points at full K (adding +0.0 to a sum that is never -0.0 is the identity).  For other label sets the two forms
 * differ in the last bits of p: the dense sum64 pairs the products by topic id mod 64, this one by slot.
 *
 * llda_attribute_sparse: the fields of llda_attr_args with the label sets in place of theta and the row strides.
 *   A fit document with L_d >= 1 gets, bit for bit, what llda_attribute gives on its one-document problem: theta_out, credit (per
 *   slot), tok, bad, site_val of its sites, and site_idx with lab[j] where that problem has j.  A fit document with L_d = 0 writes
 *   no slot; all its sites are bad.  An unfit document: every site adds f to bad, tok = 0, site_idx / site_val all -1 / 0.0; its
 *   slots of theta_out keep theta_s and those of credit get +0.0 (offsets outside [0, NL]: no slot is written).
 *   A document's outputs depend on its own inputs and on nothing else; tests/sparseref.py restates them.  D == 0 is a no-op.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args or a struct_bytes that is not the struct's; D < 0; V outside
 * 1 .. 2^31 - 1; NL < 0; ld_phi < K; max_labels outside 1 .. LLDA_SPARSE_MAX_LABELS; iters < 0; alpha negative or NaN; top_m
 * outside 0 .. 4; top_m > 0 with exactly one of site_idx / site_val NULL; with D > 0 a NULL doc_off, word, lab_off or phi_t, or
 * (NL > 0) a NULL lab or theta_s; a misaligned pointer.  All before anything touches HIP. */
#define LLDA_SPARSE_MAX_LABELS 32
typedef struct llda_attr_sparse_args {
    uint32_t struct_bytes;       /* sizeof(llda_attr_sparse_args)                                */
    int32_t  K, max_labels, iters, top_m, reserved;
    const int64_t *doc_off;      /* [dev] [D+1]                                                  */
    const int32_t *word;         /* [dev] [S]                                                    */
    const int32_t *freq;         /* [dev] [S] or NULL                                            */
    const int64_t *lab_off;      /* [dev] [D+1]                                                  */
    const int32_t *lab;          /* [dev] [NL]                                                   */
    const double  *theta_s;      /* [dev] [NL]                                                   */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    int64_t  D, V, NL, ld_phi;
    double   alpha;
    double  *theta_out;          /* [dev] [NL] or NULL                                           */
    double  *credit;             /* [dev] [NL] or NULL                                           */
    int32_t *site_idx;           /* [dev] [S][top_m] or NULL                                     */
    double  *site_val;           /* [dev] [S][top_m] or NULL                                     */
    int64_t *tok;                /* [dev] [D] or NULL                                            */
    int64_t *bad;                /* [dev] [D] or NULL                                            */
} llda_attr_sparse_args;
int llda_attr_sparse_struct_bytes(void);
int llda_attribute_sparse(const llda_attr_sparse_args *args, void *stream);

/* llda_credit_words_sparse: llda_wcredit_args with the label sets in place of theta.  A site (d, f) of word v is OK when d is in
 * [0, D) and document d is fit; then t[j] = theta_s[j] * phi_t[v][lab[j]] over the slots of d, p = sum64(t), and the site is GOOD
 * when LLDA_ATTR_MIN_P <= p < inf.  A site that is not good adds f to bad[v] and nothing else.  A good site adds f to tok[v];
 * inv = 1.0 / p; g = (double)f * inv; acc[lab[j]] = acc[lab[j]] + t[j] * g for its slots.
 * The order of the sum is llda_credit_words': chunks of `chunk` consecutive sites of the word, a chunk added in ascending site
 * order from +0.0, the chunk sums in ascending chunk order from +0.0.  credit_w is the same dense [V][ld_credit] rows; a column
 * that no good site of the word reaches is +0.0.
 * One wavefront per chunk (llda_credit_words' index and combine passes as they are), the chunk's K sums in LDS: 8 K bytes per
 * wavefront, at most 61 504.  64 / G sites are worked at a time and commit to LDS one after the other in ascending site order.
 * No floating-point atomics.  A word's outputs depend on its own sites, its row of phi_t, the label sets they name and chunk;
 * tests/sparseref.py restates them.  scratch: llda_credit_words_sparse_scratch_bytes(V, S, K, chunk), the formula of
 * llda_credit_words_scratch_bytes.  S == 0 still writes the zero rows; with every output NULL nothing is launched.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args or a struct_bytes that is not the struct's; D < 0; V outside
 * 1 .. 2^31 - 1; S outside 0 .. LLDA_WCREDIT_MAX_SITES; NL < 0; ld_phi < K or ld_credit < K; chunk < 1; max_labels outside
 * 1 .. LLDA_SPARSE_MAX_LABELS; with S > 0 a NULL word_off, site_doc, phi_t or scratch, a NULL lab_off (D > 0), a NULL lab or
 * theta_s (NL > 0), or scratch_bytes below the query; a misaligned pointer.  All before anything touches HIP. */
typedef struct llda_wcredit_sparse_args {
    uint32_t struct_bytes;       /* sizeof(llda_wcredit_sparse_args)                             */
    int32_t  K, chunk, max_labels;
    const int64_t *word_off;     /* [dev] [V+1]                                                  */
    const int32_t *site_doc;     /* [dev] [S]                                                    */
    const int32_t *freq;         /* [dev] [S] or NULL                                            */
    const int64_t *lab_off;      /* [dev] [D+1]                                                  */
    const int32_t *lab;          /* [dev] [NL]                                                   */
    const double  *theta_s;      /* [dev] [NL]                                                   */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    int64_t  D, V, S, NL, ld_phi, ld_credit;
    double  *credit_w;           /* [dev] [V][ld_credit] or NULL                                 */
    int64_t *tok;                /* [dev] [V] or NULL                                            */
    int64_t *bad;                /* [dev] [V] or NULL                                            */
    void    *scratch;            /* [dev] work space                                             */
    int64_t  scratch_bytes;
} llda_wcredit_sparse_args;
int llda_wcredit_sparse_struct_bytes(void);
int64_t llda_credit_words_sparse_scratch_bytes(int64_t V, int64_t S, int32_t K, int32_t chunk);
int llda_credit_words_sparse(const llda_wcredit_sparse_args *args, void *stream);

/* llda_heldout_loglik_sparse (additive to ABI 22): llda_heldout_args with the label sets (lab_off, lab, theta_s,
 * NL, max_labels as above) in place of theta and ld_theta.
 * Arithmetic: llda_heldout_loglik's word for word on the document's compacted problem, K' = L_d, theta' = the document's slots,
 * phi_t'[w][j] = phi_t[w][lab[j]]:
 *   site (w, f)  p = sum64 of the L_d products theta_s[j] * phi_t[w][lab[j]] in slot order; then frexp(p), p^f by right-to-left
 *                binary exponentiation, the document's pair product and the good / bad rule of llda_heldout_loglik, unchanged.
 * A fit document with L_d = 0 has p = 0 at every site: all its sites are bad.  An UNFIT document: every site adds f to bad, tok = 0,
 * the pair stays (0.5, 1), and none of its label ids is used as an index.  mant, expo, tok, bad [D]: each may be NULL.
 * With the prefix 0 .. L_d - 1 as every label set it gives the bits of llda_heldout_loglik on the scattered theta (+0.0 elsewhere);
 * for other sets the two differ in the last bits of p (sum64 pairs by slot here, by topic id mod 64 there).
 * G = the smallest of 8, 16, 32 >= max_labels lanes per document, 64 / G documents per wavefront; a site gathers L_d doubles.
 * A document's outputs depend on its own inputs only; tests/sparseheldref.py restates them.  D == 0 is a no-op.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args or a struct_bytes that is not the struct's; D < 0; V outside
 * 1 .. 2^31 - 1; NL < 0; ld_phi < K; max_labels outside 1 .. LLDA_SPARSE_MAX_LABELS; with D > 0 a NULL doc_off, word, lab_off or
 * phi_t, or (NL > 0) a NULL lab or theta_s; a misaligned pointer.  All before anything touches HIP. */
typedef struct llda_heldout_sparse_args {
    uint32_t struct_bytes;       /* sizeof(llda_heldout_sparse_args)                             */
    int32_t  K, max_labels, reserved;
    const int64_t *doc_off;      /* [dev] [D+1]                                                  */
    const int32_t *word;         /* [dev] [S]                                                    */
    const int32_t *freq;         /* [dev] [S] or NULL                                            */
    const int64_t *lab_off;      /* [dev] [D+1]                                                  */
    const int32_t *lab;          /* [dev] [NL]                                                   */
    const double  *theta_s;      /* [dev] [NL]                                                   */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    int64_t  D, V, NL, ld_phi;
    double  *mant;               /* [dev] [D] or NULL                                            */
    int64_t *expo;               /* [dev] [D] or NULL                                            */
    int64_t *tok;                /* [dev] [D] or NULL                                            */
    int64_t *bad;                /* [dev] [D] or NULL                                            */
} llda_heldout_sparse_args;
int llda_heldout_sparse_struct_bytes(void);
int llda_heldout_loglik_sparse(const llda_heldout_sparse_args *args, void *stream);

/* llda_left_to_right_sparse (additive to ABI 22): llda_leftright_args with the label sets (lab_off, lab, NL,
 * max_labels as above; no loads) in place of allowed and ld_allowed, for every K in 1 .. LLDA_MAX_K: the label-conditioned document
 * likelihood p(w_d | labels_d) at the cost of L_d gathered doubles per draw, whatever K is.
 * Arithmetic: the text of llda_left_to_right on the document's compacted problem -- K' = L_d, phi_t'[w][j] = phi_t[w][lab[j]],
 * every topic allowed, A = L_d -- with the same doc_ids, stream_id + r, seed and u(n, r, m).  Compacted topic j sits in lane j,
 * slot 0, so draw64 and sum64 are those of K' <= 32 <= 64 topics.  The kernel works them on the G = 8, 16 or 32 >= max_labels lanes
 * of a group, which gives the same bits: the lanes >= L_d hold +0.0 and x is never -0.0, so (i) the Hillis-Steele steps d >= G
 * leave the prefixes of the lanes < G as they are, and X[63] = X[G-1] + (a sum of +0.0s) = X[G-1]; (ii) the steps s >= G of sum64's
 * tree add +0.0.  The assignment a position holds is the SLOT j.  With the prefix 0 .. L_d - 1 as the label set the outputs are
 * also those of llda_left_to_right at full K with the prefix as the allowed row (K <= 1024).
 * An UNFIT document: every token is bad, tok = 0, the pair stays (0.5, 1) and no label id is used as an index.  L_d = 0 (fit):
 * A = 0, every pred is NaN, every token is bad.  max_doc_tokens and status bit 0 as in llda_left_to_right (such a document gets
 * (0.5, 1, 0, 0)).  mant, expo, tok, bad are required.
 * One workgroup per document; particle r is the lane group r of the workgroup (64 / G particles per wavefront, ceil(R G / 64)
 * wavefronts); one count per lane; the words (32 bits) and the assignments (8 bits per particle) in LDS, sized by max_doc_tokens.
 * A document's outputs depend on its own tokens, its id, its label list and the scalars only; tests/sparseheldref.py restates them.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args or a struct_bytes that is not the struct's; D < 0; V outside
 * 1 .. 2^31 - 1; NL < 0; ld_phi < K; max_labels outside 1 .. LLDA_SPARSE_MAX_LABELS; R outside 1 .. LLDA_LR_MAX_PARTICLES; alpha
 * not a finite number > 0; max_doc_tokens outside 1 .. LLDA_LR_MAX_TOKENS; with D > 0 a NULL doc_off, word, lab_off, phi_t, mant,
 * expo, tok or bad, or (NL > 0) a NULL lab; a misaligned pointer.  All before anything touches HIP. */
typedef struct llda_leftright_sparse_args {
    uint32_t struct_bytes;       /* sizeof(llda_leftright_sparse_args)                           */
    int32_t  K, R, max_doc_tokens;
    const int64_t *doc_off;      /* [dev] [D+1]                                                  */
    const int32_t *word;         /* [dev] [S]                                                    */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    const int64_t *lab_off;      /* [dev] [D+1]                                                  */
    const int32_t *lab;          /* [dev] [NL]                                                   */
    const int64_t *doc_ids;      /* [dev] [D] or NULL                                            */
    int64_t  D, V, ld_phi, NL, doc_base;
    double   alpha;
    uint64_t seed;
    uint32_t stream_id;
    int32_t  max_labels;
    double  *mant;               /* [dev] [D]                                                    */
    int64_t *expo;               /* [dev] [D]                                                    */
    int64_t *tok;                /* [dev] [D]                                                    */
    int64_t *bad;                /* [dev] [D]                                                    */
    int32_t *status;             /* [dev] [1] or NULL                                            */
} llda_leftright_sparse_args;
int llda_leftright_sparse_struct_bytes(void);
int llda_left_to_right_sparse(const llda_leftright_sparse_args *args, void *stream);

/* llda_foldin_sparse (additive to ABI 22): the test-time sampler of llda_foldin for documents that carry a handful of
 * the K labels, for every K in 1 .. LLDA_MAX_K.  The label sets are lab_off, lab, NL, max_labels as above (no loads); phi_t is the
 * word-major matrix in reference topic order that the document model reads, not llda_foldin's lane-major ph.  A site costs L_d
 * gathered doubles per sweep, whatever K is.
 * Arithmetic: the text of llda_foldin (beta_fallback = 0, avg_mode = 0, beta = 0) on the document's compacted problem -- K' = L_d,
 * ph'[j][v] = phi_t[v][lab[j]], in the layout of K' topics: one numpy leaf, compacted topic j in lane j & 7, slot j >> 3.
 *   sum      numpy's order for L_d contiguous doubles: sequential for L_d < 8, else L_d / 8 rows on eight chains, the xor butterfly
 *            1, 2, 4, then the L_d % 8 tail in order.
 *   draw     the keyed draw on that layout with u(seed; sweep, stream_id, doc, n), doc = doc_ids[d] or doc_base + d (low 32 bits).
 *   start    sweep word 0xFFFFFFFF.  Every column ph'[:, v] is divided by its own sum over the L_d labels; a document that holds a
 *            column which cannot be normalised (sum 0, or a quotient that is not finite) starts every site from the uniform row
 *            1 / L_d.  Then `while sum > 1: prob /= c_init`, draw.
 *   sweep i  prob = (n_dk + alpha) * ph'[:, v]; S = sum; prob /= S; `while sum > 1: prob /= c_loop`; draw.  Every site takes this
 *            pipeline (no decided tier); the quotients are IEEE divisions over the whole range of doubles.
 *   average  after every sweep i with (i + 1) % thinning == 0: cur = n_dk / n_dk.sum(), avg = cur for the first, else
 *            (s-1)/s * avg + (1/s) * cur with s = (i + 1) / thinning, each product rounded on its own.  th_s = 0 when there is none.
 * Outputs: z [S] the SLOT j of the document's list (not a topic id); n_dk_s, th_s [NL] per slot.
 * An UNFIT document (offsets outside [0, NL], L_d > max_labels, an id outside [0, K), ids that do not ascend strictly): z = -1 at all
 * its sites, nothing else of it is written, none of its ids is used as an index; status bit 2.  A site whose word is outside [0, V):
 * z = -1, it adds nothing to the counts, is never used as an index and keeps its site number n; status bit 1.  A site with no
 * positive probability (every site of a fit document with L_d = 0 among them): status bit 0, the document's other outputs are then
 * unspecified.  A document without sites: n_dk_s = 0, th_s = 0.  D == 0: nothing to do.
 * 8 lanes per document, 1, 2 or 4 slots per lane by max_labels; a document's outputs depend on its own sites, its id, its label list
 * and the scalars only, not on D or its place in the batch; tests/sparsefoldinref.py restates them.
 * LLDA_E_BAD_K: K outside 1 .. LLDA_MAX_K.  LLDA_E_BAD_ARG: NULL args or a struct_bytes that is not the struct's; D < 0; V outside
 * 1 .. 2^31 - 1; NL < 0; ld_phi < K; max_labels outside 1 .. LLDA_SPARSE_MAX_LABELS; iters < 0; thinning < 1; c_init or c_loop not
 * > 1; alpha NaN; with D > 0 a NULL doc_off, word, freq, lab_off, phi_t or z, or (NL > 0) a NULL lab, n_dk_s or th_s; a misaligned
 * pointer.  All before anything touches HIP. */
typedef struct llda_foldin_sparse_args {
    uint32_t struct_bytes;       /* sizeof(llda_foldin_sparse_args)                              */
    int32_t  K, max_labels, iters, thinning;
    uint32_t stream_id;
    const int64_t *doc_off;      /* [dev] [D+1]                                                  */
    const int32_t *word;         /* [dev] [S]                                                    */
    const int32_t *freq;         /* [dev] [S]                                                    */
    const double  *phi_t;        /* [dev] [V][ld_phi]                                            */
    const int64_t *lab_off;      /* [dev] [D+1]                                                  */
    const int32_t *lab;          /* [dev] [NL]                                                   */
    const int64_t *doc_ids;      /* [dev] [D] or NULL                                            */
    int64_t  D, V, NL, ld_phi, doc_base;
    double   alpha, c_init, c_loop;
    uint64_t seed;
    int32_t *z;                  /* [dev] [S]  out: the slot of every site, -1 = none            */
    int32_t *n_dk_s;             /* [dev] [NL] out                                               */
    double  *th_s;               /* [dev] [NL] out                                               */
    int32_t *status;             /* [dev] [1] or NULL                                            */
} llda_foldin_sparse_args;
int llda_foldin_sparse_struct_bytes(void);
int llda_foldin_sparse(const llda_foldin_sparse_args *args, void *stream);

/* Device self test of the kernel's division shortcut: runs >= n random (a, b) pairs through
 * "q = a * RN(1/b) + two exact-residual corrections" and through the hardware IEEE division and adds
 * the number of differing results to *mismatches_dev (dev, uint64, zeroed by the caller).  Expected: 0. */
int llda_selftest_div(uint64_t seed, int64_t n, unsigned long long *mismatches_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LLDA_GIBBS_H */
