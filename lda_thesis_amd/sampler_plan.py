"""Which arrays ``GibbsSampler`` hands to the library: the Python half of the kernel-selection policy (the other half, what
``llda_sweep`` launches for the arrays it is handed, is csrc/sweep_plan.hpp).

Host only and pure: plain Python scalars in, a small named record out -- or the ``ValueError`` of a request that cannot be met.  No
torch, no numpy, no library call; the environment is read in ``options`` and nowhere else.  A fact that costs a device reduction or
a synchronisation and is needed on some paths only (the longest document, the wide-row site share, "does any row fit 16 bits", the
sampled escape rates) is passed as a zero-argument callable and called only on those paths.  The thresholds are arguments whose
defaults are the constants below; ``GibbsSampler`` binds its class attributes of the same names to them and passes ``self.X``.

Later facts depend on earlier allocations, so the constructor calls the stages in order -- ``options``, ``commit_log``,
``shard_is_dense``, ``scratch``, ``rows_possible`` / ``rows``, ``image_bits``, ``image_order_possible`` / ``image_order_taken`` --
and collects the verdicts in one ``SamplerPlan`` on ``sampler.plan``.  None of the choices changes a result: the state after a
sweep is bit-identical whichever kernel ran, so only tests/test_sampler_plan_host.py can see a rule that an edit broke.
"""
import collections
import os

ROWS16_MIN_BYTES = 64 << 20      # rows16=None, documents of 2^16 tokens or more (three waves per SIMD): below this n_kw
                                 # the L2s serve the int32 rows and the shorter kernel wins
QUAD_MAX_WIDE_SITES = 0.02       # quad=None: largest share of the sites that may read a row which does not fit the 16-bit image
QUAD_CHECK_EVERY = 32            # ... looked at every so many sweeps (asynchronously)
IMAGE_MIN_BYTES = 32 << 20       # image=None: below this n_kw (the eight L2s hold it) or below IMAGE_MIN_SITES sites the per-sweep
IMAGE_MIN_SITES = 1 << 20        # llda_pack_image pass costs more than the line fills it saves
IMAGE_MAX_ESCAPES = 0.5          # image=None: the narrowest image whose sampled escape rate stays below this (measured: with 35 % of
                                 # the gathers escaping -- the sparse variant of configs[3] at 1 M documents -- the 8-bit image is still
                                 # 18 % faster than the 16-bit one: the escapes go to the hot words' rows, which the L2s hold)
IMAGE_ORDER_MAX_LINES = 0.9      # image_order=None: taken when a site then touches at most this share of the lines it touched before
IMAGE_LINE_BYTES = 128           # a cache line of the narrow image
COMMIT_LOG_MIN_SITES = 1 << 20   # commit_log=None: below this the extra pass costs more than the atomics it saves
MAX_CALL_SITES = (1 << 30) - 1   # llda_sweep addresses the sites of one call with 32-bit byte offsets
MAX_CALL_SITES_REC = (1 << 28) - 1   # ... and the 16-byte site records of narrow layouts
LOG_ITEM = 4096      # most log entries one wavefront of llda_commit_log folds (hot words are cut into items)
PAIR_LIMIT = 32767   # largest frequency mass of a word (all ranks) whose row is exchanged as int16 pairs
MAX_FREQ = 1 << 23   # v_mad_i32_i24 moves a site's count (include/llda_gibbs.h: freq)
HEAVY_TOPICS = 64    # a document that allows more topics than this, or more than K / HEAVY_K_PARTS, is HEAVY: the dense kernel
HEAVY_K_PARTS = 4    # with its label mask sweeps it, in a launch of its own
LANE_CLASSES = ((8, -1), (16, 8), (32, 16), (64, 32))   # sparse-label launches: (lanes per document, allowed topics above)
PRIOR_MIN = 1e-6     # the tiered kernels' domain (priors.PRIOR_MIN): below it the library runs the all-exact kernel, which has no images
VBETA_MAX = 2.0 ** 40

Options = collections.namedtuple("Options", "rows16 quad image")
Log = collections.namedtuple("Log", "commit_log site_rec call_limit")
Rows = collections.namedtuple("Rows", "form tolerate_oom max_doc_tokens")     # form: "int32", "two_doc16" or "quad16"
SamplerPlan = collections.namedtuple(
    "SamplerPlan", "commit_log site_rec call_limit sparse heavy_docs scratch rows max_doc_tokens image_bits image_order")
SamplerPlan.__new__.__defaults__ = (False, False, MAX_CALL_SITES, False, 0, False, "int32", 0, 0, False)

ENVIRONMENT = (("LLDA_ROWS16", ("on", "off")), ("LLDA_QUAD", ("on", "off")), ("LLDA_IMAGE", ("0", "8", "16")))


def options(rows16, quad, image):
    """the three arguments a caller behind the LabeledLDA front end cannot pass, from the environment: LLDA_ROWS16=on|off,
    LLDA_QUAD=on|off, LLDA_IMAGE=0|8|16.  An explicit argument wins.  (``image`` itself is checked by ``image_bits``.)"""
    env = {}
    for var, allowed in ENVIRONMENT:
        env[var] = os.environ.get(var)
        if env[var] is not None and env[var] not in allowed:
            raise ValueError("%s=%r: expected one of %s" % (var, env[var], ", ".join(allowed)))
    if rows16 is None and env["LLDA_ROWS16"] is not None:
        rows16 = env["LLDA_ROWS16"] == "on"
    if quad is None and env["LLDA_QUAD"] is not None:
        quad = env["LLDA_QUAD"] == "on"
    if image is None and env["LLDA_IMAGE"] is not None:
        image = int(env["LLDA_IMAGE"])
    return Options(rows16, quad, image)


def commit_log(wanted, S, G, max_call_sites=MAX_CALL_SITES, max_call_sites_rec=MAX_CALL_SITES_REC):
    """wanted=None: the log from COMMIT_LOG_MIN_SITES local sites up.  Never from 2^31 sites (log positions are int32) nor without
    sites.  Layouts with 8 or 16 lanes per document read {word, freq, csc_pos} as one 16-byte record per site, which bounds a call."""
    if wanted is None:
        wanted = S >= COMMIT_LOG_MIN_SITES
    on = bool(wanted) and 0 < S < (1 << 31)
    rec = on and G <= 16
    return Log(on, rec, min(max_call_sites, max_call_sites_rec) if rec else max_call_sites)


def doc_is_heavy(allowed, K):
    """(GibbsSampler._make_live states this on a tensor, from the two constants)"""
    return allowed > HEAVY_TOPICS or allowed * HEAVY_K_PARTS > K


def shard_is_dense(heavy_docs, D):
    """more than half of the documents heavy: the whole shard takes the dense kernel, as if sparse_labels were off"""
    return heavy_docs * 2 > D


def one_launch(sparse, live_max, heavy_docs):
    """dense masks, or sparse label sets of at most LANE_CLASSES[0] topics in every document: one launch per llda_sweep call"""
    return not sparse or (live_max <= LANE_CLASSES[0][0] and not heavy_docs)


def scratch(wide, D, sparse, heavy_docs):
    """wide layouts: work space for the dense / general kernel -- which also sweeps the heavy documents of sparse label sets"""
    return bool(wide and D > 0 and (not sparse or heavy_docs))


def priors_in_domain(alpha, beta):
    return alpha >= PRIOR_MIN and beta >= PRIOR_MIN


def too_many_wide_sites(share, S, max_wide_sites=QUAD_MAX_WIDE_SITES):
    """share = sites whose word's row does not fit the 16-bit image (the quad kernel reads such a row without prefetch)"""
    return share > max_wide_sites * S


def rows_possible(rows16, quad, S, dense_mask, logged, rows16_ok, quad_ok, alpha, beta):
    """the 16-bit rows are not off, and the library has a kernel that reads them for this K and these arguments.
    rows16_ok / quad_ok: the library's answers for this K."""
    return bool(rows16 is not False and S and dense_mask and logged and (rows16_ok or (quad is not False and quad_ok))
                and priors_in_domain(alpha, beta))


def rows(rows16, quad, S, V, KP, rows16_ok, quad_ok, max_doc_tokens, tokens_max, wide_share, any_row_fits,
         min_bytes=ROWS16_MIN_BYTES, max_wide_sites=QUAD_MAX_WIDE_SITES):
    """where ``rows_possible`` -> Rows: the form of the n_kw rows the dense-mask kernels read, whether a failed allocation of the
    image is tolerated (rows16=None: the shard then sweeps with int32 rows) and llda_sweep_args.max_doc_tokens.
    tokens_max(): the most tokens any document holds; wide_share(): the sites whose word has a count beyond 16 bits somewhere in
    its row; any_row_fits(): does any row's total fit 16 bits."""
    keep = Rows("int32", False, max_doc_tokens)
    auto = rows16 is None
    # site_row is an int32: the last 16-bit row starts (V+1)*KP/4 + (V-1)*KP/8 units of 16 bytes after n_kw
    if (V + 1) * (KP // 4) + V * (KP // 8) >= 1 << 31:
        if auto:
            return keep
        raise ValueError("rows16=True: n_kw of %d x %d is too large for the 32-bit row offsets of the 16-bit-row kernel" % (V, KP))
    tokens = tokens_max()
    four_waves = 0 < tokens < 65536       # the kernels pack n_dk with its sweep-start value and run four waves per SIMD
    if auto and not four_waves and V * KP * 4 < min_bytes:
        return keep
    # (the quad kernel addresses the image and the commit log with 32-bit byte offsets.  S is the whole shard, not a call: the calls
    # of a shard share one log, and csrc/sweep_plan.hpp sees one call's n_sites only -- a shard of 2^30 sites and more sweeps with the
    # two-document kernel, tests/test_gpu_offset_edges.py two_calls)
    as_quad = bool(quad is not False and four_waves and quad_ok and V < (1 << 22) and S < (1 << 30))
    if as_quad and quad is None and too_many_wide_sites(wide_share(), S, max_wide_sites):
        as_quad = False                   # ... the two-document kernel's prefetched int32 rows
    if quad and not as_quad:
        raise ValueError("quad=True: needs a K with llda_quad_ok (16 slots per lane in 8, 16 or 32 lanes: K = 100, 128, 200, 256, 400, 512 ...), "
                         "documents of fewer than 65 536 tokens, a vocabulary below 2^22 words and fewer than 2^30 sites")
    if as_quad:
        return Rows("quad16", auto, tokens)
    if not (rows16_ok and any_row_fits()):
        return keep
    return Rows("two_doc16", auto, max_doc_tokens or tokens)


def quad_handover(share, S, rows16_ok, max_wide_sites=QUAD_MAX_WIDE_SITES):
    """quad=None, every QUAD_CHECK_EVERY sweeps: None = stay, else the form the sampler goes over to for good -- the two-document
    kernel where the library has it for this K (512), else the int32 rows of the general kernel (K = 128, 256)"""
    if not too_many_wide_sites(share, S, max_wide_sites):
        return None
    return "two_doc16" if rows16_ok else "int32"


def image_bits(image, S, V, KP, sparse, live_max, alpha, beta, escape_rates, min_bytes=IMAGE_MIN_BYTES, min_sites=IMAGE_MIN_SITES,
               max_escapes=IMAGE_MAX_ESCAPES):
    """-> 8, 16 or 0 (none): the saturating narrow image of n_kw the sparse-label kernels gather from.  image=None picks by the size
    of the problem and escape_rates() -> (rate8, rate16), the sampled share of the gathers that would saturate either image."""
    if image not in (None, 0, 8, 16):
        raise ValueError("image must be None (automatic), 0 (off), 8 or 16")
    if not (image != 0 and S and sparse and priors_in_domain(alpha, beta) and V * beta < VBETA_MAX):
        return 0
    if live_max == 0:
        return 0                          # (every document is heavy: no launch of the sparse-label kernel)
    if image is not None:
        return image
    if V * KP * 4 < min_bytes or S < min_sites:
        return 0
    r8, r16 = escape_rates()
    return 8 if r8 <= max_escapes else 16 if r16 <= max_escapes else 0


def image_cols_per_line(bits):
    return IMAGE_LINE_BYTES * 8 // bits


def image_order_possible(image_order, KP, bits):
    """a row of at most one line has no order to gain"""
    return image_order is not False and KP > image_cols_per_line(bits)


def image_order_taken(image_order, before, after):
    """before / after: lines a site touches with the plain and with the clustered column order"""
    return image_order is True or after <= IMAGE_ORDER_MAX_LINES * before
