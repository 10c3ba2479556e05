"""llda_label_metrics and llda_label_sets without a GPU: the exported symbols and the two structs, and every refusal of the header --
all of them decided on the host before any HIP call (the pointers below are never dereferenced there)."""
import ctypes

import pytest

BAD_K, BAD_ARG = -1, -2
MAX_K = 7688


@pytest.fixture(scope="module")
def nat():
    from lda_thesis_amd import _native
    _native.lib()
    return _native


def test_symbols_structs_and_constants(nat):
    from test_abi import declared_symbols
    L = nat.lib()
    assert L.llda_abi_version() == 22 == nat.ABI_VERSION                # additive: the ABI number stays
    for s in ("llda_label_struct_bytes", "llda_label_scratch_bytes", "llda_label_metrics", "llda_sets_struct_bytes", "llda_label_sets"):
        assert s in nat.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_label_struct_bytes() == ctypes.sizeof(nat.LldaLabelArgs)
    assert L.llda_sets_struct_bytes() == ctypes.sizeof(nat.LldaSetsArgs)
    assert (nat.LABEL_CHUNK, nat.LABEL_TEST_CHUNK, nat.LABEL_MAX_D) == (4096, 256, 2 ** 30)
    header = open(nat.os.path.join(nat.os.path.dirname(nat._HERE), "include", "llda_gibbs.h")).read()
    assert "#define LLDA_LABEL_CHUNK 4096" in header and "#define LLDA_LABEL_TEST_CHUNK 256" in header


def label_call(nat, **kw):
    a = nat.LldaLabelArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.K, a.first, a.n_labels, a.chunk = 12, 1, 11, 0
    a.score, a.truth, a.scratch = 4096, 8192, 12288
    a.n_pos, a.n_thr, a.auc_num, a.auc, a.thr_tp, a.thr_fp, a.f1, a.thr = (16384 + 1024 * i for i in range(8))
    a.flags, a.order = 32768, 36864
    a.D, a.ld, a.scratch_bytes = 0, 12, 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_label_metrics(ctypes.byref(a), None)


def test_label_metrics_refusals_come_before_the_device(nat):
    call = lambda **kw: label_call(nat, **kw)
    assert call() == 0                                                  # D == 0: nothing to do, nothing touched
    assert call(D=9, n_labels=0) == 0                                   # no label to rank either
    assert nat.lib().llda_label_metrics(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaLabelArgs) + 8) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, first=0, n_labels=0, ld=MAX_K + 1) == BAD_K, K
    assert call(K=MAX_K, ld=MAX_K) == 0
    assert call(first=2) == BAD_ARG and call(n_labels=12) == BAD_ARG    # first + n_labels > K
    assert call(first=0, n_labels=12) == 0 and call(first=12, n_labels=0) == 0
    assert call(first=-1) == BAD_ARG and call(n_labels=-1) == BAD_ARG
    assert call(first=2 ** 31 - 1, n_labels=2 ** 31 - 1) == BAD_ARG     # (the sum is not formed in 32 bits)
    assert call(ld=11) == BAD_ARG
    assert call(D=-1) == BAD_ARG and call(D=2 ** 30 + 1) == BAD_ARG
    for chunk in (-1, 1, 128, 255, 257, 512, 4096, 8192):
        assert call(chunk=chunk) == BAD_ARG, chunk
    assert call(chunk=256) == 0
    # from here on D > 0: every call below must be refused, there is no device to take it
    for name in ("score", "truth", "scratch"):
        assert call(D=9, **{name: None}) == BAD_ARG, name
    for name in ("score", "scratch", "n_pos", "n_thr", "auc_num", "auc", "thr_tp", "thr_fp", "f1", "thr"):
        assert call(D=9, **{name: 4100}) == BAD_ARG, name              # not 8-byte aligned
    for name in ("flags", "order"):
        assert call(D=9, **{name: 4098}) == BAD_ARG, name              # not 4-byte aligned
    need = nat.label_scratch_bytes(9, 11, 0)
    assert call(D=9, scratch_bytes=need - 1) == BAD_ARG and call(D=9, scratch_bytes=0) == BAD_ARG
    need = nat.label_scratch_bytes(257, 11, 256)
    assert call(D=257, chunk=256, scratch_bytes=need - 1) == BAD_ARG
    assert call(D=2 ** 30, ld=2 ** 40, scratch_bytes=2 ** 62) == BAD_ARG   # D x ld leaves an int64


def test_label_scratch_bytes(nat):
    L = nat.lib()
    sb = nat.label_scratch_bytes
    assert sb(0, 0) > 0 and sb(5, 0) > 0                                # an allocation of that size has an address
    assert sb(1, 1) == 24 * 4096 + 16 and sb(4096, 1) == sb(1, 1) and sb(4097, 1) == 24 * 8192 + 16
    assert sb(1, 1, 256) == 24 * 256 + 16 and sb(257, 3, 256) == 24 * 512 * 3 + 16
    assert sb(100000, 511) == 24 * 102400 * 511 + 16                    # the size the header quotes: 1.26 GB
    for chunk in (0, 256):                                              # monotone in D and in n_labels
        sizes = [sb(D, 7, chunk) for D in (0, 1, 255, 256, 257, 4095, 4096, 4097, 10 ** 5, 2 ** 30)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        sizes = [sb(1000, n, chunk) for n in (0, 1, 2, 63, 64, 65, 511, MAX_K)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert sb(2 ** 30, MAX_K) < 2 ** 63
    for bad in ((-1, 3, 0), (2 ** 30 + 1, 3, 0), (5, -1, 0), (5, MAX_K + 1, 0), (5, 3, 1), (5, 3, 4096), (5, 3, -256)):
        assert L.llda_label_scratch_bytes(*bad) == BAD_ARG, bad
    with pytest.raises(nat.NativeError):
        sb(5, 3, 7)


def sets_call(nat, **kw):
    a = nat.LldaSetsArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.K, a.first, a.at_least_one = 12, 1, 1
    a.score, a.thr, a.truth = 4096, 8192, 12288
    a.mask, a.n_pred, a.n_hit, a.n_true, a.tp, a.fp, a.fn = (16384 + 1024 * i for i in range(7))
    a.D, a.ld = 0, 12
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_label_sets(ctypes.byref(a), None)


def test_label_sets_refusals_come_before_the_device(nat):
    call = lambda **kw: sets_call(nat, **kw)
    assert call() == 0                                                  # D == 0
    assert nat.lib().llda_label_sets(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaSetsArgs) + 8) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, first=0, ld=MAX_K + 1) == BAD_K, K
    assert call(first=-1) == BAD_ARG and call(first=13) == BAD_ARG and call(first=12) == 0 and call(first=0) == 0
    assert call(ld=11) == BAD_ARG and call(D=-1) == BAD_ARG
    assert call(at_least_one=2) == BAD_ARG and call(at_least_one=-1) == BAD_ARG and call(at_least_one=0) == 0
    assert call(D=2 ** 40, ld=2 ** 40) == BAD_ARG
    for name in ("score", "thr"):
        assert call(D=9, **{name: None}) == BAD_ARG, name
    for name in ("score", "thr", "tp", "fp", "fn"):
        assert call(D=9, **{name: 4100}) == BAD_ARG, name
    for name in ("mask", "n_pred", "n_hit", "n_true"):
        assert call(D=9, **{name: 4098}) == BAD_ARG, name
