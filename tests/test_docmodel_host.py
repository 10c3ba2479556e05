"""docmodel.check_offsets: the host-only check of the document offsets that heldout.loglik, attribution.attribute (D known from
theta) and leftright.loglik (D from the offsets) share."""
import numpy as np
import pytest

from lda_thesis_amd import docmodel

GIVEN = "doc_off must hold D + 1 = %d ascending offsets"
DERIVED = "doc_off must hold D + 1 ascending offsets"


def test_good_offsets_come_back_with_D_and_S():
    off_h, D, S = docmodel.check_offsets([0, 2, 2, 7], 3)
    assert off_h.dtype == np.int64 and off_h.tolist() == [0, 2, 2, 7] and (D, S) == (3, 7)
    off_h, D, S = docmodel.check_offsets(np.array([4, 4, 9], dtype=np.int64))          # (a corpus may start inside a larger array)
    assert off_h.tolist() == [4, 4, 9] and (D, S) == (2, 9)
    import torch
    off_h, D, S = docmodel.check_offsets(torch.tensor([0, 1, 3]), 2)
    assert isinstance(off_h, np.ndarray) and off_h.tolist() == [0, 1, 3] and (D, S) == (2, 3)


@pytest.mark.parametrize("off, D", [([0, 1], 2), ([0, 1, 2, 3], 2), ([], 0), ([[0, 1, 2]], 2)])
def test_wrong_length(off, D):
    with pytest.raises(ValueError) as e:
        docmodel.check_offsets(off, D)
    assert str(e.value) == GIVEN % (D + 1)


def test_no_offset_at_all_when_D_is_derived():
    for off in ([], [[0, 1], [1, 2]]):
        with pytest.raises(ValueError) as e:
            docmodel.check_offsets(off)
        assert str(e.value) == DERIVED


@pytest.mark.parametrize("D", [2, None])
def test_negative_first_offset(D):
    with pytest.raises(ValueError) as e:
        docmodel.check_offsets([-1, 0, 3], D)
    assert str(e.value) == (DERIVED if D is None else GIVEN % 3)


@pytest.mark.parametrize("D", [3, None])
@pytest.mark.parametrize("off", [[0, 5, 4, 6], [0, 1, 2, 1], [3, 2, 2, 2]])
def test_descending_pair(off, D):
    with pytest.raises(ValueError) as e:
        docmodel.check_offsets(off, D)
    assert str(e.value) == (DERIVED if D is None else GIVEN % 4)


@pytest.mark.parametrize("D", [0, None])
def test_no_document(D):
    """D = 0: one offset, whatever it is, and no site"""
    for first in (0, 5, -3):
        off_h, got_D, S = docmodel.check_offsets([first], D)
        assert off_h.tolist() == [first] and (got_D, S) == (0, 0)


@pytest.mark.parametrize("D", [3, None])
def test_empty_corpus(D):
    """documents, none with a site"""
    off_h, got_D, S = docmodel.check_offsets([0, 0, 0, 0], D)
    assert (got_D, S) == (3, 0) and off_h.tolist() == [0, 0, 0, 0]
    assert docmodel.check_offsets([6, 6, 6, 6], D)[1:] == (3, 6)
