"""csrc/quad_doc_map.hpp: how quad_tier1_doc (csrc/kernel_quad.hpp) lays ONE document over the 64 lanes of a wavefront -- lane s takes the
n = KP / 64 consecutive positions s n .. s n + n - 1 of the document's draw order.  The header is plain constexpr C++: it is compiled
here with the host compiler around a driver that prints every (lane, term), and the table is compared with what the rest of the
project says about the same positions -- the layout's own lane / slot / draw order (lda_thesis_amd/layout.py), the slot number of the
quad kernels (rho = 8 i + 2 c + e) and the place llda_pack_rows16_all writes a count to in the 16-bit image."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DRIVER = r"""
#include "quad_doc_map.hpp"
#include <stdio.h>
static_assert(quad_doc_terms(4) == 8 && quad_doc_terms(3) == 4 && quad_doc_terms(2) == 2, "KP / 64 terms per lane");
static_assert(quad_doc_pos(4, 511) == 511 && quad_doc_rho(511) == 31, "the last position of the draw order is what QUAD_KEY_NONE names");
int main()
{
    for (int LB = 2; LB <= 4; ++LB)
        for (int s = 0; s < 64; ++s)
            for (int t = 0; t < quad_doc_terms(LB); ++t) {
                const int o = quad_doc_order(LB, s, t);
                printf("%d %d %d %d %d %d %d %d %d %d %d\n", LB, s, t, o, quad_doc_pos(LB, o), quad_doc_rho(o), quad_doc_lane(o),
                       quad_doc_chain(o), quad_doc_std_lane(o), quad_doc_std_slot(o), quad_doc_image_byte(LB, o));
            }
    return 0;
}
"""
FIELDS = ("LB", "s", "t", "o", "pos", "rho", "lane", "chain", "std_lane", "std_slot", "byte")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("quad_doc_map")
    src, exe = d / "driver.cpp", str(d / "driver")
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", exe, str(src), "-I", os.path.join(ROOT, "lda_thesis_amd", "csrc")])
    rows = np.array([[int(x) for x in l.split()] for l in subprocess.check_output([exe], universal_newlines=True).splitlines()])
    return {LB: {k: rows[rows[:, 0] == LB][:, i] for i, k in enumerate(FIELDS)} for LB in (2, 3, 4)}


def quad_rho(pos, LB):
    """csrc/kernel_quad.hpp, quad_rho (tests/test_quad_entry_encoding.py holds the source to this line)"""
    return ((pos >> LB) & 0x18) | ((pos & 3) << 1) | ((pos >> 2) & 1)


def packed_byte_of_position(G):
    """llda_pack_rows16_all_kernel<G>, thread c of a row: j = c / G, g = c & (G - 1) reads slots 8 j .. 8 j + 7 of standard lane g (two
    16-byte chunks of the int32 row) and writes them, in order, as the 16-byte unit (2 j + (g & 1)) * (G / 2) + (g >> 1) of the image"""
    byte = np.full(16 * G, -1, dtype=np.int64)
    for c in range(2 * G):
        j, g = c // G, c & (G - 1)
        unit = (2 * j + (g & 1)) * (G // 2) + (g >> 1)
        for m in range(8):
            slot = 8 * j + m
            pos = (((slot >> 2) * G + g) << 2) | (slot & 3)             # pos_of<G, 16>: where the int32 row holds (g, slot)
            assert byte[pos] == -1
            byte[pos] = 16 * unit + 2 * m
    assert sorted(byte.tolist()) == list(range(0, 32 * G, 2))           # every count of the row, once
    return byte


@pytest.mark.parametrize("LB", [2, 3, 4])
def test_one_document_on_sixty_four_lanes(table, LB):
    from lda_thesis_amd.layout import GroupLayout
    T = table[LB]
    LPD, KP, G, n = 1 << LB, 32 << LB, 2 << LB, (32 << LB) // 64
    L = GroupLayout(KP)
    assert (L.G, L.T, L.KP) == (G, 16, KP)
    # (lane, term) -> position: a bijection onto 0 .. KP - 1, walked in the draw order
    assert len(T["o"]) == 64 * n == KP
    np.testing.assert_array_equal(T["o"], T["s"] * n + T["t"])
    np.testing.assert_array_equal(T["o"], np.arange(KP))
    assert sorted(T["pos"].tolist()) == list(range(KP))
    np.testing.assert_array_equal(L.draw_rank[T["pos"]], T["o"])
    # the slot number, the quad lane whose LDS holds the counts, the chain
    np.testing.assert_array_equal(T["rho"], quad_rho(T["pos"], LB))
    np.testing.assert_array_equal(T["lane"], (T["pos"] >> 3) & (LPD - 1))
    np.testing.assert_array_equal(T["chain"], (T["pos"] >> 2) & 1)
    # the validity bit: word and bit of the standard layout's lane masks (GroupLayout.lane_masks)
    np.testing.assert_array_equal(T["std_lane"], L.pos_lane[T["pos"]])
    np.testing.assert_array_equal(T["std_slot"], L.pos_slot[T["pos"]])
    np.testing.assert_array_equal(T["std_lane"], 2 * T["lane"] + T["chain"])
    # the image: the byte the packer writes the position to; a lane's n counts are 2 n contiguous bytes, aligned to 2 n (ONE load)
    np.testing.assert_array_equal(T["byte"], packed_byte_of_position(G)[T["pos"]])
    first = T["byte"][T["t"] == 0]
    assert not np.any(first % (2 * n))
    np.testing.assert_array_equal(T["byte"], np.repeat(first, n) + 2 * T["t"])
    # what quad_tier1_doc takes once per lane from term 0 is the same for all terms of the lane
    for k in ("lane", "chain", "std_lane"):
        np.testing.assert_array_equal(T[k], np.repeat(T[k][T["t"] == 0], n))
    # the count's place in the per-document LDS arrays [rho >> 2][thread][rho & 3] is the one the kernel's prologue fills for the
    # position (i << IS) + lq * 8 + j: rho = 8 i + 2 (j & 3) + (j >> 2)
    i, lq, j = T["pos"] >> (3 + LB), (T["pos"] >> 3) & (LPD - 1), T["pos"] & 7
    np.testing.assert_array_equal(T["rho"], 8 * i + 2 * (j & 3) + (j >> 2))
    np.testing.assert_array_equal(T["lane"], lq)
