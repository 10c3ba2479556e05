"""numpy statements of the image packers (llda_pack_rows16, llda_pack_rows16_all, llda_pack_image, llda_pack_image_cols), written
from the side of the kernels that READ the images, and the sentinel-margin buffers of tests/test_gpu_count_kernels.py.

A row of n_kw with 16 slots per lane holds slot s of lane g at position ((s // 4) * G + g) * 4 + s % 4 (lda_thesis_amd/layout.py).
The two readers of its 16-bit image:

  * the R16 loader of llda_sweep_kernel (csrc/kernel_sweep.hpp, load_word_row): lane g reads the 16-byte units g and G + g of the
    row; half h of register r of unit j is the count of slot 8 j + 2 r + h -- unit j * G + g holds the slots 8 j .. 8 j + 7 of
    lane g as eight uint16 in slot order;
  * load_row16 / convert_row of the quad kernel (csrc/kernel_quad.hpp): quad lane lq reads the units (2 j + e) * G / 2 + lq for
    j, e = 0, 1 and takes unit (j, e) as the slots 8 j .. 8 j + 7 of standard lane 2 lq + e, again eight uint16 in slot order.

``decode_rows16`` / ``decode_quad`` state those two orders; the packers' references are their inverses.
"""
import numpy as np

MARGIN = 64             # sentinel elements in front of and behind every buffer a kernel writes


def lane_slot(rows, G):
    """(V, 16 G) rows in memory order -> (V, G, 16): [v, lane, slot]"""
    rows = np.asarray(rows)
    return rows.reshape(-1, 4, G, 4).transpose(0, 2, 1, 3).reshape(-1, G, 16)


def decode_rows16(img, G):
    """(V, 16 G) uint16 image of llda_pack_rows16 -> (V, G, 16) as the R16 loader reads it"""
    return np.asarray(img).reshape(-1, 2, G, 8).transpose(0, 2, 1, 3).reshape(-1, G, 16)


def decode_quad(img, G):
    """(V, 16 G) uint16 image of llda_pack_rows16_all -> (V, G, 16) as load_row16 / convert_row read it"""
    a = np.asarray(img).reshape(-1, 2, 2, G // 2, 8)            # [v, j, e, lq, m]
    return a.transpose(0, 3, 2, 1, 4).reshape(-1, G, 16)       # [v, lq, e, j, m] -> lane 2 lq + e, slot 8 j + m


def _out_of_range(n_kw):
    n = np.asarray(n_kw).astype(np.int64)
    return ((n < 0) | (n > 65535)).any(axis=1)


def pack_rows16_ref(n_kw, row16, G, img):
    """-> (image, status): ``img`` (V, 16 G) uint16 with the rows flagged in row16 replaced by their 16-bit image, and 4 when a
    flagged row holds a count outside 0 .. 65535 (else 0)"""
    n_kw = np.asarray(n_kw).reshape(-1, 16 * G)
    out = np.array(img, dtype=np.uint16).reshape(-1, 16 * G)
    ls = (lane_slot(n_kw, G).astype(np.int64) & 0xffff).astype(np.uint16)          # [v, g, 8 j + m]
    packed = ls.reshape(-1, G, 2, 8).transpose(0, 2, 1, 3).reshape(-1, 16 * G)     # unit j * G + g
    flagged = np.asarray(row16) != 0
    out[flagged] = packed[flagged]
    return out, 4 if (flagged & _out_of_range(n_kw)).any() else 0


def pack_rows16_all_ref(n_kw, G):
    """-> (image (V, 16 G) uint16 of EVERY row, row16 (V,) uint8: 1 iff every count of the row is in 0 .. 65535)"""
    n_kw = np.asarray(n_kw).reshape(-1, 16 * G)
    ls = (lane_slot(n_kw, G).astype(np.int64) & 0xffff).astype(np.uint16)
    a = ls.reshape(-1, G // 2, 2, 2, 8)                          # [v, lq, e, j, m]
    packed = a.transpose(0, 3, 2, 1, 4).reshape(-1, 16 * G)     # unit (2 j + e) * G / 2 + lq
    return packed, (~_out_of_range(n_kw)).astype(np.uint8)


def pack_image_ref(n_kw, bits, col_src=None):
    """the saturating image: min(count as uint32, 255 | 65535) -- a negative count saturates -- as uint8 / uint16, in the shape of
    n_kw; with col_src, image column c of every row holds the count at position col_src[c]"""
    n_kw = np.ascontiguousarray(n_kw, dtype=np.int32)
    if col_src is not None:
        n_kw = np.ascontiguousarray(n_kw[:, np.asarray(col_src).astype(np.int64)])
    sat = {8: 255, 16: 65535}[bits]
    return np.minimum(n_kw.view(np.uint32), np.uint32(sat)).astype({8: np.uint8, 16: np.uint16}[bits])


# ------------------------------------------------------------------------------------------------
# buffers with sentinel margins
# ------------------------------------------------------------------------------------------------
SENTINEL = {"int32": -0x5A5A5A5B, "int16": 0x5A5B, "uint8": 0xA5, "float64": -12345.678, "int64": -0x5A5A5A5A5A5A5A5B}


def with_margins(body, shift=0):
    """numpy copy of the 1-D array ``body`` with MARGIN + shift sentinel elements in front and MARGIN behind"""
    body = np.ascontiguousarray(body).reshape(-1)
    s = SENTINEL[body.dtype.name]
    return np.concatenate([np.full(MARGIN + shift, s, dtype=body.dtype), body, np.full(MARGIN, s, dtype=body.dtype)])


class Guarded(object):
    """a device buffer with sentinel margins: ``t`` is the body (a 1-D slice, what the kernel is given), ``host()`` the body's
    contents after checking that both margins still hold the sentinel.  shift = s moves the body by s elements, for the entry
    points that take a pointer of any alignment."""

    def __init__(self, body, shift=0):
        import torch
        body = np.ascontiguousarray(body).reshape(-1)
        self.dtype = body.dtype
        if body.dtype == np.uint16:                             # (torch: as int16, the same bits)
            body = body.view(np.int16)
        self.full = torch.from_numpy(with_margins(body, shift)).cuda()
        self.lo, self.n = MARGIN + shift, int(body.size)
        self.t = self.full[self.lo:self.lo + self.n]
        self.sentinel = SENTINEL[body.dtype.name]

    def host(self, what=""):
        a = self.full.cpu().numpy()
        assert (a[:self.lo] == self.sentinel).all(), "%s: written in front of the buffer" % what
        assert (a[self.lo + self.n:] == self.sentinel).all(), "%s: written behind the buffer" % what
        return a[self.lo:self.lo + self.n].view(self.dtype)
