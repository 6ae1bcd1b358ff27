"""numpy restatement of the pixel arithmetic of the library's JPEG decoder (csrc/jpeg.hip): DCT
coefficients and quantisation tables as eosv_jpeg_entropy writes them -> the [H,W,3] uint8 RGB image
libjpeg (PIL) decodes.  All 32-bit integer arithmetic with arithmetic right shifts: dequantisation,
the 13-bit slow-integer inverse DCT, the triangle-filter 4:2:0 upsampling, 16-bit fixed-point
YCbCr -> RGB.  Used by tests/test_cpu_jpeg.py (the host stage against PIL without a GPU)."""
import ctypes

import numpy as np

from eosv import _lib


def _idct_lines(x):
    """8-point inverse DCT along the last axis, before the descale (int64 holds the int32 values)."""
    i = [x[..., k] for k in range(8)]
    z = (i[2] + i[6]) * 4433
    t2, t3 = z - i[6] * 15137, z + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i[7], i[5], i[3], i[1]
    z5 = (a + c + b + d) * 9633
    z1, z2 = -(a + d) * 7373, -(b + c) * 20995
    z3, z4 = -(a + c) * 16069 + z5, -(b + d) * 3196 + z5
    a, b, c, d = a * 2446 + z1 + z3, b * 16819 + z2 + z4, c * 25172 + z2 + z3, d * 12299 + z1 + z4
    return np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], axis=-1)


def plane(coef, q):
    """coef [bh,bw,64] int16 (natural order), q [64] -> uint8 plane [bh*8, bw*8]."""
    bh, bw, _ = coef.shape
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(bh, bw, 8, 8)
    ws = (_idct_lines(x.transpose(0, 1, 3, 2)) + (1 << 10)) >> 11  # down the columns: [.., column, row]
    out = (_idct_lines(ws.transpose(0, 1, 3, 2)) + (1 << 17)) >> 18  # along the rows: [.., row, column]
    out = np.clip(out + 128, 0, 255)
    return out.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample420(c, H, W):
    """chroma plane (padded) -> [H,W]: reads only its ceil(H/2) x ceil(W/2) samples."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    c = c[:ch, :cw].astype(np.int64)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    rows = np.arange(ch)
    for v in (0, 1):
        r2 = np.clip(rows - 1 if v == 0 else rows + 1, 0, ch - 1)
        s = 3 * c + c[r2]
        prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[v::2, 0::2] = (3 * s + prev + 8) >> 4  # first column: (4 s[0] + 8) >> 4
        out[v::2, 1::2] = (3 * s + nxt + 7) >> 4   # last column: (4 s[last] + 7) >> 4
    return out[:H, :W]


def rgb_from_coefficients(coef, quant, W, H, sampling):
    """One frame's coefficients (int16, [component][block row][block column][64]) and tables
    ([3,64]) -> [H,W,3] uint8."""
    s = 2 if sampling == _lib.JPEG_420 else 1
    mx, my = -(-W // (8 * s)), -(-H // (8 * s))
    ny = mx * s * my * s * 64
    Y = plane(coef[:ny].reshape(my * s, mx * s, 64), quant[0])[:H, :W]
    if sampling == _lib.JPEG_GREY:
        return np.stack([Y, Y, Y], axis=-1).astype(np.uint8)
    nc = mx * my * 64
    cb = plane(coef[ny:ny + nc].reshape(my, mx, 64), quant[1])
    cr = plane(coef[ny + nc:ny + 2 * nc].reshape(my, mx, 64), quant[2])
    if sampling == _lib.JPEG_420:
        cb, cr = upsample420(cb, H, W), upsample420(cr, H, W)
    else:
        cb, cr = cb[:H, :W], cr[:H, :W]
    cb, cr = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


class Scan:
    """eosv_jpeg_scan over a list of byte strings, through ctypes alone (no torch, no GPU)."""

    def __init__(self, blobs):
        n = len(blobs)
        self.n = n
        self.blobs = list(blobs)
        self.data = (ctypes.c_char_p * max(n, 1))(*self.blobs)
        self.nbytes = (ctypes.c_int64 * max(n, 1))(*[len(b) for b in self.blobs])
        self.frames = (_lib.EosvJpegFrame * max(n, 1))()
        assert _lib.lib().eosv_jpeg_scan(self.data, self.nbytes, n, self.frames) == 0

    def status(self):
        return [self.frames[i].status for i in range(self.n)]

    def entropy(self, threads, guard=0):
        """(coef int16, quant uint16 [n,3,64], offsets); frames refused by the scan take no room."""
        offs, total = [], 0
        for i in range(self.n):
            f = self.frames[i]
            f.coef_offset = total
            offs.append(total)
            total += f.coef_elems if f.status == 0 else 0
        coef = np.full(total + 2 * guard, 0x5A5A, np.int16)
        quant = np.zeros((self.n, 3, 64), np.uint16)
        body = coef[guard:guard + total]
        assert _lib.lib().eosv_jpeg_entropy(self.data, self.nbytes, self.n, self.frames, body.ctypes.data, total,
                                            quant.ctypes.data, threads) == 0
        assert (coef[:guard] == 0x5A5A).all() and (coef[guard + total:] == 0x5A5A).all()
        return body, quant, offs

    def image(self, i, coef, quant, offs):
        f = self.frames[i]
        return rgb_from_coefficients(coef[offs[i]:offs[i] + f.coef_elems], quant[i], f.width, f.height, f.sampling)
