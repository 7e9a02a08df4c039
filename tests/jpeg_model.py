"""An independent statement of the baseline JPEG encoder that csrc/jpeg.hip implements, for tests/test_jpeg_cpu.py and
tests/test_jpeg_gpu.py: written from ITU-T T.81 (Annex A: DCT and zigzag, Annex C / F: Huffman coding, Annex K: tables) and
from libjpeg's documented integer colour conversion and 2x2 downsampling.  fp64 / integer numpy plus a bit-level writer in
plain Python; it imports nothing from the package.

    coefficients(frames, quality) -> (coef int16 (n, R, C, 6, 64), unquantised fp64 values, divisors)
    entropy_segment(coef_frame, restart_mcus) -> (bytes, per-interval padding bit counts)
"""

import numpy as np

# T.81 Table K.1 / K.2, natural (row-major) order
LUMA_BASE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
    100, 103, 99], dtype=np.int64)
CHROMA_BASE = np.array([17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99], dtype=np.int64)
CHROMA_BASE = np.pad(CHROMA_BASE.reshape(4, 4), ((0, 4), (0, 4)), constant_values=99).reshape(64)

# T.81 Tables K.3 - K.6: (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFFMAN_SPECS = (DC_LUMA, DC_CHROMA, AC_LUMA, AC_CHROMA)


def zigzag():
    """zigzag position -> natural index, walked diagonal by diagonal (T.81 Figure A.6)."""
    order, r, c, up = [], 0, 0, True
    for _ in range(64):
        order.append(r * 8 + c)
        if up:
            if c == 7: r, up = r + 1, False
            elif r == 0: c, up = c + 1, False
            else: r, c = r - 1, c + 1
        else:
            if r == 7: c, up = c + 1, True
            elif c == 0: r, up = r + 1, True
            else: r, c = r + 1, c - 1
    return np.array(order)


ZIGZAG = zigzag()


def quant_tables(quality):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): natural order, int64."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA_BASE, CHROMA_BASE))


def planes(frames):
    """uint8 (n, h, w, 3) -> level-unshifted integer planes Y (n, 16R, 16C), Cb / Cr (n, 8R, 8C) of the replicated picture."""
    n, h, w, _ = frames.shape
    rows, cols = -(-h // 16), -(-w // 16)
    p = np.pad(frames, ((0, 0), (0, rows * 16 - h), (0, cols * 16 - w), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    bias = np.tile(np.array([1, 2]), cols * 4)

    def down(c):
        return (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + bias) >> 2

    return y, down(cb), down(cr)


def dct_matrix():
    u, x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    d = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    d[0] = np.sqrt(1 / 8)
    return d


def blocks_of(frames):
    """(n, R, C, 6, 8, 8) fp64 level-shifted blocks in the order Y00 Y01 Y10 Y11 Cb Cr."""
    y, cb, cr = planes(frames)
    n, hh, ww = y.shape
    rows, cols = hh // 16, ww // 16
    yb = y.reshape(n, rows, 2, 8, cols, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(n, rows, cols, 4, 8, 8)
    cbb = cb.reshape(n, rows, 8, cols, 8).transpose(0, 1, 3, 2, 4)[:, :, :, None]
    crb = cr.reshape(n, rows, 8, cols, 8).transpose(0, 1, 3, 2, 4)[:, :, :, None]
    return np.concatenate([yb, cbb, crb], axis=3).astype(np.float64) - 128.0


def quantise(f, div):
    """fp64 DCT values (.., 6, 64) in zigzag order / divisors -> int16: half away from zero, AC clamped to +-1023."""
    v = f / div
    q = np.sign(v) * np.floor(np.abs(v) + 0.5)
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q.astype(np.int16)


def divisors(quality):
    """(6, 64) divisors in zigzag order, per block of the MCU."""
    lu, ch = quant_tables(quality)
    return np.stack([lu[ZIGZAG]] * 4 + [ch[ZIGZAG]] * 2).astype(np.float64)


def coefficients(frames, quality):
    """-> (coef int16 (n, R, C, 6, 64) zigzag, f fp64 unquantised DCT values same shape, div (6, 64))."""
    d = dct_matrix()
    b = blocks_of(frames)
    f = np.einsum("ux,...xy,vy->...uv", d, b, d).reshape(*b.shape[:4], 64)[..., ZIGZAG]
    div = divisors(quality)
    return quantise(f, div), f, div


def near_boundary(f, div, width):
    """Where the unquantised value lies within `width` of a rounding boundary (k + 1/2) * q, in unquantised units."""
    v = np.abs(f) / div
    frac = v - np.floor(v)
    return np.abs(frac - 0.5) * div <= width


def huffman_codes(spec):
    """symbol -> (code, length): the canonical assignment of T.81 Annex C."""
    bits, vals = spec
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


CODES = [huffman_codes(s) for s in HUFFMAN_SPECS]


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def value(self, table, run, v):
        size = int(abs(v)).bit_length()
        self.put(*table[(run << 4) | size])
        if size:
            self.put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)

    def flush(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        data = self.acc.to_bytes(self.n // 8, "big")
        self.acc, self.n = 0, 0
        return data.replace(b"\xff", b"\xff\x00"), pad


def entropy_segment(coef, restart_mcus):
    """coef (R, C, 6, 64) int16 -> (entropy-coded segment of the scan, list of padding bits per restart interval)."""
    mcus = coef.reshape(-1, 6, 64).astype(np.int64).tolist()
    out, pads, bits, pred = [], [], _Bits(), [0, 0, 0]
    for m, mcu in enumerate(mcus):
        if m and m % restart_mcus == 0:
            data, pad = bits.flush()
            out.append(data + bytes([0xFF, 0xD0 + (m // restart_mcus - 1) % 8]))
            pads.append(pad)
            pred = [0, 0, 0]
        for b, block in enumerate(mcu):
            comp = max(0, b - 3)
            dc_tab, ac_tab = CODES[1 if comp else 0], CODES[3 if comp else 2]
            bits.value(dc_tab, 0, block[0] - pred[comp])
            pred[comp] = block[0]
            run = 0
            for v in block[1:]:
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    bits.put(*ac_tab[0xF0])
                    run -= 16
                bits.value(ac_tab, run, v)
                run = 0
            if run:
                bits.put(*ac_tab[0x00])
    data, pad = bits.flush()
    out.append(data)
    pads.append(pad)
    return b"".join(out), pads


# ------------------------------------------------------------------------------------------------ inputs of the tests
def noise_frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def scene_frames(n, h, w, seed):
    """A smooth two-sinusoid colour field that moves from frame to frame, plus sigma = 8 noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((n, h, w, 3))
    for f in range(n):
        for c in range(3):
            out[f, :, :, c] = (128 + 70 * np.sin(2 * np.pi * (x / (37.0 + 9 * c) + 0.13 * f))
                               + 45 * np.sin(2 * np.pi * (y / (23.0 + 5 * c) + x / 91.0 - 0.07 * f * (c + 1))))
    return np.clip(np.rint(out + rng.normal(0, 8, out.shape)), 0, 255).astype(np.uint8)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse) if mse else np.inf


# ------------------------------------------------------------------------------------------------ RIFF walker
def walk_avi(data):
    """Parse an AVI 1.0 file strictly: every chunk and list must add up to the file length.  -> dict with `avih` (14 ints),
    `strh` (bytes), `strf` (bytes), `frames` (payloads of the 00dc chunks), `frame_offsets` (of each 00dc chunk header from
    the `movi` fourcc), `index` (list of (ckid, flags, offset, size))."""
    import struct

    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8, "RIFF size is not the file length"
    res = {"frames": [], "frame_offsets": [], "index": [], "lists": []}

    def chunks(lo, hi, movi_at=None):
        at = lo
        while at < hi:
            assert at + 8 <= hi, "chunk header crosses its parent's end"
            cc, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
            body, end = at + 8, at + 8 + size
            assert end <= hi, f"{cc!r} of {size} bytes crosses its parent's end"
            if cc == b"LIST":
                kind = data[body:body + 4]
                res["lists"].append(kind)
                chunks(body + 4, end, movi_at=body if kind == b"movi" else None)
            elif cc == b"avih":
                assert size == 56
                res["avih"] = struct.unpack("<14I", data[body:end])
            elif cc == b"strh":
                res["strh"] = data[body:end]
            elif cc == b"strf":
                res["strf"] = data[body:end]
            elif cc == b"00dc":
                assert movi_at is not None, "a frame outside LIST movi"
                res["frames"].append(data[body:end])
                res["frame_offsets"].append(at - movi_at)
            elif cc == b"idx1":
                assert size % 16 == 0
                res["index"] = [struct.unpack("<4sIII", data[body + 16 * i:body + 16 * i + 16]) for i in range(size // 16)]
            else:
                raise AssertionError(f"unexpected chunk {cc!r}")
            at = end + (size & 1)
            if size & 1:
                assert at <= hi and data[end] == 0, "an odd chunk is not padded with a zero byte"
        assert at == hi, "chunks do not add up to their parent's size"

    chunks(12, len(data))
    return res
