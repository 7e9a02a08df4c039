"""An independent statement of the baseline JPEG decoder that csrc/jpeg_decode.hip implements, for tests/test_jpeg_decode_cpu.py
and tests/test_jpeg_decode_gpu.py: written from ITU-T T.81 (Annex B: markers, Annex C / F: Huffman decoding, Annex A: zigzag)
and from libjpeg's documented integer arithmetic (jidctint's inverse DCT, jdsample's triangle-filter upsampling, jdcolor's
YCbCr -> RGB).  Integer numpy plus a symbol-level decoder in plain Python; it imports nothing from the package.

    parse(data)                         -> Header (its own marker walk)
    decode_serial(data)                 -> coef int16 (mcu_rows, mcu_cols, blocks_per_mcu, 64), zigzag, DC absolute
    emulate_passes(data, subseq_bits)   -> (the same coef by the multi-pass scheme, count of passes)
    pixels(data, coef=None)             -> (h, w, 3) uint8
    fixtures()                          -> the table of test files: name -> (bytes, subseq_bits)
"""

import functools
import io
import struct

import numpy as np

from tests import jpeg_model

ZIGZAG = jpeg_model.ZIGZAG
CONT, STOP, BAD = 0, 1, 2


class Header:
    pass


def parse(data):
    """SOI .. SOS of a baseline file; asserts the scope instead of reporting it (the package's parser is what is under test)."""
    assert data[:2] == b"\xff\xd8"
    h = Header()
    h.quant, h.dht, h.restart, at = {}, {}, 0, 2
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        body = data[at + 4:at + 2 + length]
        if marker == 0xDB:
            for k in range(0, len(body), 65):
                assert body[k] >> 4 == 0
                table = np.zeros(64, np.int64)
                table[ZIGZAG] = np.frombuffer(body[k + 1:k + 65], np.uint8)
                h.quant[body[k] & 15] = table
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                bits = list(body[k + 1:k + 17])
                h.dht[(body[k] >> 4, body[k] & 15)] = (bits, list(body[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        elif marker == 0xC0:
            assert body[0] == 8
            h.height, h.width, n = struct.unpack(">HHB", body[1:6])
            h.comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(n)]
        elif marker == 0xDD:
            h.restart = struct.unpack(">H", body)[0]
        elif marker == 0xDA:
            n = body[0]
            assert n == len(h.comps) and tuple(body[1 + 2 * n:4 + 2 * n]) == (0, 63, 0)
            h.td = [body[2 + 2 * i] >> 4 for i in range(n)]
            h.ta = [body[2 + 2 * i] & 15 for i in range(n)]
            break
        else:
            assert marker not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"
        at += 2 + length
    h.start = at + 2 + length
    h.end = data.rfind(b"\xff\xd9")
    if h.end < h.start:
        h.end = len(data)
    h.ncomp = len(h.comps)
    h.hs, h.vs = (h.comps[0][1], h.comps[0][2]) if h.ncomp == 3 else (1, 1)
    h.bpm = 1 if h.ncomp == 1 else h.hs * h.vs + 2
    h.blk_comp = [0] if h.ncomp == 1 else [0] * (h.hs * h.vs) + [1, 2]
    h.mcu_cols, h.mcu_rows = -(-h.width // (8 * h.hs)), -(-h.height // (8 * h.vs))
    h.total_mcus = h.mcu_cols * h.mcu_rows
    h.interval = min(h.restart, h.total_mcus) if h.restart else h.total_mcus
    h.n_iv = -(-h.total_mcus // h.interval)
    return h


def unstuff_split(seg, n_iv):
    """The entropy-coded segment -> (clean bytes, [start of every interval .. end]) serially; ValueError for what the device
    reports in its error word."""
    clean, starts, i, k = bytearray(), [0], 0, 0
    while i < len(seg):
        b = seg[i]
        if b != 0xFF:
            clean.append(b)
            i += 1
            continue
        nxt = seg[i + 1] if i + 1 < len(seg) else -1
        if nxt == 0x00:
            clean.append(0xFF)
        elif 0xD0 <= nxt <= 0xD7:
            if nxt != 0xD0 + k % 8:
                raise ValueError("restart markers out of order")
            k += 1
            starts.append(len(clean))
        else:
            raise ValueError("a 0xFF that neither 0x00 nor RSTn follows")
        i += 2
    if k != n_iv - 1:
        raise ValueError("number of restart markers")
    return bytes(clean), starts + [len(clean)]


def code_table(spec):
    """(bits16, vals) -> two lists over every 16-bit window: length of the code that starts it (0: unassigned) and its symbol."""
    bits, vals = spec
    length, symbol = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lo = code << (16 - l)
            length[lo:lo + (1 << (16 - l))] = l
            symbol[lo:lo + (1 << (16 - l))] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return length.tolist(), symbol.tolist()


class Stream:
    """The clean stream as 32-bit windows at every bit position (1-bits behind the end), plus the tables of each block."""

    def __init__(self, data):
        self.h = h = parse(data)
        self.clean, self.bounds = unstuff_split(data[h.start:h.end], h.n_iv)
        bits = np.unpackbits(np.frombuffer(self.clean + b"\xff" * 8, np.uint8)).astype(np.int64)
        n = 8 * len(self.clean)
        win = np.zeros(n + 1, np.int64)
        for i in range(32):
            win = (win << 1) | bits[i:i + n + 1]
        self.win = win.tolist()
        tables = {key: code_table(spec) for key, spec in h.dht.items()}
        self.dc = [tables[(0, h.td[c])] for c in h.blk_comp]
        self.ac = [tables[(1, h.ta[c])] for c in h.blk_comp]

    def run(self, pos, blk, zz, sub_end, end_bits, out=None, block=0, block_end=0):
        """One lane from (pos, blk, zz) until it has stepped past sub_end: -> (pos, blk, zz, blocks completed, STOP | BAD as bits).
        BAD: the walk met what no valid stream holds and went on by the rules of jpeg_decode_core.h's jd_step.
        `out`: (blocks, 64) array that takes the coefficients, DC as differences."""
        h, win, nblk, seen = self.h, self.win, 0, 0
        while pos < sub_end:
            w = win[pos]
            dc = zz == 0
            length, symbol = (self.dc if dc else self.ac)[blk]
            peek = w >> 16
            l = length[peek]
            if l == 0:
                if end_bits - pos < 16:
                    return pos, blk, zz, nblk, seen | STOP
                pos, seen = pos + 1, seen | BAD                 # an unassigned code is passed over by one bit
                continue
            sym = symbol[peek]
            size, run = (sym, 0) if dc else (sym & 15, sym >> 4)
            if pos + l + size > end_bits:
                return pos, blk, zz, nblk, seen | STOP
            if size > (11 if dc else 10):
                seen |= BAD
            z = zz
            if not dc and size == 0:
                if run == 15:
                    z += 16
                    if z > 64:
                        z, seen = 64, seen | BAD
                else:
                    if run:
                        seen |= BAD
                    z = 64
            else:
                z += run
                if z > 63:
                    z, seen = 64, seen | BAD                    # the block ends
                else:
                    if size:
                        v = (w >> (32 - l - size)) & ((1 << size) - 1)
                        if v < 1 << (size - 1):
                            v -= (1 << size) - 1
                        if out is not None and block + nblk < block_end:
                            out[block + nblk, z] = v
                    z += 1
            pos += l + size
            if z == 64:
                zz, blk, nblk = 0, (blk + 1) % h.bpm, nblk + 1
            else:
                zz = z
        return pos, blk, zz, nblk, seen


def _finish(h, diff):
    """(blocks, 64) with DC differences -> coef (mcu_rows, mcu_cols, bpm, 64) int16 with DC values (predictors 0 at every interval)."""
    c = diff.reshape(h.total_mcus, h.bpm, 64).copy()
    for k in range(h.n_iv):
        lo, hi = k * h.interval, min((k + 1) * h.interval, h.total_mcus)
        for comp in range(h.ncomp):
            idx = [b for b in range(h.bpm) if h.blk_comp[b] == comp]
            d = c[lo:hi, idx, 0]
            c[lo:hi, idx, 0] = np.cumsum(d.reshape(-1)).reshape(d.shape)
    return np.clip(c, -32768, 32767).astype(np.int16).reshape(h.mcu_rows, h.mcu_cols, h.bpm, 64)


def _interval_blocks(h, k):
    return (min((k + 1) * h.interval, h.total_mcus) - k * h.interval) * h.bpm


def decode_serial(data, stream=None):
    s = stream or Stream(data)
    h = s.h
    diff = np.zeros((h.total_mcus * h.bpm, 64), np.int64)
    for k in range(h.n_iv):
        bit0, end = 8 * s.bounds[k], 8 * s.bounds[k + 1]
        base = k * h.interval * h.bpm
        _, _, _, nblk, rc = s.run(bit0, 0, 0, end, end, diff, base, base + _interval_blocks(h, k))
        if rc & BAD or nblk != _interval_blocks(h, k):
            raise ValueError(f"interval {k}: {nblk} blocks of {_interval_blocks(h, k)}, status {rc}")
    return _finish(h, diff)


def emulate_passes(data, subseq_bits, stream=None):
    """The scheme of sp_jpeg_decode_sync: every interval is cut into subsequences of `subseq_bits`; pass 0 starts every lane at
    its nominal first bit in state (0, 0), pass q starts lane j from lane j - 1's exit of pass q - 1 (a lane whose start did not
    change keeps its record); a record notes whether its walk met something invalid, which the next lane's start does not see; the
    first pass that changes no record ends it.  -> (coef, passes, that last one included)."""
    s = stream or Stream(data)
    h = s.h
    lanes = []                                                  # (interval, j, bit0, end_bits)
    for k in range(h.n_iv):
        bit0, end = 8 * s.bounds[k], 8 * s.bounds[k + 1]
        lanes += [(k, j, bit0, end) for j in range(-(-(end - bit0) // subseq_bits))]

    def walk(lane, pos, st, out=None, block=0, block_end=0):
        k, j, bit0, end = lane
        return s.run(pos, st >> 8, st & 255, min(bit0 + (j + 1) * subseq_bits, end), end, out, block, block_end)

    rec, passes = [None] * len(lanes), 0
    while True:
        new, changed = [], False
        for g, lane in enumerate(lanes):
            k, j, bit0, end = lane
            if j == 0:
                start = (bit0, 0)
            elif passes == 0:
                start = (bit0 + j * subseq_bits, 0)
            else:
                start = rec[g - 1][1]
            if passes and rec[g][0] == start:
                r = rec[g]
            else:
                pos, blk, zz, nblk, rc = walk(lane, *start)
                r = (start, (pos, (blk << 8) | zz), nblk, rc & BAD)
            changed |= passes == 0 or r[1:] != rec[g][1:]
            new.append(r)
        rec, passes = new, passes + 1
        if not changed:
            break
    if any(r[3] for r in rec):
        raise ValueError("an unassigned code, an index past 63 or a size out of range")
    diff = np.zeros((h.total_mcus * h.bpm, 64), np.int64)
    by_interval = [[] for _ in range(h.n_iv)]
    for g, lane in enumerate(lanes):
        by_interval[lane[0]].append(g)
    for k, mine in enumerate(by_interval):
        total = sum(rec[i][2] for i in mine)
        if total != _interval_blocks(h, k):
            raise ValueError(f"interval {k}: {total} blocks of {_interval_blocks(h, k)}")
        base = k * h.interval * h.bpm
        first = base
        for i in mine:
            walk(lanes[i], *rec[i][0], diff, first, base + _interval_blocks(h, k))
            first += rec[i][2]
    return _finish(h, diff), passes


# ------------------------------------------------------------------------------------------------ pixels
def _idct_1d(v, descale):
    """jidctint's butterfly over v[0..7] (arrays); 13-bit constants."""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
    tmp0, tmp1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = 1 << (descale - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return [(o + half) >> descale for o in out]


def idct_blocks(coef, table):
    """coef (..., 64) zigzag, table (64,) natural -> (..., 8, 8) samples 0..255."""
    nat = np.zeros(coef.shape, np.int64)
    nat[..., ZIGZAG] = coef.astype(np.int64)
    b = (nat * table).reshape(*coef.shape[:-1], 8, 8)
    cols = np.stack(_idct_1d([b[..., r, :] for r in range(8)], 11), axis=-2)          # column pass: over the row index
    rows = np.stack(_idct_1d([cols[..., :, c] for c in range(8)], 18), axis=-1)
    v = rows & 1023                                                                    # libjpeg's range table
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896)))


def upsample(c, hs, vs, h, w):
    """A chrominance component at its own size (ceil(h / vs), ceil(w / hs)) -> (h, w): libjpeg's triangle filter."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    if hs == 1:
        return c[:h, :w]
    if cw <= 2:                                                   # libjpeg repeats samples where a row has one or two
        return np.repeat(np.repeat(c, vs, axis=0), 2, axis=1)[:h, :w]
    if vs == 2:
        above, below = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
        s = np.empty((2 * ch, cw), np.int64)
        s[0::2], s[1::2] = 3 * c + above, 3 * c + below
        out = np.empty((2 * ch, 2 * cw), np.int64)
        out[:, 2::2] = (3 * s[:, 1:] + s[:, :-1] + 8) >> 4
        out[:, 1:-1:2] = (3 * s[:, :-1] + s[:, 1:] + 7) >> 4
        out[:, 0], out[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        return out[:h, :w]
    out = np.empty((ch, 2 * cw), np.int64)
    out[:, 2::2] = (3 * c[:, 1:] + c[:, :-1] + 1) >> 2
    out[:, 1:-1:2] = (3 * c[:, :-1] + c[:, 1:] + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out[:h, :w]


def pixels(data, coef=None):
    h = parse(data)
    coef = decode_serial(data) if coef is None else coef
    tables = [h.quant[c[3]] for c in h.comps]
    n = h.hs * h.vs if h.ncomp == 3 else 1
    lum = idct_blocks(coef[:, :, :n], tables[0]).reshape(h.mcu_rows, h.mcu_cols, h.vs, h.hs, 8, 8)
    lum = lum.transpose(0, 2, 4, 1, 3, 5).reshape(h.mcu_rows * h.vs * 8, h.mcu_cols * h.hs * 8)[:h.height, :h.width]
    if h.ncomp == 1:
        return np.repeat(lum[:, :, None], 3, axis=2).astype(np.uint8)
    ch, cw = -(-h.height // h.vs), -(-h.width // h.hs)
    planes = []
    for i in (1, 2):
        p = idct_blocks(coef[:, :, n + i - 1], tables[i]).transpose(0, 2, 1, 3).reshape(h.mcu_rows * 8, h.mcu_cols * 8)
        planes.append(upsample(p[:ch, :cw], h.hs, h.vs, h.height, h.width) - 128)
    cb, cr = planes
    r = lum + ((91881 * cr + 32768) >> 16)
    g = lum + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = lum + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ fixtures of the tests
def _jpeg(frame, **options):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", **options)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (file, subseq_bits): the smallest shapes at which each part of the decoder can go wrong."""
    out = {}
    noise = jpeg_model.noise_frames(1, 48, 64, 11)[0]
    for q in (100, 90, 5):
        for sub, name in ((0, "444"), (1, "422"), (2, "420")):
            out[f"noise48x64_q{q}_{name}"] = (_jpeg(noise, quality=q, subsampling=sub), 1024)
    odd = jpeg_model.noise_frames(1, 37, 51, 12)[0]
    out["noise37x51_420"] = (_jpeg(odd, quality=90, subsampling=2), 1024)
    out["noise37x51_422"] = (_jpeg(odd, quality=90, subsampling=1), 1024)
    out["noise37x51_420_rst1"] = (_jpeg(odd, quality=90, subsampling=2, restart_marker_blocks=1), 1024)
    out["noise37x51_420_rst5"] = (_jpeg(odd, quality=90, subsampling=2, restart_marker_blocks=5), 1024)
    for hh, ww in ((1, 1), (8, 8), (17, 16)):
        out[f"noise{hh}x{ww}_420"] = (_jpeg(jpeg_model.noise_frames(1, hh, ww, 13)[0], quality=90, subsampling=2), 1024)
    scene = jpeg_model.scene_frames(1, 144, 256, 14)[0]
    out["scene144x256_q90"] = (_jpeg(scene, quality=90), 1024)
    out["scene144x256_q90_optimize"] = (_jpeg(scene, quality=90, optimize=True), 1024)
    big = jpeg_model.noise_frames(1, 144, 256, 15)[0]
    out["noise144x256_q90_s1024"] = (_jpeg(big, quality=90), 1024)
    out["noise144x256_q90_s128"] = (out["noise144x256_q90_s1024"][0], 128)
    from PIL import Image

    grey = np.asarray(Image.fromarray(jpeg_model.scene_frames(1, 40, 56, 16)[0]).convert("L"))
    out["grey40x56"] = (_jpeg(grey, quality=90), 1024)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(coef, passes, pixels) of fixture `name` by the model, computed once for all the tests that need it."""
    data, subseq_bits = fixtures()[name]
    stream = Stream(data)
    coef, passes = emulate_passes(data, subseq_bits, stream)
    coef.setflags(write=False)
    px = pixels(data, coef)
    px.setflags(write=False)
    return coef, passes, px


def pillow_pixels(data):
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()
