"""An independent statement of the animated-GIF path that csrc/gif.hip and models/image_io.py implement, for
tests/test_gif_cpu.py and tests/test_gif_gpu.py: integer numpy and plain Python, written from the GIF89a specification and
from the rules of the quantiser and of the strip-parallel LZW stream as the project fixes them.  It imports nothing from the
package.

    quantise(frame)                      -> (palette (256, 3) uint8, indices (h, w) uint8, boxes in use)
    lzw_image_data(indices, strip_rows)  -> (image data of one image block, per-strip records)
    gif_file(palettes, datas, w, h, fps) -> the file
    walk_gif(data)                       -> blocks, palettes and de-sub-blocked data, parsed strictly
"""

import struct

import numpy as np

CLEAR, EOI, FIRST_FREE, TABLE_END = 256, 257, 258, 4096


# ------------------------------------------------------------------------------------------------ quantiser
def histogram(frame):
    """(h, w, 3) uint8 -> (count (32, 32, 32), sums (32, 32, 32, 3)) int64 over the bins (r >> 3, g >> 3, b >> 3)."""
    px = frame.reshape(-1, 3).astype(np.int64)
    b = ((px[:, 0] >> 3) << 10) | ((px[:, 1] >> 3) << 5) | (px[:, 2] >> 3)
    count = np.bincount(b, minlength=32768)
    sums = np.stack([np.bincount(b, weights=px[:, c], minlength=32768).astype(np.int64) for c in range(3)], axis=-1)
    return count.reshape(32, 32, 32), sums.reshape(32, 32, 32, 3)


def _sub(a, lo, hi):
    return a[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]


def _shrunk(count, lo, hi):
    """The box (lo, hi), inclusive, drawn in to the occupied bins inside it."""
    sub = _sub(count, lo, hi)
    new_lo, new_hi = [], []
    for axis in range(3):
        occupied = np.nonzero(sub.sum(axis=tuple(a for a in range(3) if a != axis)))[0]
        new_lo.append(lo[axis] + int(occupied[0]))
        new_hi.append(lo[axis] + int(occupied[-1]))
    return new_lo, new_hi


def boxes_of(count):
    """The list of (lo, hi, pixels) after the splits."""
    lo, hi = _shrunk(count, [0, 0, 0], [31, 31, 31])
    boxes = [(lo, hi, int(count.sum()))]
    while len(boxes) < 256:
        best, best_score = None, 0
        for i, (lo, hi, pixels) in enumerate(boxes):
            e = max(h - l for l, h in zip(lo, hi))
            if e > 0 and pixels * e > best_score:                       # (strictly greater: a tie stays with the lower index)
                best, best_score = i, pixels * e
        if best is None:
            break
        lo, hi, pixels = boxes[best]
        extents = [h - l for l, h in zip(lo, hi)]
        e = max(extents)
        axis = extents.index(e)
        planes = _sub(count, lo, hi).sum(axis=tuple(a for a in range(3) if a != axis))
        running = np.cumsum(planes)
        c = min(int(np.nonzero(2 * running >= pixels)[0][0]), e - 1)
        lower_hi, upper_lo = list(hi), list(lo)
        lower_hi[axis], upper_lo[axis] = lo[axis] + c, lo[axis] + c + 1
        boxes[best] = (*_shrunk(count, lo, lower_hi), int(running[c]))
        boxes.append((*_shrunk(count, upper_lo, hi), pixels - int(running[c])))
    return boxes


def quantise(frame):
    """(h, w, 3) uint8 -> (palette (256, 3) uint8, indices (h, w) uint8, number of palette entries in use)."""
    count, sums = histogram(frame)
    boxes = boxes_of(count)
    palette = np.zeros((256, 3), dtype=np.int64)
    for i, (lo, hi, pixels) in enumerate(boxes):
        s = _sub(sums, lo, hi).reshape(-1, 3).sum(axis=0)
        palette[i] = (2 * s + pixels) // (2 * pixels)
    occupied = np.nonzero(count.reshape(-1))[0]
    n = count.reshape(-1)[occupied][:, None]
    mean = (2 * sums.reshape(-1, 3)[occupied] + n) // (2 * n)
    dist = ((mean[:, None, :] - palette[None, :len(boxes), :]) ** 2).sum(axis=-1)
    table = np.zeros(32768, dtype=np.uint8)
    table[occupied] = np.argmin(dist, axis=1)                           # (the first of equal minima: the lowest index)
    px = frame.astype(np.int64)
    bins = ((px[..., 0] >> 3) << 10) | ((px[..., 1] >> 3) << 5) | (px[..., 2] >> 3)
    return palette.astype(np.uint8), table[bins], len(boxes)


def quantise_frames(frames):
    """(n, h, w, 3) -> (palettes (n, 256, 3), indices (n, h, w), boxes in use per frame)."""
    res = [quantise(f) for f in frames]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), [r[2] for r in res]


# ------------------------------------------------------------------------------------------------ LZW
class _Codes:
    """Codes packed least significant bit first."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, width):
        self.acc |= code << self.n
        self.n += width

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _strip(pixels, bits, end_code):
    """Code one strip with a dictionary of its own into `bits`; -> (codes written without the end code, next free code at the
    end, counting the last code's own entry)."""
    table, free, width, codes = {}, FIRST_FREE, 9, 0
    prefix = pixels[0]
    for k in pixels[1:]:
        found = table.get((prefix, k))
        if found is not None:
            prefix = found
            continue
        bits.put(prefix, width)
        codes += 1
        table[(prefix, k)] = free
        free += 1
        if free > (1 << width):                                         # the decoder, one entry behind, reads the next code wider
            width += 1
        if free == TABLE_END:
            bits.put(CLEAR, 12)
            table, free, width = {}, FIRST_FREE, 9
        prefix = k
    bits.put(prefix, width)
    codes += 1
    free += 1                                                           # the entry the decoder makes of the last code
    if free > (1 << width):
        width += 1
    bits.put(end_code, width)
    return codes, free


def sub_blocks(data):
    return b"".join(bytes([len(data[i:i + 255])]) + data[i:i + 255] for i in range(0, len(data), 255)) + b"\0"


def lzw_image_data(indices, strip_rows):
    """(h, w) uint8 indices -> (the image data of a GIF image block: 08, the sub-blocks, 00; one record per strip:
    dict(start_bit, bits, codes, free))."""
    h, _ = indices.shape
    bits, strips = _Codes(), []
    bits.put(CLEAR, 9)
    for top in range(0, h, strip_rows):
        start = bits.n
        last = top + strip_rows >= h
        codes, free = _strip(indices[top:top + strip_rows].reshape(-1).tolist(), bits, EOI if last else CLEAR)
        strips.append({"start_bit": start, "bits": bits.n - start, "codes": codes, "free": free})
    return b"\x08" + sub_blocks(bits.bytes()), strips


def lzw_decode(data):
    """De-sub-blocked LZW data at minimum code size 8 -> list of indices; strict: every code must be known, the stream must end
    with EOI and only zero bits may follow it."""
    acc, n = int.from_bytes(data, "little"), 8 * len(data)
    at, width, free, out = 0, 9, FIRST_FREE, []
    table, prev = {}, None
    while True:
        assert at + width <= n, "the data ends before EOI"
        code = (acc >> at) & ((1 << width) - 1)
        at += width
        if code == CLEAR:
            table, free, width, prev = {}, FIRST_FREE, 9, None
            continue
        if code == EOI:
            break
        if code < 256:
            entry = [code]
        elif code in table:
            entry = table[code]
        else:
            assert code == free and prev is not None, f"code {code} is not in the table"
            entry = prev + [prev[0]]
        out.extend(entry)
        if prev is not None and free < TABLE_END:
            table[free] = prev + [entry[0]]
            free += 1
            if free == (1 << width) and width < 12:
                width += 1
        prev = entry
    assert acc >> at == 0 and n - at < 8, "bits after EOI"
    return out


# ------------------------------------------------------------------------------------------------ the file
def gif_file(palettes, datas, width, height, fps):
    """GIF89a, no global table, NETSCAPE2.0 loop for ever, per frame a graphic control extension, an image descriptor with a
    256-entry local table, the table and the image data."""
    delay = max(1, round(100 / fps))
    out = [b"GIF89a", struct.pack("<HHBBB", width, height, 0x70, 0, 0), b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"]
    for palette, data in zip(palettes, datas):
        out.append(b"\x21\xf9\x04" + struct.pack("<BHB", 0, delay, 0) + b"\x00")
        out.append(b"\x2c" + struct.pack("<HHHHB", 0, 0, width, height, 0x87))
        out.append(np.asarray(palette, dtype=np.uint8).reshape(256, 3).tobytes())
        out.append(bytes(data))
    out.append(b"\x3b")
    return b"".join(out)


def walk_gif(data):
    """Parse a GIF strictly: every block must be one this path writes, and the trailer must be the last byte.  -> dict with
    `size`, `screen` (packed, background, aspect), `loop` (None without the extension), `frames`: list of dict(delay,
    disposal, rect, palette (k, 3) uint8, min_code, data (sub-blocks joined), block_lengths)."""
    assert data[:6] == b"GIF89a"
    w, h, packed, background, aspect = struct.unpack("<HHBBB", data[6:13])
    assert not packed & 0x80, "a global colour table"
    at, res, control = 13, {"size": (w, h), "screen": (packed, background, aspect), "loop": None, "frames": []}, None

    def blocks(at):
        parts, lengths = [], []
        while data[at]:
            lengths.append(data[at])
            parts.append(data[at + 1:at + 1 + data[at]])
            assert len(parts[-1]) == data[at], "a sub-block crosses the end of the file"
            at += 1 + data[at]
        return b"".join(parts), lengths, at + 1

    while True:
        kind = data[at]
        if kind == 0x3B:
            assert at == len(data) - 1, "bytes after the trailer"
            return res
        if kind == 0x21 and data[at + 1] == 0xFF:
            assert data[at + 2] == 11 and data[at + 3:at + 14] == b"NETSCAPE2.0"
            body, lengths, at = blocks(at + 14)
            assert lengths == [3] and body[0] == 1
            res["loop"] = struct.unpack("<H", body[1:3])[0]
        elif kind == 0x21 and data[at + 1] == 0xF9:
            assert data[at + 2] == 4 and data[at + 7] == 0
            flags, delay, _ = struct.unpack("<BHB", data[at + 3:at + 7])
            control, at = (flags, delay), at + 8
        elif kind == 0x2C:
            assert control is not None, "an image without a graphic control extension"
            left, top, iw, ih, flags = struct.unpack("<HHHHB", data[at + 1:at + 10])
            assert flags & 0x80 and not flags & 0x40, "no local table, or interlaced"
            k = 2 << (flags & 7)
            palette = np.frombuffer(data[at + 10:at + 10 + 3 * k], dtype=np.uint8).reshape(k, 3)
            at += 10 + 3 * k
            min_code = data[at]
            body, lengths, at = blocks(at + 1)
            assert all(n == 255 for n in lengths[:-1]) and lengths, "a short sub-block before the last"
            res["frames"].append({"delay": control[1], "disposal": (control[0] >> 2) & 7, "rect": (left, top, iw, ih),
                                  "palette": palette, "min_code": min_code, "data": body, "block_lengths": lengths})
            control = None
        else:
            raise AssertionError(f"unexpected block {kind:#x} at {at}")


# ------------------------------------------------------------------------------------------------ inputs of the tests
def noise_frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def scene_frames(n, h, w, seed):
    """A smooth two-sinusoid colour field that moves from frame to frame, plus sigma = 8 noise (tests/jpeg_model.py has the
    same field)."""
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


def noise_indices(h, w, seed, levels=256):
    return np.random.default_rng(seed).integers(0, levels, (h, w), dtype=np.uint8)


def strip_ending_at(free, rows=2):
    """(indices (rows, w), for strip_rows 1): uniform noise whose first strip -- one row, so CLEAR follows it -- ends with the
    next free code at exactly `free`, its own last entry counted.  Found with the model alone: a longer prefix of one noise
    row never takes fewer codes and takes at most one more per pixel, so the shortest prefix with free - 258 codes has exactly
    that many, and no dictionary has filled before."""
    want = free - FIRST_FREE
    row = noise_indices(1, 2 * want, 7000)
    lo, hi = want, 2 * want                                             # (a code covers at least one pixel)
    while lo < hi:
        mid = (lo + hi) // 2
        if lzw_image_data(row[:, :mid], 1)[1][0]["codes"] >= want:
            hi = mid
        else:
            lo = mid + 1
    idx = np.concatenate([row[:, :lo], noise_indices(rows - 1, lo, 7001)])
    assert lzw_image_data(idx, 1)[1][0]["free"] == free
    return idx


def frame_with_whole_blocks(h=6, strip_rows=2):
    """Noise indices whose LZW data is a whole number of 255-byte sub-blocks (a search over widths and seeds)."""
    for w in range(40, 400):
        for seed in range(4):
            idx = noise_indices(h, w, 9000 + seed, levels=64)
            data, strips = lzw_image_data(idx, strip_rows)
            if (strips[-1]["start_bit"] + strips[-1]["bits"] + 7) // 8 % 255 == 0:
                return idx
    raise AssertionError("no width gives a whole number of sub-blocks")
