"""An independent statement of the PNG / APNG path that csrc/png.hip and models/image_io.py implement, for
tests/test_png_cpu.py and tests/test_png_gpu.py: integer numpy and plain Python, written from the PNG specification, RFC 1950,
RFC 1951, the APNG specification and the rules of the row filter and of the strip-parallel deflate stream as the project fixes
them (include/svdpipe.h).  It imports nothing from the package.

    filter_frame(frame)                   -> filtered bytes (h, 1 + 3w) uint8, the tag in column 0
    tokens(data)                          -> the tokens of one strip: ("lit", byte) / ("match", length)
    huffman_lengths(counts, limit)        -> code lengths
    deflate_stream(filtered, strip_rows)  -> (zlib stream of one frame, per-strip records)
    png_file(h, w, stream), apng_file(streams, w, h, fps), walk_png(data)
"""

import heapq
import struct
import zlib
from fractions import Fraction

import numpy as np

from tests.gif_model import noise_frames, scene_frames  # noqa: F401  (the inputs of the tests)

END_OF_BLOCK = 256
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# block header at its largest: BFINAL + BTYPE, HLIT + HDIST + HCLEN, 19 lengths of 3 bits, 286 + 2 code lengths of at most 7 bits
# and 7 extra bits each
HEADER_BITS_MAX = 3 + 14 + 19 * 3 + (286 + 2) * 14
TOKEN_BITS_MAX = 15


# ------------------------------------------------------------------------------------------------ filter
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_frame(frame):
    """(h, w, 3) uint8 -> (h, 1 + 3w) uint8.  Every row takes the filter type with the least sum of min(b, 256 - b) over its
    filtered bytes, the lowest type among equals; the row above is the frame's own (zeros above row 0)."""
    h, w, _ = frame.shape
    rows = frame.reshape(h, 3 * w).astype(np.int64)
    out = np.empty((h, 1 + 3 * w), dtype=np.uint8)
    for y in range(h):
        x = rows[y]
        b = rows[y - 1] if y else np.zeros_like(x)
        a = np.concatenate([np.zeros(3, dtype=np.int64), x[:-3]])
        c = np.concatenate([np.zeros(3, dtype=np.int64), b[:-3]])
        cands = [x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]
        cands = [v & 255 for v in cands]
        scores = [int(np.minimum(v, 256 - v).sum()) for v in cands]
        t = scores.index(min(scores))
        out[y, 0] = t
        out[y, 1:] = cands[t]
    return out


def filter_frames(frames):
    return np.stack([filter_frame(f) for f in frames])


def unfilter(filtered, w):
    """The PNG decoder's side, for the model's own checks."""
    h = filtered.shape[0]
    out = np.zeros((h, 3 * w), dtype=np.int64)
    for y in range(h):
        t, row = int(filtered[y, 0]), filtered[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(3 * w, dtype=np.int64)
        for i in range(3 * w):
            a = out[y, i - 3] if i >= 3 else 0
            b = up[i]
            c = up[i - 3] if i >= 3 else 0
            pred = [0, a, b, (a + b) >> 1, int(_paeth(np.int64(a), np.int64(b), np.int64(c)))][t]
            out[y, i] = (row[i] + pred) & 255
    return out.astype(np.uint8).reshape(h, w, 3)


# ------------------------------------------------------------------------------------------------ tokens
def tokens(data):
    """One strip's bytes -> list of ("lit", byte) / ("match", length); every match is at distance 1."""
    out, p, n = [("lit", data[0])], 1, len(data)
    while p < n:
        r = 0
        while r < 258 and p + r < n and data[p + r] == data[p - 1]:
            r += 1
        if r >= 3:
            out.append(("match", r))
            p += r
        else:
            out.append(("lit", data[p]))
            p += 1
    return out


def tokens_by_runs(data):
    """The same tokens from the runs of equal bytes: per run of n one literal, floor((n - 1) / 258) matches of 258, then the
    remainder as a match if it is at least 3, else as literals."""
    out, p, total = [], 0, len(data)
    while p < total:
        n = 1
        while p + n < total and data[p + n] == data[p]:
            n += 1
        out.append(("lit", data[p]))
        out += [("match", 258)] * ((n - 1) // 258)
        rem = (n - 1) % 258
        out += [("match", rem)] if rem >= 3 else [("lit", data[p])] * rem
        p += n
    return out


def length_symbol(length):
    """-> (symbol, extra bits, extra value)"""
    i = max(k for k in range(29) if LENGTH_BASE[k] <= length)
    return 257 + i, LENGTH_EXTRA[i], length - LENGTH_BASE[i]


# ------------------------------------------------------------------------------------------------ codes
def huffman_depths(counts):
    """Plain Huffman over the non-zero counts: the two least nodes are joined until one is left; nodes are ordered by weight,
    then by age: leaves, in order of (count, symbol), are older than every joined node, joined nodes age in order of their
    making.  -> depth per symbol (0 for unused)."""
    leaves = sorted((c, s) for s, c in enumerate(counts) if c)
    heap = [(c, age, s) for age, (c, s) in enumerate(leaves)]
    heapq.heapify(heap)
    parent, age = {}, len(leaves)
    while len(heap) > 1:
        wa, _, a = heapq.heappop(heap)
        wb, _, b = heapq.heappop(heap)
        node = ("node", age)
        parent[a] = parent[b] = node
        heapq.heappush(heap, (wa + wb, age, node))
        age += 1
    depths = [0] * len(counts)
    for _, s in leaves:
        d, at = 0, s
        while at in parent:
            at, d = parent[at], d + 1
        depths[s] = d
    return depths


def huffman_lengths(counts, limit):
    """-> (lengths, number of halvings).  Fewer than two symbols in use: the lowest unused ones get count 1.  While a length
    passes `limit`, every non-zero count becomes (f + 1) >> 1 and the tree is made again."""
    counts = list(counts)
    while sum(1 for c in counts if c) < 2:
        counts[next(s for s, c in enumerate(counts) if not c)] = 1
    halvings = 0
    while True:
        depths = huffman_depths(counts)
        if max(depths) <= limit:
            return depths, halvings
        counts = [(c + 1) >> 1 if c else 0 for c in counts]
        halvings += 1


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> code per symbol, most significant bit first."""
    bl_count = [0] * 17
    for n in lengths:
        bl_count[n] += 1
    bl_count[0] = 0
    code, next_code = 0, [0] * 17
    for bits in range(1, 17):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            codes[s] = next_code[n]
            next_code[n] += 1
    return codes


def run_length_form(lengths):
    """zlib's scan of one code's lengths -> list of (symbol 0..18, extra bits, extra value)."""
    out, prev, count = [], -1, 0
    nxt = lengths[0]
    max_count, min_count = (138, 3) if nxt == 0 else (7, 4)
    for n in range(len(lengths)):
        cur, nxt = nxt, (lengths[n + 1] if n + 1 < len(lengths) else -1)
        count += 1
        if count < max_count and cur == nxt:
            continue
        if count < min_count:
            out += [(cur, 0, 0)] * count
        elif cur != 0:
            if cur != prev:
                out.append((cur, 0, 0))
                count -= 1
            out.append((16, 2, count - 3))
        elif count <= 10:
            out.append((17, 3, count - 3))
        else:
            out.append((18, 7, count - 11))
        count, prev = 0, cur
        max_count, min_count = (138, 3) if nxt == 0 else ((6, 3) if cur == nxt else (7, 4))
    return out


class _Bits:
    """Deflate's packing: least significant bit first; Huffman codes go in most significant bit first."""

    def __init__(self):
        self.done, self.acc, self.held, self.n = bytearray(), 0, 0, 0

    def put(self, value, width):
        self.acc |= value << self.held
        self.held += width
        self.n += width
        while self.held >= 8:
            self.done.append(self.acc & 255)
            self.acc >>= 8
            self.held -= 8

    def put_code(self, code, width):
        self.put(int(format(code, f"0{width}b")[::-1], 2) if width else 0, width)

    def bytes(self):
        return bytes(self.done) + (bytes([self.acc]) if self.held else b"")


def deflate_block(data, final, bits):
    """One strip as one dynamic-Huffman block into `bits`; -> dict of what the tests want to see."""
    toks = tokens(data)
    counts = [0] * 286
    for kind, v in toks:
        counts[v if kind == "lit" else length_symbol(v)[0]] += 1
    counts[END_OF_BLOCK] = 1
    lengths, halvings = huffman_lengths(counts, 15)
    codes = canonical_codes(lengths)
    nlit = max(s for s in range(286) if lengths[s]) + 1                    # >= 257: end-of-block is in use
    dist_lengths = [1, 1]                                                  # the constant distance code: 0 -> '0', 1 -> '1'
    seq = run_length_form(lengths[:nlit]) + run_length_form(dist_lengths)
    cl_counts = [0] * 19
    for s, _, _ in seq:
        cl_counts[s] += 1
    cl_lengths, _ = huffman_lengths(cl_counts, 7)
    cl_codes = canonical_codes(cl_lengths)
    ncl = max(i for i in range(19) if cl_lengths[CL_ORDER[i]]) + 1
    ncl = max(ncl, 4)
    start = bits.n
    bits.put(1 if final else 0, 1)
    bits.put(2, 2)
    bits.put(nlit - 257, 5)
    bits.put(len(dist_lengths) - 1, 5)
    bits.put(ncl - 4, 4)
    for i in range(ncl):
        bits.put(cl_lengths[CL_ORDER[i]], 3)
    for s, nbits, value in seq:
        bits.put_code(cl_codes[s], cl_lengths[s])
        bits.put(value, nbits)
    header = bits.n - start
    for kind, v in toks:
        if kind == "lit":
            bits.put_code(codes[v], lengths[v])
        else:
            s, nbits, value = length_symbol(v)
            bits.put_code(codes[s], lengths[s])
            bits.put(value, nbits)
            bits.put_code(0, 1)                                            # distance 1
    bits.put_code(codes[END_OF_BLOCK], lengths[END_OF_BLOCK])
    return {"start_bit": start, "bits": bits.n - start, "header_bits": header, "tokens": toks, "lengths": lengths,
            "halvings": halvings, "literals": sorted({v for k, v in toks if k == "lit"}),
            "matches": [v for k, v in toks if k == "match"]}


def adler32(data):
    a, b = 1, 0
    for v in data:
        a = (a + v) % 65521
        b = (b + a) % 65521
    return (b << 16) | a


def deflate_stream(filtered, strip_rows):
    """(h, 1 + 3w) uint8 -> (78 9C, the strips' blocks joined bit by bit, zero padding, Adler-32; one record per strip)."""
    h = filtered.shape[0]
    bits, strips = _Bits(), []
    for top in range(0, h, strip_rows):
        data = filtered[top:top + strip_rows].reshape(-1).tolist()
        strips.append(deflate_block(data, top + strip_rows >= h, bits))
    whole = filtered.tobytes()
    return b"\x78\x9c" + bits.bytes() + struct.pack(">I", zlib.adler32(whole)), strips


def stream_bound(h, w, strip_rows):
    """The header's derivation of sp_png_stream_bytes."""
    rows = min(strip_rows, h)
    strips = -(-h // rows)
    bits = strips * (HEADER_BITS_MAX + TOKEN_BITS_MAX) + TOKEN_BITS_MAX * h * (1 + 3 * w)
    return 2 + -(-bits // 8) + 4


# ------------------------------------------------------------------------------------------------ the files
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def ihdr(h, w):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))


def png_file(h, w, stream):
    return SIGNATURE + ihdr(h, w) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


def apng_file(streams, w, h, fps):
    delay = (1 / Fraction(fps)).limit_denominator(65535)
    out, seq = [SIGNATURE, ihdr(h, w), chunk(b"acTL", struct.pack(">II", len(streams), 0))], 0
    for i, s in enumerate(streams):
        out.append(chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, delay.numerator, delay.denominator, 0, 0)))
        seq += 1
        if i == 0:
            out.append(chunk(b"IDAT", s))
        else:
            out.append(chunk(b"fdAT", struct.pack(">I", seq) + s))
            seq += 1
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def walk_png(data):
    """Parse strictly: the signature, then chunks with right CRCs up to IEND as the last bytes -> list of (kind, payload)."""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while True:
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        assert len(payload) == n and struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload), kind
        out.append((kind, payload))
        at += 12 + n
        if kind == b"IEND":
            assert at == len(data), "bytes after IEND"
            return out


# ------------------------------------------------------------------------------------------------ inputs of the tests
def ramps(h=8, w=40):
    """(4, h, w, 3): a horizontal ramp, a vertical ramp, a diagonal ramp, and noise."""
    y, x = np.mgrid[0:h, 0:w]
    hor = np.stack([(5 * x) % 256, (3 * x + 7) % 256, (7 * x + 1) % 256], axis=-1)
    ver = np.stack([(5 * y + 3) % 256, (9 * y) % 256, (11 * y + 2) % 256], axis=-1)
    # a step every other pixel: the value left of x is the one above-left of it, so Average / Paeth beat Sub and Up
    dia = np.stack([(6 * (x + y)) % 256, (4 * (x + y) + 9) % 256, (10 * (x + y)) % 256], axis=-1)
    out = np.stack([hor, ver, dia, noise_frames(1, h, w, 77)[0]]).astype(np.uint8)
    return out


def fibonacci_row(total=4201):
    """One row of `total` bytes (a 1 x (total - 1) / 3 frame's filtered row, tag 0 in front) in which the counts of the byte
    values follow a Fibonacci series, no two equal bytes adjacent: the unlimited Huffman code is deeper than 15."""
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= total - 1:
        fib.append(fib[-1] + fib[-2])
    values = []
    for i, c in enumerate(fib[2:]):                                       # (the tag and end-of-block are the series' 1, 1)
        values += [i + 1] * c
    values += [len(fib) - 2] * (total - 1 - len(values))                      # the rest goes to the most frequent value
    # the most frequent value first on the even places, then the odd ones: no value takes more than half, so no two meet
    order = sorted(values, key=lambda v: (-values.count(v), v))
    out = np.zeros(len(order), dtype=np.uint8)
    out[0::2] = order[:len(out[0::2])]
    out[1::2] = order[len(out[0::2]):]
    assert not np.any(out[1:] == out[:-1]) and out[0] != 0
    return np.concatenate([[0], out]).astype(np.uint8)
