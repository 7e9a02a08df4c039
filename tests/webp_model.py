"""An independent statement of the lossless / animated WebP path that csrc/webp.hip and models/image_io.py implement, for
tests/test_webp_cpu.py and tests/test_webp_gpu.py: integer numpy and plain Python, written from the WebP lossless bitstream
specification, the WebP container specification and the encoder's rules as the project fixes them (include/svdpipe.h).  It
imports nothing from the package; the Huffman construction, the canonical codes, the run-length form of code lengths and the
bit packer are those of tests/png_model.py (the two formats share them).

    subtract_green_costs(frame)           -> (cost with green taken out, cost of the plain form)
    transform(frame, pred_bits)           -> (flag, modes (bh, bw) uint8, residual (h, w, 4) uint8 in byte order B G R A)
    tokens(pixels)                        -> the tokens of one strip: ("lit", pixel) / ("copy", length)
    encode_residual(...), encode_frame(frame, pred_bits, group_bits) -> the VP8L stream, records
    stream_bound(h, w, pred_bits, group_bits)
    webp_file(stream), webp_animation(streams, w, h, fps), walk_webp(data)
"""

import struct

import numpy as np

from tests.png_model import (_Bits, canonical_codes, huffman_lengths, noise_frames, run_length_form,  # noqa: F401
                             scene_frames)

CL_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
ALPHABETS = (280, 256, 256, 256, 40)            # green + lengths, red, blue, alpha, distance
MAX_COPY = 4096
MIN_COPY = 3
# a normal code's header at its largest: the form bit, the count of 19-symbol lengths, 19 lengths of 3 bits, the max_symbol
# bit, and per code length a run-length symbol of at most 7 bits with at most 7 extra bits
def _normal_bits(alphabet):
    return 1 + 4 + 19 * 3 + 1 + alphabet * 14


SIMPLE_1BIT, SIMPLE_8BIT = 4, 11
GROUP_HEADER_MAX = _normal_bits(280) + 2 * _normal_bits(256) + 2 * SIMPLE_1BIT        # alpha is always 0, distance 0 or 1
SUB_HEADER_MAX = _normal_bits(280) + _normal_bits(256) + SIMPLE_1BIT + SIMPLE_8BIT + SIMPLE_1BIT
MAIN_PIXEL_BITS_MAX = 45
SUB_PIXEL_BITS_MAX = 30


# ------------------------------------------------------------------------------------------------ inputs of the tests
def correlated_frame(h=144, w=256, seed=5):
    """The green of scene_frames(1, h, w, seed)[0] with R = clip(g + 20 + n), B = clip(g - 15 + n), n uniform in [-2, 2]:
    channels that follow each other, as a real picture's do."""
    g = scene_frames(1, h, w, seed=seed)[0][:, :, 1].astype(np.int32)
    rng = np.random.default_rng(1)
    r = np.clip(g + 20 + rng.integers(-2, 3, g.shape), 0, 255)
    b = np.clip(g - 15 + rng.integers(-2, 3, g.shape), 0, 255)
    return np.stack([r, g, b], 2).astype(np.uint8)


def every_mode_frame(pred_bits=2, seed=11):
    """One frame whose blocks are built pixel by pixel so that, for block k, predictor 1 + k % 13 reproduces it exactly from
    the pixels before it plus a noise of +-1 on one pixel: the tests check that every mode 1..13 is chosen somewhere."""
    bs = 1 << pred_bits
    by, bx = 6, 13
    h, w = bs * by + 1, bs * bx + 1
    rng = np.random.default_rng(seed)
    px = np.zeros((h, w, 3), dtype=np.int64)                              # R G B
    px[0] = rng.integers(0, 256, (w, 3))
    px[:, 0] = rng.integers(0, 256, (h, 3))
    flat = px.reshape(-1, 3)
    for y in range(1, h):
        for x in range(1, w):
            mode = 1 + (((y - 1) // bs) * bx + (x - 1) // bs) % 13
            p = y * w + x
            flat[p] = _predict(mode, flat[p - 1], flat[p - w], flat[p - w - 1], flat[p - w + 1])
            if (x + y) % 3 == 0:                                          # keep the neighbourhood from going flat
                flat[p] = (flat[p] + rng.integers(-40, 41, 3)) % 256
    return flat.reshape(h, w, 3).astype(np.uint8)


def fibonacci_values(terms=19):
    """10945 byte values (11 x 995) whose counts are the Fibonacci series 1, 1, 2, 3, ... of `terms` terms, no two equal values
    adjacent: the unlimited Huffman code of their histogram is deeper than 15."""
    fib = [1, 1]
    while len(fib) < terms:
        fib.append(fib[-1] + fib[-2])
    values = [v for v, c in enumerate(fib) for _ in range(c)]
    # the most frequent value first on the even places, then the odd ones: no value takes more than half, so no two meet
    order = sorted(values, key=lambda v: (-fib[v], v))
    out = np.zeros(len(order), dtype=np.uint8)
    out[0::2] = order[:len(out[0::2])]
    out[1::2] = order[len(out[0::2]):]
    assert not np.any(out[1:] == out[:-1])
    return out


# ------------------------------------------------------------------------------------------------ transforms
def _cost(v):
    v = np.asarray(v) & 255
    return np.minimum(v, 256 - v)


def subtract_green_costs(frame):
    """-> (with green taken out, plain): the sum over the frame of min(d, 256 - d) of the left-neighbour differences of the R
    and B bytes."""
    f = frame.astype(np.int64)
    out = []
    for sub in (True, False):
        rb = f[:, :, [0, 2]] - (f[:, :, 1:2] if sub else 0)
        out.append(int(_cost(rb[:, 1:] - rb[:, :-1]).sum()))
    return tuple(out)


def _avg(a, b):
    return (a + b) >> 1


def _predict(mode, L, T, TL, TR):
    """The format's 14 predictors on the R, G, B channels of one pixel (alpha is 255 everywhere and predicts itself)."""
    L, T, TL, TR = (np.asarray(v, dtype=np.int64) for v in (L, T, TL, TR))
    if mode == 0:
        return np.zeros(3, dtype=np.int64)
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:
        return L if int(np.abs(T - TL).sum()) < int(np.abs(L - TL).sum()) else T
    if mode == 12:
        return np.clip(L + T - TL, 0, 255)
    a = _avg(L, T)
    d = a - TL
    half = np.where(d >= 0, d >> 1, -((-d) >> 1))                         # C's division: toward zero
    return np.clip(a + half, 0, 255)


def _predict_all(flat, w):
    """(14, h*w, 3) predictions of every pixel by every mode from the flat neighbours p-1, p-w, p-w-1, p-w+1 (so the top-right
    neighbour of a row's last pixel is the first pixel of the current row); edge pixels are overruled by the caller."""
    n = flat.shape[0]
    idx = np.arange(n)

    def at(off):
        return flat[np.clip(idx - off, 0, n - 1)]
    L, T, TL, TR = at(1), at(w), at(w + 1), at(w - 1)
    P = np.zeros((14, n, 3), dtype=np.int64)
    P[1], P[2], P[3], P[4] = L, T, TR, TL
    P[5] = _avg(_avg(L, TR), T)
    P[6], P[7], P[8], P[9] = _avg(L, TL), _avg(L, T), _avg(TL, T), _avg(T, TR)
    P[10] = _avg(_avg(L, TL), _avg(T, TR))
    P[11] = np.where((np.abs(T - TL).sum(1) < np.abs(L - TL).sum(1))[:, None], L, T)
    P[12] = np.clip(L + T - TL, 0, 255)
    a = _avg(L, T)
    d = a - TL
    P[13] = np.clip(a + np.where(d >= 0, d >> 1, -((-d) >> 1)), 0, 255)
    return P, L, T


def transform(frame, pred_bits):
    """(h, w, 3) uint8 RGB -> (subtract-green flag, modes (bh, bw) uint8, residual (h, w, 4) uint8 as B, G, R, A with A = 0)."""
    h, w, _ = frame.shape
    with_green, plain = subtract_green_costs(frame)
    flag = 1 if with_green < plain else 0                                  # ties take the plain form
    px = frame.astype(np.int64)
    if flag:
        px = np.stack([(px[:, :, 0] - px[:, :, 1]) & 255, px[:, :, 1], (px[:, :, 2] - px[:, :, 1]) & 255], 2)
    flat = px.reshape(-1, 3)
    P, L, T = _predict_all(flat, w)
    res = (flat[None] - P) & 255                                           # (14, h*w, 3)
    cost = _cost(res).sum(2).reshape(14, h, w)
    cost[:, 0, :] = 0                                                      # the edges' residuals do not depend on the mode
    cost[:, :, 0] = 0
    bs = 1 << pred_bits
    bh, bw = -(-h // bs), -(-w // bs)
    modes = np.zeros((bh, bw), dtype=np.uint8)
    for by in range(bh):
        for bx in range(bw):
            sums = cost[:, by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs].reshape(14, -1).sum(1)
            modes[by, bx] = int(np.argmin(sums))                           # the lowest mode among equals
    full = np.repeat(np.repeat(modes, bs, 0), bs, 1)[:h, :w].reshape(-1)
    pred = P[full, np.arange(h * w)].reshape(h, w, 3)
    pred[0, :] = L.reshape(h, w, 3)[0, :]
    pred[:, 0] = T.reshape(h, w, 3)[:, 0]
    pred[0, 0] = 0                                                         # 0xff000000
    r = (px - pred) & 255
    residual = np.zeros((h, w, 4), dtype=np.uint8)
    residual[:, :, 0], residual[:, :, 1], residual[:, :, 2] = r[:, :, 2], r[:, :, 1], r[:, :, 0]
    return flag, modes, residual


def untransform(flag, modes, residual, pred_bits):
    """The decoder's side, for the model's own checks."""
    h, w, _ = residual.shape
    out = np.zeros((h * w, 3), dtype=np.int64)
    r = residual.reshape(-1, 4).astype(np.int64)[:, [2, 1, 0]]
    for p in range(h * w):
        y, x = divmod(p, w)
        if p == 0:
            pred = np.zeros(3, dtype=np.int64)
        elif y == 0:
            pred = out[p - 1]
        elif x == 0:
            pred = out[p - w]
        else:
            pred = _predict(int(modes[y >> pred_bits, x >> pred_bits]), out[p - 1], out[p - w], out[p - w - 1], out[p - w + 1])
        out[p] = (r[p] + pred) & 255
    if flag:
        out[:, 0] = (out[:, 0] + out[:, 1]) & 255
        out[:, 2] = (out[:, 2] + out[:, 1]) & 255
    return out.reshape(h, w, 3).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ tokens
def tokens(pixels):
    """One strip's pixels (32-bit ARGB values) -> list of ("lit", pixel) / ("copy", length); every copy is at distance 1."""
    out, p, n = [("lit", pixels[0])], 1, len(pixels)
    while p < n:
        r = 0
        while r < MAX_COPY and p + r < n and pixels[p + r] == pixels[p - 1]:
            r += 1
        if r >= MIN_COPY:
            out.append(("copy", r))
            p += r
        else:
            out.append(("lit", pixels[p]))
            p += 1
    return out


def prefix_symbol(value):
    """The format's prefix coding of a length or distance code >= 1 -> (symbol, extra bits, extra value)."""
    d = value - 1
    if d < 4:
        return d, 0, 0
    hb = d.bit_length() - 1
    extra = hb - 1
    return 2 * hb + ((d >> extra) & 1), extra, d & ((1 << extra) - 1)


def histograms(toks):
    counts = [[0] * a for a in ALPHABETS]
    for kind, v in toks:
        if kind == "lit":
            counts[0][(v >> 8) & 255] += 1
            counts[1][(v >> 16) & 255] += 1
            counts[2][v & 255] += 1
            counts[3][v >> 24] += 1
        else:
            counts[0][256 + prefix_symbol(v)[0]] += 1
            counts[4][1] += 1                                              # distance 1 is plane code 2: prefix symbol 1
    return counts


# ------------------------------------------------------------------------------------------------ codes
def write_code(bits, counts):
    """One prefix code into `bits` -> (lengths, codes, record).  Fewer than two symbols in use and that symbol below 256: the
    simple form with one symbol (zero bits per use).  Else a normal code."""
    used = [s for s, c in enumerate(counts) if c]
    if len(used) < 2 and (not used or used[0] < 256):
        s = used[0] if used else 0
        bits.put(1, 1)
        bits.put(0, 1)
        if s < 2:
            bits.put(0, 1)
            bits.put(s, 1)
        else:
            bits.put(1, 1)
            bits.put(s, 8)
        return [0] * len(counts), [0] * len(counts), {"simple": True, "halvings": 0}
    lengths, halvings = huffman_lengths(counts, 15)
    codes = canonical_codes(lengths)
    seq = run_length_form(lengths)
    cl_counts = [0] * 19
    for s, _, _ in seq:
        cl_counts[s] += 1
    cl_lengths, _ = huffman_lengths(cl_counts, 7)
    cl_codes = canonical_codes(cl_lengths)
    ncl = max(4, max(i for i in range(19) if cl_lengths[CL_ORDER[i]]) + 1)
    bits.put(0, 1)
    bits.put(ncl - 4, 4)
    for i in range(ncl):
        bits.put(cl_lengths[CL_ORDER[i]], 3)
    bits.put(0, 1)                                                         # max_symbol: the whole alphabet
    for s, nbits, value in seq:
        bits.put_code(cl_codes[s], cl_lengths[s])
        bits.put(value, nbits)
    return lengths, codes, {"simple": False, "halvings": halvings, "lengths": lengths}


def write_codes(bits, toks):
    return [write_code(bits, c) for c in histograms(toks)]


def write_tokens(bits, toks, codes):
    (lg, cg, _), (lr, cr, _), (lb, cb, _), (la, ca, _), (ld, cd, _) = codes
    for kind, v in toks:
        if kind == "lit":
            g, r, b, a = (v >> 8) & 255, (v >> 16) & 255, v & 255, v >> 24
            bits.put_code(cg[g], lg[g])
            bits.put_code(cr[r], lr[r])
            bits.put_code(cb[b], lb[b])
            bits.put_code(ca[a], la[a])
        else:
            s, nbits, value = prefix_symbol(v)
            bits.put_code(cg[256 + s], lg[256 + s])
            bits.put(value, nbits)
            bits.put_code(cd[1], ld[1])


def write_sub_image(bits, pixels):
    """An entropy-coded sub-image with one code set: no colour cache, the five codes, the pixels."""
    toks = tokens(pixels)
    bits.put(0, 1)
    codes = write_codes(bits, toks)
    write_tokens(bits, toks, codes)
    return toks, codes


# ------------------------------------------------------------------------------------------------ the stream
def encode_residual(h, w, flag, modes, residual, pred_bits, group_bits):
    """-> (the VP8L stream from the signature byte on, records).  residual: (h, w, 4) uint8 B, G, R, A; A is coded as 0."""
    assert 1 <= h <= 16384 and 1 <= w <= 16384 and h * w <= 1 << 24
    assert 2 <= pred_bits <= 9 and (group_bits == 0 or 2 <= group_bits <= 9)
    bits = _Bits()
    bits.put(0x2F, 8)
    bits.put(w - 1, 14)
    bits.put(h - 1, 14)
    bits.put(0, 1)
    bits.put(0, 3)
    if flag:
        bits.put(1, 1)
        bits.put(2, 2)
    bits.put(1, 1)
    bits.put(0, 2)
    bits.put(pred_bits - 2, 3)
    mode_pixels = [0xFF000000 | (int(m) << 8) for m in np.asarray(modes).reshape(-1)]
    mode_toks, mode_codes = write_sub_image(bits, mode_pixels)
    seg0 = bits.n
    bits.put(0, 1)                                                         # no more transforms
    bits.put(0, 1)                                                         # no colour cache
    pixels = (np.ascontiguousarray(residual).view("<u4").reshape(-1) & 0x00FFFFFF).tolist()
    if group_bits:
        rows = 1 << group_bits
        groups, across = -(-h // rows), -(-w // rows)
        bits.put(1, 1)
        bits.put(group_bits - 2, 3)
        write_sub_image(bits, [0xFF000000 | ((g >> 8) << 16) | ((g & 255) << 8) for g in range(groups) for _ in range(across)])
    else:
        rows, groups = h, 1
        bits.put(0, 1)
    seg1 = bits.n
    strips = []
    for g in range(groups):
        toks = tokens(pixels[g * rows * w:min(h, (g + 1) * rows) * w])
        start = bits.n
        codes = write_codes(bits, toks)
        strips.append({"tokens": toks, "codes": codes, "header_bits": bits.n - start})
    for s in strips:
        start = bits.n
        write_tokens(bits, s["tokens"], s["codes"])
        s["pixel_bits"] = bits.n - start
    return bits.bytes(), {"strips": strips, "seg0_bits": seg0, "seg1_bits": seg1 - seg0, "mode_tokens": mode_toks, "bits": bits.n}


def encode_frame(frame, pred_bits, group_bits):
    flag, modes, residual = transform(frame, pred_bits)
    stream, rec = encode_residual(frame.shape[0], frame.shape[1], flag, modes, residual, pred_bits, group_bits)
    rec.update(flag=flag, modes=modes, residual=residual)
    return stream, rec


def stream_bound(h, w, pred_bits, group_bits):
    """The header's derivation of sp_webp_stream_bytes."""
    bs = 1 << pred_bits
    bits = 40 + 3 + 6 + 1 + SUB_HEADER_MAX + SUB_PIXEL_BITS_MAX * (-(-h // bs)) * (-(-w // bs))
    bits += 3
    groups = 1
    if group_bits:
        rows = 1 << group_bits
        groups = -(-h // rows)
        bits += 3 + 1 + SUB_HEADER_MAX + SUB_PIXEL_BITS_MAX * groups * (-(-w // rows))
    bits += groups * GROUP_HEADER_MAX + MAIN_PIXEL_BITS_MAX * h * w
    return -(-bits // 8)


# ------------------------------------------------------------------------------------------------ the files
def chunk(kind, payload):
    return kind + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _u24(v):
    assert 0 <= v < 1 << 24
    return struct.pack("<I", v)[:3]


def _riff(body):
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


def webp_file(stream):
    return _riff(chunk(b"VP8L", stream))


def webp_animation(streams, w, h, fps):
    ms = round(1000 / fps)
    body = chunk(b"VP8X", bytes([0x02, 0, 0, 0]) + _u24(w - 1) + _u24(h - 1))
    body += chunk(b"ANIM", struct.pack("<IH", 0, 0))
    for s in streams:
        body += chunk(b"ANMF", _u24(0) + _u24(0) + _u24(w - 1) + _u24(h - 1) + _u24(ms) + bytes([0x02]) + chunk(b"VP8L", s))
    return _riff(body)


def walk_webp(data):
    """Parse strictly: RIFF with the right size, WEBP, then chunks with even padding up to the last byte -> list of
    (kind, payload); an ANMF's payload is (its 16 header bytes, the chunks inside)."""
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8 and len(data) % 2 == 0

    def walk(buf):
        at, out = 0, []
        while at < len(buf):
            kind, n = buf[at:at + 4], struct.unpack("<I", buf[at + 4:at + 8])[0]
            payload = buf[at + 8:at + 8 + n]
            assert len(payload) == n, kind
            at += 8 + n
            if n & 1:
                assert buf[at:at + 1] == b"\0", "odd payload without its padding byte"
                at += 1
            out.append((kind, (payload[:16], walk(payload[16:])) if kind == b"ANMF" else payload))
        assert at == len(buf)
        return out
    return walk(data[12:])
