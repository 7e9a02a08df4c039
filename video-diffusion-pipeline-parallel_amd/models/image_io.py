"""Picture in, 8-bit frames out: the host-side image handling of the reference's demo
(``/root/reference/scripts/generate_video_demo.py``) around the edge stages of ``edge_stages.py``.

  * ``ImageFrontEnd``: ``load_and_preprocess_image`` (ref ``:71-89``: Lanczos cover-resize + centre crop) followed by what
    ``encode_image`` does to the cropped picture before the two encoders run (ref ``:108-126``: the ``CLIPImageProcessor``
    -- bicubic shortest-edge resize, centre crop, rescale, normalise -- and ``ToTensor`` + ``Normalize([0.5], [0.5])``), on
    the device with the kernels of ``csrc/image.hip``.  Pillow's resize is reproduced to within one 8-bit level (its
    weights are 22-bit fixed point, the kernel's fp32); the geometry rules below are the reference's exactly.
  * ``frames_to_uint8`` / ``save_frames``: ``save_video`` / ``save_gif`` (ref ``:198-222``) without imageio.
  * ``JpegEncoder`` / ``jpeg_header`` / ``write_avi``: the video file of ``save_video`` as Motion-JPEG in an AVI container
    (no ffmpeg): frames on the device are compressed there by the kernels of ``csrc/jpeg.hip`` and only the compressed
    bytes come to the host; the marker segments and the RIFF container are written here.
  * ``GifEncoder`` / ``write_gif``: the animated GIF of ``save_gif``: frames on the device are quantised to a palette each
    and LZW-coded there by the kernels of ``csrc/gif.hip``; the blocks of the file around them are written here.
  * ``PngEncoder`` / ``png_file`` / ``write_apng``: the lossless frames (a directory or a ``%03d.png`` pattern) and an
    animated PNG: frames on the device are filtered and deflated there by the kernels of ``csrc/png.hip``, and so are
    signature, chunks and their CRC-32 (``csrc/crc32.hip``); ``png_file`` / ``write_apng`` build the same files here.
  * ``WebpEncoder`` / ``webp_file`` / ``write_webp``: lossless WebP stills and one animated WebP, full colour and playable
    in a browser: frames on the device become VP8L bitstreams there by the kernels of ``csrc/webp.hip``; the RIFF container
    has no checksum, so the host only wraps bytes.
  * ``FrameInterpolator``: frames between the frames (2x or 4x the frame rate) before any of the writers above: block motion
    search on luma, a vector median and an overlapped blend by the kernels of ``csrc/interp.hip``, integer arithmetic only.
  * ``load_image``: the decode half of ``load_and_preprocess_image`` (Pillow; a file format is host work).
  * ``parse_jpeg`` / ``JpegDecoder`` / ``load_image_device``: the same decode for the common baseline JPEG on the device: the
    host walks the markers, the compressed bytes are uploaded, and the kernels of ``csrc/jpeg_decode.hip`` go from the
    entropy-coded segment to (H, W, 3) uint8 RGB, which the front end takes as it is.
"""

from __future__ import annotations

import os
import struct
import zlib
from fractions import Fraction

import numpy as np
import torch

from ..hip import ops
from . import common

# image_mean / image_std of the CLIPImageProcessor (the OpenAI CLIP constants: every SVD feature_extractor config has them)
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def cover_geometry(src_h: int, src_w: int, height: int, width: int) -> tuple[int, int, int, int]:
    """``(new_h, new_w, top, left)`` of the reference's cover rule (ref ``:76-88``): scale so that the picture covers the
    target, Python ``round`` (half to even), crop the centre."""
    scale = max(width / src_w, height / src_h)
    new_w, new_h = round(src_w * scale), round(src_h * scale)
    return new_h, new_w, (new_h - height) // 2, (new_w - width) // 2


def clip_geometry(h: int, w: int, size: int) -> tuple[int, int, int, int]:
    """``(new_h, new_w, top, left)`` of the CLIP processor: the shortest edge becomes ``size``, the other
    ``int(size * long / short)`` (transformers ``get_resize_output_image_size``, ``default_to_square=False``), then the
    centre ``size`` x ``size`` crop."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_h, new_w = (new_long, new_short) if w <= h else (new_short, new_long)
    return new_h, new_w, (new_h - size) // 2, (new_w - size) // 2


class ImageFrontEnd:
    """uint8 picture -> ``(pixel_values, image_tensor, cropped_u8)``, the first two as ``edge_stages.encode_image`` takes them.

    Every call only enqueues kernels on the current stream (plus the upload of a host picture); scratch is cached per
    size, the three results are fresh tensors."""

    def __init__(self, device, height: int = 576, width: int = 1024, clip_size: int | None = None, clip_mean=None,
                 clip_std=None) -> None:
        from .clip_hip import CLIPVisionSpec

        self.device = common.hip_device(device, "ImageFrontEnd")
        if height <= 0 or width <= 0:
            raise ValueError("height and width must be positive")
        self.height, self.width = int(height), int(width)
        self.clip_size = int(clip_size if clip_size is not None else CLIPVisionSpec().image_size)
        self.clip_mean = tuple(float(v) for v in (clip_mean if clip_mean is not None else OPENAI_CLIP_MEAN))
        self.clip_std = tuple(float(v) for v in (clip_std if clip_std is not None else OPENAI_CLIP_STD))
        self._scratch: dict = {}

    def _buf(self, name: str, nbytes_or_shape) -> torch.Tensor:
        key = (name, nbytes_or_shape)
        if key not in self._scratch:
            self._scratch[key] = torch.empty(nbytes_or_shape, dtype=torch.uint8, device=self.device)
        return self._scratch[key]

    def _resize(self, src: torch.Tensor, new_h: int, new_w: int, filt: int, name: str) -> torch.Tensor:
        dst = self._buf(name, (new_h, new_w, 3))
        tmp = self._buf(name + ".tmp", ops.image_resample_tmp_bytes(src.shape[0], new_w))
        return ops.image_resample_u8(src, dst, tmp, filter=filt)

    def __call__(self, image_u8) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``image_u8``: (H, W, 3) uint8 tensor or ndarray, any size and layout.  Returns ``pixel_values``
        (1, 3, clip_size, clip_size) fp16, ``image_tensor`` (1, 3, height, width) fp16 in [-1, 1] and the cropped picture
        (height, width, 3) uint8 they were made from."""
        if isinstance(image_u8, np.ndarray):
            image_u8 = np.ascontiguousarray(image_u8)                 # (a flipped view has strides torch refuses)
        img = torch.as_tensor(image_u8)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or img.shape[0] == 0 or img.shape[1] == 0:
            raise ValueError(f"image must be a uint8 (H, W, 3) array; got {img.dtype} {tuple(img.shape)}")
        img = img.to(self.device, non_blocking=True).contiguous()
        src_h, src_w = img.shape[0], img.shape[1]
        h, w, cs = self.height, self.width, self.clip_size
        new_h, new_w, top, left = cover_geometry(src_h, src_w, h, w)
        if new_h < h or new_w < w:
            raise ValueError(f"a {src_h}x{src_w} picture does not cover {h}x{w} after the cover-resize ({new_h}x{new_w})")
        if (new_h, new_w) != (src_h, src_w):
            img = self._resize(img, new_h, new_w, ops.FILTER_LANCZOS3, "cover")
        crop = img[top:top + h, left:left + w]                        # pointer + pitch: no crop kernel
        image_tensor = torch.empty((1, 3, h, w), dtype=torch.float16, device=self.device)
        ops.image_to_tensor(crop, image_tensor, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
        # the CLIP processor starts from the CROPPED picture (ref :110 passes the image load_and_preprocess_image returned)
        ch, cw, ctop, cleft = clip_geometry(h, w, cs)
        small = crop if (ch, cw) == (h, w) else self._resize(crop, ch, cw, ops.FILTER_BICUBIC, "clip")
        pixel_values = torch.empty((1, 3, cs, cs), dtype=torch.float16, device=self.device)
        ops.image_to_tensor(small[ctop:ctop + cs, cleft:cleft + cs], pixel_values, mean=self.clip_mean, std=self.clip_std)
        return pixel_values, image_tensor, crop.clone(memory_format=torch.contiguous_format)


def frames_to_uint8(frames: torch.Tensor) -> torch.Tensor:
    """(B, 3, F, H, W) fp16 / fp32 frames in [-1, 1] -> (B, F, H, W, 3) uint8 on the same device, the conversion of the
    reference's ``save_video`` (ref ``:205``): ``((x + 1) / 2 * 255).clamp(0, 255).to(torch.uint8)`` (truncation)."""
    out = torch.empty((frames.shape[0], frames.shape[2], frames.shape[3], frames.shape[4], 3), dtype=torch.uint8,
                      device=frames.device)
    return ops.frames_to_u8(frames.contiguous(), out)


def load_image(path: str) -> np.ndarray:
    """Decode a picture file to (H, W, 3) uint8 RGB (ref ``:75``: ``Image.open(path).convert("RGB")``)."""
    from PIL import Image

    with Image.open(path) as im:
        return np.asarray(im.convert("RGB")).copy()


def _zigzag() -> list[int]:
    """Position k of the zigzag sequence -> natural (row-major) index of the 8x8 block."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return order


def _check_quality(quality) -> int:
    if not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"quality must be an integer from 1 to 100; got {quality!r}")
    return int(quality)


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(height: int, width: int, quality: int, restart_mcus: int) -> bytes:
    """The fixed front of every frame ``JpegEncoder`` makes, SOI up to and including SOS: JFIF APP0, the two quantisation
    tables (``sp_jpeg_quant_tables``, written in zigzag order), SOF0 (baseline, 8 bit, three components sampled 2x2, 1x1,
    1x1), the four Annex K Huffman tables (``sp_jpeg_huffman_table``), DRI and SOS.  The entropy-coded segment and EOI
    follow it."""
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError(f"a JPEG frame is 1..65535 pixels on a side; got {height}x{width}")
    if not 1 <= restart_mcus <= 65535:
        raise ValueError(f"restart_mcus must be 1..65535; got {restart_mcus}")
    luma, chroma = ops.jpeg_quant_tables(_check_quality(quality))
    zz = _zigzag()
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for tq, table in ((0, luma), (1, chroma)):
        out.append(_segment(0xDB, bytes([tq]) + bytes(table[i] for i in zz)))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for which, tc_th in ((0, 0x00), (2, 0x10), (1, 0x01), (3, 0x11)):
        bits, vals = ops.jpeg_huffman_table(which)
        out.append(_segment(0xC4, bytes([tc_th]) + bits + vals))
    out.append(_segment(0xDD, struct.pack(">H", restart_mcus)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


class _FrameEncoder:
    """What the encoders of (F, H, W, 3) uint8 frames share: device and frame size, scratch kept per name and shape, the
    check of the frames, the copy of the used bytes, and the call that waits for them."""

    def __init__(self, device, height: int, width: int) -> None:
        self.device = common.hip_device(device, type(self).__name__)
        self.height, self.width = int(height), int(width)
        self._scratch: dict = {}

    def _buf(self, name: str, shape, dtype) -> torch.Tensor:
        key = (name, shape)
        if key not in self._scratch:
            self._scratch[key] = torch.empty(shape, dtype=dtype, device=self.device)
        return self._scratch[key]

    def _check_frames(self, frames_u8) -> int:
        """The count of frames, or ``ValueError`` for anything but a (F, height, width, 3) uint8 tensor with F > 0."""
        if (not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4
                or tuple(frames_u8.shape[1:]) != (self.height, self.width, 3) or frames_u8.shape[0] == 0):
            raise ValueError(f"frames must be a (F, {self.height}, {self.width}, 3) uint8 tensor; got "
                             f"{getattr(frames_u8, 'dtype', type(frames_u8))} {tuple(getattr(frames_u8, 'shape', ()))}")
        return frames_u8.shape[0]

    @staticmethod
    def _used_rows(out: torch.Tensor, lens: torch.Tensor) -> list[bytes]:
        """Row i of ``out`` up to ``lens[i]``: the lengths come to the host in one copy, then only the used bytes."""
        return [out[i, :n].cpu().numpy().tobytes() for i, n in enumerate(lens.cpu().tolist())]

    def _finished(self, enqueue, collect, *args):
        """``collect`` of what ``enqueue(*args)`` returned, once the current stream has done the work."""
        bufs = enqueue(*args)
        torch.cuda.current_stream(self.device).synchronize()
        return collect(*bufs)


class JpegEncoder(_FrameEncoder):
    """(F, H, W, 3) uint8 frames on the device -> one baseline JPEG (4:2:0) per frame, compressed on the device.

    ``restart_mcus`` (default: one MCU row) is the restart interval: intervals are coded concurrently.  Coefficient, stream,
    length and scratch buffers are kept per frame count; the stream buffer holds ``sp_jpeg_stream_bytes`` per frame (the size
    no input can exceed), of which only the used bytes are ever copied to the host."""

    def __init__(self, device, height: int, width: int, quality: int = 90, restart_mcus: int | None = None) -> None:
        super().__init__(device, height, width)
        self.quality = _check_quality(quality)
        self.mcu_rows, self.mcu_cols = ops.jpeg_mcu_grid(self.height, self.width)
        self.restart_mcus = int(restart_mcus) if restart_mcus is not None else min(self.mcu_cols, 65535)
        self.header = jpeg_header(self.height, self.width, self.quality, self.restart_mcus)
        self.cap = ops.jpeg_stream_bytes(self.height, self.width, self.restart_mcus)

    def enqueue(self, frames_u8: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Run the two stages on the current stream and return ``(streams (F, cap) uint8, lengths (F,) int32)``: views of
        this encoder's buffers, valid until the next call with as many frames."""
        n = self._check_frames(frames_u8)
        coef = self._buf("coef", (n, self.mcu_rows, self.mcu_cols, 6, 64), torch.int16)
        out = self._buf("stream", (n, self.cap), torch.uint8)
        lens = self._buf("len", (n,), torch.int32)
        ws = self._buf("ws", (ops.jpeg_entropy_ws_bytes(n, self.mcu_rows, self.mcu_cols, self.restart_mcus),), torch.uint8)
        ops.jpeg_dct_quant(frames_u8.to(self.device).contiguous(), coef, quality=self.quality)
        ops.jpeg_entropy(coef, out, lens, ws, restart_mcus=self.restart_mcus)
        return out, lens

    def collect(self, out: torch.Tensor, lens: torch.Tensor) -> list[bytes]:
        """The files of an ``enqueue`` whose work has finished: the lengths come to the host first, then only the used bytes."""
        return [self.header + s + b"\xff\xd9" for s in self._used_rows(out, lens)]

    def encode(self, frames_u8: torch.Tensor) -> list[bytes]:
        return self._finished(self.enqueue, self.collect, frames_u8)


class UnsupportedJpeg(ValueError):
    """A well-formed JPEG that the device decoder does not take (the message names the cause); Pillow decodes it."""


class JpegInfo:
    """What ``parse_jpeg`` reads out of the marker segments of a baseline JPEG."""

    __slots__ = ("width", "height", "components", "hs", "vs", "tq", "td", "ta", "quant", "dht", "restart_interval",
                 "segment_offset", "segment_length")

    def __init__(self, **kw) -> None:
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def plan_fields(self, subseq_bits: int) -> list[int]:
        pad = lambda t: list(t) + [0] * (3 - len(t))                      # noqa: E731
        return [self.width, self.height, self.components, self.hs, self.vs, self.restart_interval, self.segment_length,
                int(subseq_bits)] + pad(self.tq) + pad(self.td) + pad(self.ta)

    def plan_tables(self) -> tuple[bytes, int, bytes, bytes, int]:
        """``(quant 4 x 64, have_quant, bits 4 x 16, vals 4 x 256, have_huff)`` as ``ops.jpeg_decode_plan`` takes them."""
        quant, bits, vals, have_q, have_h = bytearray(256), bytearray(64), bytearray(1024), 0, 0
        for tq, table in self.quant.items():
            quant[64 * tq:64 * tq + 64] = bytes(table)
            have_q |= 1 << tq
        for (tc, th), (b, v) in self.dht.items():
            slot = 2 * tc + th
            bits[16 * slot:16 * slot + 16] = b
            vals[256 * slot:256 * slot + len(v)] = v
            have_h |= 1 << slot
        return bytes(quant), have_q, bytes(bits), bytes(vals), have_h


_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic-coded sequential",
              0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless", 0xCD: "arithmetic-coded differential",
              0xCE: "arithmetic-coded differential progressive", 0xCF: "arithmetic-coded differential lossless"}


def parse_jpeg(data) -> JpegInfo:
    """The marker walk of a JPEG file, SOI up to SOS: size, sampling, table selectors, quantisation tables (natural order), the
    DHT specifications ``(bits16, vals)``, the restart interval, and offset and length of the entropy-coded segment, which runs
    from behind SOS to the last EOI of the file (to the file's end without one).  No entropy-coded byte is read.
    ``UnsupportedJpeg`` names what is outside the device decoder's scope (SOF0, 8 bit, one component or YCbCr 4:4:4 / 4:2:2 /
    4:2:0, one interleaved scan); ``ValueError`` reports a malformed header."""
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file: no SOI marker at its start")
    zz = _zigzag()
    quant, dht, frame, restart, jfif, adobe = {}, {}, None, 0, False, None
    at = 2
    while True:
        if at + 2 > len(data):
            raise ValueError("truncated JPEG header: the file ends before SOS")
        if data[at] != 0xFF:
            raise ValueError(f"malformed JPEG header: byte {data[at]:#04x} at offset {at} where a marker should start")
        while at + 1 < len(data) and data[at + 1] == 0xFF:              # fill bytes
            at += 1
        marker = data[at + 1]
        at += 2
        if marker == 0x01 or 0xD0 <= marker <= 0xD7:
            continue
        if marker in (0xD8, 0xD9):
            raise ValueError(f"malformed JPEG header: marker {marker:#04x} before SOS")
        if at + 2 > len(data):
            raise ValueError("truncated JPEG header: the file ends inside a marker segment")
        length = struct.unpack(">H", data[at:at + 2])[0]
        if length < 2 or at + length > len(data):
            raise ValueError(f"malformed JPEG header: the segment of marker {marker:#04x} at offset {at - 2} has a length past the end")
        body = data[at + 2:at + length]
        if marker == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise UnsupportedJpeg("16-bit quantisation table")
                if tq > 3 or k + 65 > len(body):
                    raise ValueError("malformed DQT segment")
                table = np.zeros(64, np.uint8)
                table[zz] = np.frombuffer(body[k + 1:k + 65], np.uint8)
                if not table.all():
                    raise ValueError("malformed DQT segment: a zero divisor")
                quant[tq] = table
                k += 65
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    raise ValueError("malformed DHT segment")
                tc, th = body[k] >> 4, body[k] & 15
                bits = body[k + 1:k + 17]
                n = sum(bits)
                if tc > 1 or th > 3 or n > 256 or k + 17 + n > len(body):
                    raise ValueError("malformed DHT segment")
                if th > 1:
                    raise UnsupportedJpeg("Huffman table selector above 1 (not baseline)")
                dht[(tc, th)] = (bits, body[k + 17:k + 17 + n])
                k += 17 + n
        elif marker == 0xC0:
            if frame is not None:
                raise ValueError("malformed JPEG header: two frame headers")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("malformed SOF0 segment")
            precision, height, width, nf = struct.unpack(">BHHB", body[:6])
            if precision != 8:
                raise UnsupportedJpeg(f"{precision}-bit samples")
            if width == 0 or height == 0:
                raise ValueError("malformed SOF0 segment: zero size")
            frame = (width, height, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)])
        elif marker in _SOF_NAMES:
            raise UnsupportedJpeg(f"{_SOF_NAMES[marker]} JPEG (SOF{marker - 0xC0})")
        elif marker == 0xDC:
            raise UnsupportedJpeg("DNL segment")
        elif marker == 0xDD:
            if len(body) != 2:
                raise ValueError("malformed DRI segment")
            restart = struct.unpack(">H", body)[0]
        elif marker == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif marker == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif marker == 0xDA:
            break
        at += length
    if frame is None:
        raise ValueError("malformed JPEG header: SOS before a frame header")
    width, height, comps = frame
    if len(comps) == 4:
        raise UnsupportedJpeg("four components (CMYK / YCCK)")
    if len(comps) not in (1, 3):
        raise UnsupportedJpeg(f"{len(comps)} components")
    ns = body[0] if body else 0
    if len(body) != 4 + 2 * ns:
        raise ValueError("malformed SOS segment")
    if ns != len(comps):
        raise UnsupportedJpeg("more than one scan (the first holds not all components)")
    if [body[1 + 2 * i] for i in range(ns)] != [c[0] for c in comps]:
        raise UnsupportedJpeg("the scan's components are not in the frame's order")
    ss, se, ahal = body[1 + 2 * ns:4 + 2 * ns]
    if (ss, se, ahal) != (0, 63, 0):
        raise UnsupportedJpeg(f"spectral selection / successive approximation in a scan (Ss={ss}, Se={se}, Ah/Al={ahal:#04x})")
    if len(comps) == 3:
        if not jfif and (adobe == 0 or (adobe is None and [c[0] for c in comps] == [82, 71, 66])):
            raise UnsupportedJpeg("three components that are RGB, not YCbCr (Adobe transform 0)")
        if adobe == 2 and not jfif:
            raise UnsupportedJpeg("Adobe transform 2 (YCCK)")
        hs, vs = comps[0][1], comps[0][2]
        if any((c[1], c[2]) != (1, 1) for c in comps[1:]) or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
            raise UnsupportedJpeg("sampling factors " + ", ".join(f"{c[1]}x{c[2]}" for c in comps)
                                  + " (chrominance must be 1x1, luminance 1x1, 2x1 or 2x2)")
    else:
        hs, vs = 1, 1
        if (comps[0][1], comps[0][2]) != (1, 1):
            raise UnsupportedJpeg(f"one component sampled {comps[0][1]}x{comps[0][2]}")
    tq = tuple(c[3] for c in comps)
    td = tuple(body[2 + 2 * i] >> 4 for i in range(ns))
    ta = tuple(body[2 + 2 * i] & 15 for i in range(ns))
    if any(t > 1 for t in td + ta):
        raise UnsupportedJpeg("Huffman table selector above 1 (not baseline)")
    if not quant or not dht:
        raise ValueError("malformed JPEG header: a missing table (no " + ("DQT" if not quant else "DHT") + " segment before SOS)")
    for c in range(ns):
        if tq[c] not in quant or (0, td[c]) not in dht or (1, ta[c]) not in dht:
            raise ValueError(f"malformed JPEG header: component {c} selects a table that is not defined (a table selector without its table)")
    start = at + length
    end = data.rfind(b"\xff\xd9")
    if end < start:
        end = len(data)
    if end <= start:
        raise ValueError("truncated JPEG: no entropy-coded data behind SOS")
    return JpegInfo(width=width, height=height, components=len(comps), hs=hs, vs=vs, tq=tq, td=td, ta=ta, quant=quant, dht=dht,
                    restart_interval=restart, segment_offset=start, segment_length=end - start)


# the largest count of passes seen over the fixtures of tests/test_jpeg_decode_cpu.py plus 2 (profiles/jpeg_decode_parity.txt)
JPEG_SYNC_PASSES = 51

_JPEG_ERRORS = ((1, "a 0xFF in the coded data that neither 0x00 nor RSTn follows"), (2, "restart markers out of order"),
                (4, "the number of restart markers does not fit the restart interval"),
                (8, "an unassigned Huffman code, a coefficient index past 63 or a size category out of range"),
                (16, "a restart interval whose blocks do not come to its MCUs"))


class JpegDecoder:
    """A baseline JPEG file in host memory -> (H, W, 3) uint8 RGB on the device, decoded there (``csrc/jpeg_decode.hip``).

    Only the compressed bytes are uploaded, behind the plan ``parse_jpeg``'s fields become.  Every restart interval (the whole
    scan in a file without DRI) is cut into subsequences of ``subseq_bits`` bits, one lane each; the lanes synchronise in
    passes, and ``sync_passes`` of them are enqueued at a time: ``decode`` reads the status block once behind them and
    enqueues further rounds only where the fixed point was not reached, so the result never depends on ``sync_passes``.
    ``last_passes`` is the count of passes the last picture took (the one that found nothing changed included),
    ``last_coef`` its coefficients (a view of this decoder's buffer, valid until the next call)."""

    def __init__(self, device, subseq_bits: int = 1024, sync_passes: int = JPEG_SYNC_PASSES) -> None:
        self.device = common.hip_device(device, "JpegDecoder")
        if isinstance(subseq_bits, bool) or not isinstance(subseq_bits, (int, np.integer)) or subseq_bits < 32 or subseq_bits % 32:
            raise ValueError(f"subseq_bits must be a multiple of 32, at least 32; got {subseq_bits!r}")
        if isinstance(sync_passes, bool) or not isinstance(sync_passes, (int, np.integer)) or not 1 <= sync_passes <= 4096:
            raise ValueError(f"sync_passes must be an integer in 1..4096; got {sync_passes!r}")
        self.subseq_bits, self.sync_passes = int(subseq_bits), int(sync_passes)
        self.last_passes, self.last_coef, self.last_status, self.last_info = 0, None, None, None
        self._scratch: dict = {}
        self._job = None

    def _buf(self, name: str, nbytes: int, dtype=torch.uint8) -> torch.Tensor:
        key = (name, nbytes, dtype)
        if key not in self._scratch:
            self._scratch = {k: v for k, v in self._scratch.items() if k[0] != name}      # one buffer per name: pictures differ in size
            self._scratch[key] = torch.empty(nbytes // torch.empty((), dtype=dtype).element_size(), dtype=dtype, device=self.device)
        return self._scratch[key]

    def _round(self, first_pass: int) -> None:
        plan, ws, coef, rgb = self._job[:4]
        ops.jpeg_decode_sync(plan, ws, first_pass, self.sync_passes)
        ops.jpeg_decode_coefficients(plan, ws, first_pass + self.sync_passes - 1, coef)
        ops.jpeg_decode_pixels(plan, ws, coef, rgb)
        self._job[4] = first_pass + self.sync_passes

    def enqueue(self, data) -> torch.Tensor:
        """Parse, upload, and enqueue the four stages with one round of passes on the current stream.  Returns the (H, W, 3)
        uint8 tensor the picture is written to; whether it was is known only to ``finish`` (``decode`` = ``enqueue`` + ``finish``)."""
        data = bytes(data)
        info = parse_jpeg(data)
        plan_host = ops.jpeg_decode_plan(info.plan_fields(self.subseq_bits), *info.plan_tables())
        blob = bytearray(plan_host) + data[info.segment_offset:info.segment_offset + info.segment_length]
        up = torch.frombuffer(blob, dtype=torch.uint8).to(self.device, non_blocking=True)
        plan = ops.JpegPlan(plan_host, up[:len(plan_host)])
        ws = self._buf("ws", plan.ws_bytes)
        coef = self._buf("coef", plan.coef_bytes, torch.int16)
        rgb = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=self.device)
        self._job = [plan, ws, coef, rgb, 0, up]
        self.last_info = info
        ops.jpeg_decode_split(plan, up[len(plan_host):], ws)
        self._round(0)
        return rgb

    def finish(self) -> torch.Tensor:
        """Read the status block of the picture enqueued last (this waits for the stream), enqueue further rounds of passes while
        the fixed point is not reached, and return the picture.  ``ValueError`` where the status block reports an error."""
        if self._job is None:
            raise RuntimeError("JpegDecoder.finish: nothing was enqueued")
        plan, ws, coef, rgb = self._job[:4]
        while True:
            st = ws[:256].view(torch.int32).cpu().tolist()
            self.last_status, self.last_passes = st, st[2]
            if st[0]:
                self._job = None
                raise ValueError("JpegDecoder: broken entropy-coded segment: " + "; ".join(m for b, m in _JPEG_ERRORS if st[0] & b))
            if st[10]:
                break
            if self._job[4] > st[6] + 1:
                done, self._job = self._job[4], None
                raise RuntimeError(f"JpegDecoder: no fixed point after {done} passes over {st[6]} subsequences")
            self._round(self._job[4])
        info = self.last_info
        mcu_cols, mcu_rows = -(-info.width // (8 * info.hs)), -(-info.height // (8 * info.vs))
        self.last_coef = coef.view(mcu_rows, mcu_cols, 1 if info.components == 1 else info.hs * info.vs + 2, 64)
        self._job = None
        return rgb

    def decode(self, data) -> torch.Tensor:
        self.enqueue(data)
        return self.finish()


def load_image_device(path: str, device) -> torch.Tensor:
    """A picture file -> (H, W, 3) uint8 RGB on ``device``: a JPEG that ``parse_jpeg`` accepts is decoded there from its
    compressed bytes (``JpegDecoder``); every other file is decoded by Pillow (``load_image``) and uploaded."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:2] == b"\xff\xd8":
        try:
            parse_jpeg(data)
        except ValueError:                                            # UnsupportedJpeg too: Pillow's file, and Pillow's message
            pass
        else:
            return JpegDecoder(device).decode(data)
    return torch.from_numpy(load_image(path)).to(common.hip_device(device, "load_image_device"))


def _pillow_bytes(frame: np.ndarray, format: str, **options) -> bytes:
    """Pillow's encode of one frame in host memory, for arrays that never were on a GPU."""
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format=format, **options)
    return buf.getvalue()


def _write(path: str, data: bytes) -> None:
    with open(path, "wb") as fh:
        fh.write(data)


def _write_numbered(pattern: str, count: int, datas) -> list[str]:
    """``datas`` (an iterable of ``count`` files' bytes) to ``pattern % 0 ..``; the names."""
    files = [pattern % i for i in range(count)]
    for name, data in zip(files, datas):
        _write(name, data)
    return files


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


AVI_MAX_BYTES = 2 ** 31 - 1          # one RIFF chunk of an AVI 1.0 file (OpenDML extends it; not written here)


def write_avi(path: str, jpegs: list[bytes], width: int, height: int, fps: int) -> None:
    """Motion-JPEG in a plain AVI 1.0 file: ``RIFF 'AVI '`` { ``LIST 'hdrl'`` { ``avih``, ``LIST 'strl'`` { ``strh``
    (``vids`` / ``MJPG``, scale 1, rate ``fps``), ``strf`` (BITMAPINFOHEADER, ``MJPG``, 24 bit) } }, ``LIST 'movi'`` { one
    ``00dc`` chunk per frame, padded to even length }, ``idx1`` { one key-frame entry per chunk, offsets from the ``movi``
    fourcc } }.  Every frame is a complete JPEG file."""
    if not jpegs:
        raise ValueError("write_avi: no frames")
    if not isinstance(fps, (int, np.integer)) or fps <= 0:
        raise ValueError("fps must be a positive integer")
    if width <= 0 or height <= 0:
        raise ValueError("width and height must be positive")
    n, largest = len(jpegs), max(len(j) for j in jpegs)
    movi_bytes = 4 + sum(8 + len(j) + (len(j) & 1) for j in jpegs)
    total = 12 + (8 + 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))) + (8 + movi_bytes) + (8 + 16 * n)
    if total > AVI_MAX_BYTES:
        raise ValueError(f"'{path}': {total} bytes pass the 2 GiB of an AVI 1.0 file (OpenDML is not written)")
    avih = struct.pack("<14I", 1000000 // int(fps), largest * int(fps), 0, 0x10, n, 0, 1, largest, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIHHHH", b"vids", b"MJPG", 0, 0, 0, 0, 1, int(fps), 0, n, largest, 0xFFFFFFFF, 0,
                       0, 0, min(width, 65535), min(height, 65535))
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
    movi, index, at = [b"movi"], [], 4
    for j in jpegs:
        index.append(struct.pack("<4sIII", b"00dc", 0x10, at, len(j)))
        movi.append(_chunk(b"00dc", j))
        at += len(movi[-1])
    body = b"AVI " + _chunk(b"LIST", hdrl) + _chunk(b"LIST", b"".join(movi)) + _chunk(b"idx1", b"".join(index))
    assert 8 + len(body) == total
    _write(path, b"RIFF" + struct.pack("<I", len(body)) + body)


def _check_fps(fps) -> float:
    if isinstance(fps, bool) or not isinstance(fps, (int, float, np.integer, np.floating)) or not fps > 0:
        raise ValueError(f"fps must be a positive number; got {fps!r}")
    return float(fps)


def write_gif(path, palettes, datas, width: int, height: int, fps=7) -> bytes:
    """An animated GIF that loops for ever, returned as ``bytes`` and written to ``path`` unless that is ``None``:
    ``GIF89a``, the logical screen descriptor (no global table), the NETSCAPE2.0 extension with loop count 0, and per frame
    a graphic control extension (delay ``max(1, round(100 / fps))`` centiseconds, no disposal, no transparency), an image
    descriptor of the whole screen with a 256-entry local table, the table (``palettes[i]``: 768 bytes or a (256, 3) uint8
    array) and the image data (``datas[i]``: minimum code size, sub-blocks, terminator -- what ``sp_gif_lzw`` writes); then
    the trailer."""
    if len(palettes) == 0 or len(palettes) != len(datas):
        raise ValueError(f"write_gif: no frames, or {len(palettes)} palettes for {len(datas)} frames")
    delay = max(1, round(100 / _check_fps(fps)))
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"a GIF is 1..65535 pixels on a side; got {height}x{width}")
    out = [b"GIF89a", struct.pack("<HHBBB", width, height, 0x70, 0, 0),
           b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", 0) + b"\x00"]
    control = b"\x21\xf9\x04" + struct.pack("<BHB", 0, min(delay, 65535), 0) + b"\x00"
    descriptor = b"\x2c" + struct.pack("<HHHHB", 0, 0, width, height, 0x87)
    for palette, data in zip(palettes, datas):
        table = palette if isinstance(palette, (bytes, bytearray)) else np.ascontiguousarray(palette, dtype=np.uint8).tobytes()
        if len(table) != 768:
            raise ValueError(f"write_gif: a local table holds 256 x 3 bytes; got {len(table)}")
        out += [control, descriptor, bytes(table), bytes(data)]
    out.append(b"\x3b")
    blob = b"".join(out)
    if path is not None:
        _write(path, blob)
    return blob


class GifEncoder(_FrameEncoder):
    """(F, H, W, 3) uint8 frames on the device -> one animated GIF, quantised and LZW-coded on the device (``csrc/gif.hip``).

    Every frame has a palette of its own (median cut over a 32^3 histogram, no dithering) and is coded in strips of
    ``strip_rows`` rows with a dictionary each, so that a frame is many independent sequences; at 576 x 1024 strips of 8 rows
    cost 2.1 % in size over one dictionary per frame and are the fastest measured (profiles/gif_timing.txt; 16 rows: 0.95 %).  Palette, index, stream, length and scratch buffers are kept
    per frame count; the stream buffer holds ``sp_gif_stream_bytes`` per frame (the size no input can exceed), of which only
    the used bytes are ever copied to the host."""

    def __init__(self, device, height: int, width: int, strip_rows: int = 8, fps=7) -> None:
        super().__init__(device, height, width)
        self.fps = _check_fps(fps)
        if not isinstance(strip_rows, (int, np.integer)) or strip_rows < 1:
            raise ValueError(f"strip_rows must be a positive integer; got {strip_rows!r}")
        self.strip_rows = int(strip_rows)
        self.cap = ops.gif_stream_bytes(self.height, self.width, self.strip_rows)
        if self.cap == 0:
            raise ValueError(f"a GIF frame is 1..65535 pixels on a side and at most 2^24 in all; got {height}x{width}")

    def enqueue(self, frames_u8: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Run the two stages on the current stream and return ``(palettes (F, 256, 3) uint8, streams (F, cap) uint8, lengths
        (F,) int32)``: views of this encoder's buffers, valid until the next call with as many frames."""
        n = self._check_frames(frames_u8)
        palettes = self._buf("palette", (n, 256, 3), torch.uint8)
        indices = self._buf("index", (n, self.height, self.width), torch.uint8)
        out = self._buf("stream", (n, self.cap), torch.uint8)
        lens = self._buf("len", (n,), torch.int32)
        ws = self._buf("ws", (ops.gif_ws_bytes(n, self.height, self.width, self.strip_rows),), torch.uint8)
        ops.gif_quantise(frames_u8.to(self.device).contiguous(), palettes, indices, ws)
        ops.gif_lzw(indices, out, lens, ws, strip_rows=self.strip_rows)
        return palettes, out, lens

    def collect(self, palettes: torch.Tensor, out: torch.Tensor, lens: torch.Tensor) -> bytes:
        """The file of an ``enqueue`` whose work has finished: the lengths come to the host first, then only the used bytes."""
        tables = palettes.cpu().numpy()
        return write_gif(None, list(tables), self._used_rows(out, lens), self.width, self.height, self.fps)

    def encode(self, frames_u8: torch.Tensor) -> bytes:
        return self._finished(self.enqueue, self.collect, frames_u8)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind: bytes, payload: bytes) -> bytes:
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(payload, zlib.crc32(kind)))


def _png_ihdr(height: int, width: int) -> bytes:
    if not (1 <= width <= 2 ** 31 - 1 and 1 <= height <= 2 ** 31 - 1):
        raise ValueError(f"a PNG is 1..2^31-1 pixels on a side; got {height}x{width}")
    return _png_chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))       # 8 bit, RGB, no interlace


def png_file(height: int, width: int, zlib_stream: bytes) -> bytes:
    """A PNG file around the zlib stream of an 8-bit RGB image's filtered rows (what ``sp_png_deflate`` writes): signature,
    IHDR, one IDAT, IEND.  The CRC-32 of every chunk is computed here (``zlib.crc32``)."""
    return PNG_SIGNATURE + _png_ihdr(height, width) + _png_chunk(b"IDAT", bytes(zlib_stream)) + _png_chunk(b"IEND", b"")


def write_apng(path, streams, width: int, height: int, fps=7) -> bytes:
    """An animated PNG that loops for ever, returned as ``bytes`` and written to ``path`` unless that is ``None``: signature,
    IHDR, acTL (``num_plays`` 0), and per frame an fcTL (the whole frame, delay ``1 / fps`` s as a fraction of two 16-bit
    numbers, dispose none, blend source) and its zlib stream, in IDAT for frame 0 and in fdAT behind a sequence number for the
    others; then IEND.  A viewer that knows no APNG shows frame 0."""
    if len(streams) == 0:
        raise ValueError("write_apng: no frames")
    delay = _apng_delay(fps, "write_apng: ")
    out, seq = [PNG_SIGNATURE, _png_ihdr(height, width), _png_chunk(b"acTL", struct.pack(">II", len(streams), 0))], 0
    for i, stream in enumerate(streams):
        out.append(_png_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, width, height, 0, 0, delay.numerator, delay.denominator, 0, 0)))
        seq += 1
        if i == 0:
            out.append(_png_chunk(b"IDAT", bytes(stream)))
        else:
            out.append(_png_chunk(b"fdAT", struct.pack(">I", seq) + bytes(stream)))
            seq += 1
    out.append(_png_chunk(b"IEND", b""))
    blob = b"".join(out)
    if path is not None:
        _write(path, blob)
    return blob


def _apng_delay(fps, who: str = "") -> Fraction:
    """The delay of an fcTL, for ``write_apng`` and for the device route, which takes the two numbers: ``1 / fps`` s as a
    fraction of two 16-bit numbers.  ``who`` goes in front of the refusal."""
    delay = (1 / Fraction(_check_fps(fps))).limit_denominator(65535)
    if not 0 < delay.numerator <= 65535:
        raise ValueError(f"{who}a delay of 1 / {fps} s does not fit the frame control chunk")
    return delay


PNG_ASSEMBLE = "device"             # chunks and CRC-32 on the device ("host": png_file / write_apng around the streams); profiles/png_timing.txt
PNG_STRIP_ROWS = 16                  # the fastest of 4 / 8 / 16 / 32 rows within 1 % of one strip per frame (profiles/png_timing.txt)


class PngEncoder(_FrameEncoder):
    """(F, H, W, 3) uint8 frames on the device -> one PNG file per frame, filtered and deflated on the device (``csrc/png.hip``).

    Every row takes the filter with the least sum of min(b, 256 - b); a frame is coded in strips of ``strip_rows`` rows, each
    one dynamic-Huffman block of literals and of matches at distance 1 (zlib's ``Z_RLE`` idea), so that a frame is many
    independent sequences; at 576 x 1024 strips of 16 rows cost 0.11 % in size over one strip per frame and are the fastest
    measured (profiles/png_timing.txt).  Filtered, stream, length and scratch
    buffers are kept per frame count; the stream buffer holds ``sp_png_stream_bytes`` per frame (the size no input can exceed),
    of which only the used bytes are ever copied to the host.

    ``assemble="device"`` (the default) also puts the files together there (``sp_png_wrap``: chunks, the CRC-32 of each, an
    animation's frames at the exclusive sum of their lengths), so that ``encode`` / ``encode_apng`` only copy finished files
    (``enqueue_files`` / ``collect_files``, ``enqueue_apng`` / ``collect_apng``); ``assemble="host"`` copies the streams and
    wraps them with ``png_file`` / ``write_apng`` (``zlib.crc32``).  The bytes are the same; ``enqueue`` / ``collect_streams``
    / ``collect`` are the host route's pieces under either setting."""

    def __init__(self, device, height: int, width: int, strip_rows: int = PNG_STRIP_ROWS, assemble: str = PNG_ASSEMBLE) -> None:
        super().__init__(device, height, width)
        if assemble not in ("device", "host"):
            raise ValueError(f"assemble must be 'device' or 'host'; got {assemble!r}")
        self.assemble = assemble
        if isinstance(strip_rows, bool) or not isinstance(strip_rows, (int, np.integer)) or strip_rows < 1:
            raise ValueError(f"strip_rows must be a positive integer; got {strip_rows!r}")
        self.strip_rows = int(strip_rows)
        self.cap = ops.png_stream_bytes(self.height, self.width, self.strip_rows)
        if self.cap == 0:
            raise ValueError(f"a frame for the PNG kernels is 1..65535 pixels on a side and at most 2^24 in all; got {height}x{width}")

    def enqueue(self, frames_u8: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Run the two stages on the current stream and return ``(streams (F, cap) uint8, lengths (F,) int32)``: views of
        this encoder's buffers, valid until the next call with as many frames."""
        n = self._check_frames(frames_u8)
        filtered = self._buf("filtered", (n, self.height, 1 + 3 * self.width), torch.uint8)
        out = self._buf("stream", (n, self.cap), torch.uint8)
        lens = self._buf("len", (n,), torch.int32)
        ws = self._buf("ws", (ops.png_ws_bytes(n, self.height, self.width, self.strip_rows),), torch.uint8)
        ops.png_filter(frames_u8.to(self.device).contiguous(), filtered)
        ops.png_deflate(filtered, out, lens, ws, strip_rows=self.strip_rows)
        return out, lens

    def collect_streams(self, out: torch.Tensor, lens: torch.Tensor) -> list[bytes]:
        """The zlib streams of an ``enqueue`` whose work has finished: the lengths come to the host first, then only the used
        bytes."""
        return self._used_rows(out, lens)

    def collect(self, out: torch.Tensor, lens: torch.Tensor) -> list[bytes]:
        """The PNG files of an ``enqueue`` whose work has finished."""
        return [png_file(self.height, self.width, s) for s in self.collect_streams(out, lens)]

    def enqueue_files(self, frames_u8: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """``enqueue``, then the files around the streams on the device (``sp_png_wrap``): ``(files (F, file_cap) uint8, lengths
        (F,) int32)``, row i the complete PNG of frame i, equal to ``png_file`` of its stream.  Views of this encoder's buffers,
        valid until the next call with as many frames."""
        out, lens = self.enqueue(frames_u8)
        n = out.shape[0]
        files = self._buf("files", (n, ops.png_file_bytes(self.height, self.width, self.strip_rows)), torch.uint8)
        file_lens = self._buf("file_len", (n,), torch.int32)
        ws = self._buf("wrap_ws", (ops.png_wrap_ws_bytes(n, self.cap),), torch.uint8)
        ops.png_wrap(out, lens, files, file_lens, ws, height=self.height, width=self.width)
        return files, file_lens

    def enqueue_apng(self, frames_u8: torch.Tensor, fps=7) -> tuple[torch.Tensor, torch.Tensor]:
        """``enqueue``, then one animated PNG of the frames on the device: ``(file (apng_file_bytes,) uint8, length (F,) int32 of
        which [0] counts)``, equal to ``write_apng`` of the streams (whose delay, ``1 / fps`` s as a fraction of two 16-bit
        numbers, is worked out here on the host)."""
        delay = _apng_delay(fps)
        out, lens = self.enqueue(frames_u8)
        n = out.shape[0]
        file = self._buf("apng", (ops.apng_file_bytes(n, self.height, self.width, self.strip_rows),), torch.uint8)
        file_lens = self._buf("apng_len", (n,), torch.int32)
        ws = self._buf("wrap_ws", (ops.png_wrap_ws_bytes(n, self.cap),), torch.uint8)
        ops.png_wrap(out, lens, file, file_lens, ws, height=self.height, width=self.width, animate=True,
                     delay=(delay.numerator, delay.denominator))
        return file, file_lens

    def collect_files(self, files: torch.Tensor, file_lens: torch.Tensor) -> list[bytes]:
        """The PNG files of an ``enqueue_files`` whose work has finished: the lengths come to the host first, then only the used
        bytes; the host adds nothing to them."""
        return self._used_rows(files, file_lens)

    def collect_apng(self, file: torch.Tensor, file_lens: torch.Tensor) -> bytes:
        """The animated PNG of an ``enqueue_apng`` whose work has finished: one copy of the length, one of the used bytes."""
        return file[:int(file_lens[:1].cpu()[0])].cpu().numpy().tobytes()

    def encode(self, frames_u8: torch.Tensor) -> list[bytes]:
        if self.assemble == "device":
            return self._finished(self.enqueue_files, self.collect_files, frames_u8)
        return self._finished(self.enqueue, self.collect, frames_u8)

    def encode_apng(self, frames_u8: torch.Tensor, fps=7) -> bytes:
        """One animated PNG of the frames: put together on the device, or under ``assemble="host"`` by ``write_apng`` around the
        same streams; the bytes are the same."""
        _check_fps(fps)
        if self.assemble == "device":
            return self._finished(self.enqueue_apng, self.collect_apng, frames_u8, fps)
        return write_apng(None, self._finished(self.enqueue, self.collect_streams, frames_u8), self.width, self.height, fps)


def _riff_chunk(kind: bytes, payload: bytes) -> list[bytes]:
    """The pieces of a RIFF chunk (an odd payload is padded to even); the caller joins all pieces of a file once, so that a
    frame's bytes are copied once."""
    return [kind, struct.pack("<I", len(payload)), payload] + ([b"\0"] if len(payload) & 1 else [])


def _riff_file(pieces: list[bytes]) -> bytes:
    return b"".join([b"RIFF", struct.pack("<I", 4 + sum(len(p) for p in pieces)), b"WEBP"] + pieces)


def _u24(value: int) -> bytes:
    return struct.pack("<I", value)[:3]


def webp_file(stream: bytes) -> bytes:
    """A still lossless WebP around a VP8L bitstream (what ``sp_webp_code`` writes): RIFF, WEBP, one VP8L chunk (an odd
    payload is padded to even).  The container has no checksum."""
    return _riff_file(_riff_chunk(b"VP8L", bytes(stream)))


def write_webp(path, streams, width: int, height: int, fps=7) -> bytes:
    """An animated lossless WebP that loops for ever, returned as ``bytes`` and written to ``path`` unless that is ``None``:
    VP8X (the animation flag only; the canvas is the frame), ANIM (background 0, loop count 0), and per frame an ANMF (offsets
    0, the whole frame, ``round(1000 / fps)`` ms in the 24-bit duration field, no blending, no disposal) around the frame's
    VP8L chunk."""
    if len(streams) == 0:
        raise ValueError("write_webp: no frames")
    ms = round(1000 / _check_fps(fps))
    if not 0 <= ms < 1 << 24:
        raise ValueError(f"write_webp: a duration of 1 / {fps} s does not fit the frame's 24-bit field of milliseconds")
    if not (1 <= width <= 16384 and 1 <= height <= 16384):
        raise ValueError(f"a lossless WebP frame is 1..16384 pixels on a side; got {height}x{width}")
    size = _u24(width - 1) + _u24(height - 1)
    out = _riff_chunk(b"VP8X", bytes([0x02, 0, 0, 0]) + size) + _riff_chunk(b"ANIM", struct.pack("<IH", 0, 0))
    frame_head = _u24(0) + _u24(0) + size + _u24(ms) + bytes([0x02])
    for stream in streams:
        inner = _riff_chunk(b"VP8L", bytes(stream))                 # (even in all, so the ANMF around it needs no padding)
        out += [b"ANMF", struct.pack("<I", len(frame_head) + sum(len(p) for p in inner)), frame_head] + inner
    blob = _riff_file(out)
    if path is not None:
        _write(path, blob)
    return blob


# blocks of 8 x 8 pixels and strips of 16 rows: the fastest whole call of the grid 4 / 8 / 16 / 32 x 8 / 16 / 32, or within the
# spread of the rounds of it, its files within 0.6 % of the grid's smallest (profiles/webp_timing.txt)
WEBP_PRED_BITS = 3
WEBP_GROUP_BITS = 4


def _check_webp_bits(pred_bits, group_bits) -> tuple[int, int]:
    if isinstance(pred_bits, bool) or not isinstance(pred_bits, (int, np.integer)) or not 2 <= pred_bits <= 9:
        raise ValueError(f"pred_bits must be an integer in 2..9; got {pred_bits!r}")
    if isinstance(group_bits, bool) or not isinstance(group_bits, (int, np.integer)) or not (group_bits == 0 or 2 <= group_bits <= 9):
        raise ValueError(f"group_bits must be 0 or an integer in 2..9; got {group_bits!r}")
    return int(pred_bits), int(group_bits)


class WebpEncoder(_FrameEncoder):
    """(F, H, W, 3) uint8 frames on the device -> one lossless WebP per frame or one animated WebP, transformed and entropy-coded
    on the device (``csrc/webp.hip``).

    Green is taken out of red and blue when an integer rule says it pays; every block of ``2^pred_bits`` pixels square takes
    the predictor with the least sum of min(b, 256 - b); a frame is coded in strips of ``2^group_bits`` rows, each with five
    prefix codes of its own (``group_bits = 0``: one set for the frame), of literals and of copies at distance 1, so that a
    frame is many independent sequences.  The defaults are blocks of 8 and strips of 16 rows: of the grid 4 / 8 / 16 / 32 x
    8 / 16 / 32 measured on one video of 14 x 576 x 1024 (profiles/webp_timing.txt) the row "pred_bits 3, group_bits 4" is the
    fastest whole call with channels that follow green (3.01 ms) and 0.1 ms, less than the spread of its rounds, behind
    "pred_bits 4, group_bits 4" with independent channels (3.62 against 3.52 ms); its file is within 0.2 % (independent
    channels) and 0.6 % (channels that follow green) of the smallest of the grid; strips of 16 rows have the fastest coder at
    every block size, strips of 8 and of 32 rows are 0.1 to 0.2 ms slower.  Residual, mode, flag, stream, length and scratch buffers are kept per frame count; the
    stream buffer holds ``sp_webp_stream_bytes`` per frame (the size no input can exceed), of which only the used bytes are
    ever copied to the host."""

    def __init__(self, device, height: int, width: int, pred_bits: int = WEBP_PRED_BITS, group_bits: int = WEBP_GROUP_BITS) -> None:
        super().__init__(device, height, width)
        self.pred_bits, self.group_bits = _check_webp_bits(pred_bits, group_bits)
        self.cap = ops.webp_stream_bytes(self.height, self.width, self.pred_bits, self.group_bits)
        if self.cap == 0:
            raise ValueError(f"a frame for the WebP kernels is 1..16384 pixels on a side and at most 2^24 in all; got {height}x{width}")

    def enqueue(self, frames_u8: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Run the two stages on the current stream and return ``(streams (F, cap) uint8, lengths (F,) int32)``: views of
        this encoder's buffers, valid until the next call with as many frames."""
        n, block = self._check_frames(frames_u8), 1 << self.pred_bits
        residual = self._buf("residual", (n, self.height, self.width, 4), torch.uint8)
        modes = self._buf("modes", (n, -(-self.height // block), -(-self.width // block)), torch.uint8)
        flags = self._buf("flags", (n,), torch.int32)
        out = self._buf("stream", (n, self.cap), torch.uint8)
        lens = self._buf("len", (n,), torch.int32)
        ws = self._buf("ws", (ops.webp_ws_bytes(n, self.height, self.width, self.pred_bits, self.group_bits),), torch.uint8)
        ops.webp_transform(frames_u8.to(self.device).contiguous(), residual, modes, flags, ws, pred_bits=self.pred_bits)
        ops.webp_code(residual, modes, flags, out, lens, ws, pred_bits=self.pred_bits, group_bits=self.group_bits)
        return out, lens

    def collect_streams(self, out: torch.Tensor, lens: torch.Tensor) -> list[bytes]:
        """The VP8L streams of an ``enqueue`` whose work has finished: the lengths come to the host first, then only the used
        bytes."""
        return self._used_rows(out, lens)

    def collect(self, out: torch.Tensor, lens: torch.Tensor) -> list[bytes]:
        """The still ``.webp`` files of an ``enqueue`` whose work has finished."""
        return [webp_file(s) for s in self.collect_streams(out, lens)]

    def encode(self, frames_u8: torch.Tensor) -> list[bytes]:
        return self._finished(self.enqueue, self.collect, frames_u8)

    def encode_animation(self, frames_u8: torch.Tensor, fps=7) -> bytes:
        """One animated WebP of the frames (``write_webp`` around the same streams)."""
        _check_fps(fps)
        return write_webp(None, self._finished(self.enqueue, self.collect_streams, frames_u8), self.width, self.height, fps)


INTERP_FACTORS = (1, 2, 4)


def _check_interpolate(factor) -> int:
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or factor not in INTERP_FACTORS:
        raise ValueError(f"interpolate must be 1, 2 or 4; got {factor!r}")
    return int(factor)


def _check_interp_search(search_range, penalty) -> tuple[int, int]:
    """``(search_range, penalty)`` as ints, or ``ValueError``: the one check of ``FrameInterpolator`` and its callers."""
    if isinstance(search_range, bool) or not isinstance(search_range, (int, np.integer)) or not 1 <= search_range <= 24:
        raise ValueError(f"search_range must be an integer from 1 to 24; got {search_range!r}")
    if isinstance(penalty, bool) or not isinstance(penalty, (int, np.integer)) or not 0 <= penalty <= 255:
        raise ValueError(f"penalty must be an integer from 0 to 255; got {penalty!r}")
    return int(search_range), int(penalty)


class FrameInterpolator(_FrameEncoder):
    """(F, H, W, 3) uint8 frames on the device -> ((F - 1) * factor + 1, H, W, 3) uint8 on the device: every round puts the
    motion-compensated midpoint between neighbours (``out[2i]`` is frame i), ``factor`` 4 is two rounds, ``factor`` 1 hands the
    input back as it is.  Per pair and 8x8 block an exhaustive bilateral search over ``[-search_range, search_range]^2`` on
    luma (``penalty`` per unit of |vy| + |vx| against wandering vectors in flat areas), a 3x3 median of the vectors and an
    overlapped blend of the two displaced frames (``ops.interp_motion`` / ``ops.interp_compensate``); H and W are multiples
    of 8, at least 16.  Scratch, vectors and frames are kept per frame count; the result is a view of this object's buffers,
    valid until the next call with as many frames.  ``vectors`` is the last round's (pairs, H / 8, W / 8, 2) int16 in (vy, vx)
    order.  This is classical interpolation: no learned model's quality, and where something is uncovered or hidden between
    two frames the blend of the two is all there is."""

    def __init__(self, device, height: int, width: int, factor: int = 2, search_range: int = 16, penalty: int = 4) -> None:
        super().__init__(device, height, width)
        self.factor = _check_interpolate(factor)
        if self.height % 8 or self.width % 8 or self.height < 16 or self.width < 16:
            raise ValueError(f"frame interpolation needs a height and width that are multiples of 8 and at least 16; got "
                             f"{self.height} x {self.width}")
        self.search_range, self.penalty = _check_interp_search(search_range, penalty)
        self.vectors = None

    def enqueue(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """Run the rounds on the current stream and return the frames (for ``factor`` 1, or one frame, the input itself)."""
        n = self._check_frames(frames_u8)
        if self.factor == 1 or n == 1:
            return frames_u8
        frames = frames_u8.to(self.device).contiguous()
        h, w = self.height, self.width
        for rnd in range(self.factor.bit_length() - 1):
            ws = self._buf(f"ws{rnd}", (ops.interp_ws_bytes(n, h, w, self.search_range),), torch.uint8)
            self.vectors = self._buf(f"vectors{rnd}", (n - 1, h // 8, w // 8, 2), torch.int16)
            out = self._buf(f"out{rnd}", (2 * n - 1, h, w, 3), torch.uint8)
            ops.interp_motion(frames, self.vectors, ws, search_range=self.search_range, penalty=self.penalty)
            frames, n = ops.interp_compensate(frames, self.vectors, out), 2 * n - 1
        return frames

    __call__ = enqueue


def _jpeg_frames(frames_u8, quality: int) -> tuple[list[bytes], int, int]:
    """``(files, height, width)``: a tensor on a GPU is compressed there (``JpegEncoder``), anything else by Pillow."""
    if isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda:
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or 0 in frames_u8.shape:
            raise ValueError(f"frames must be (F, H, W, 3) uint8; got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        _, h, w, _ = frames_u8.shape
        return JpegEncoder(frames_u8.device, h, w, quality).encode(frames_u8), h, w
    a = _frames_array(frames_u8)
    return [_pillow_bytes(f, "JPEG", quality=quality, subsampling=2) for f in a], a.shape[1], a.shape[2]      # 4:2:0


def _frames_array(frames_u8) -> np.ndarray:
    a = frames_u8.cpu().numpy() if isinstance(frames_u8, torch.Tensor) else np.asarray(frames_u8)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"frames must be (F, H, W, 3) uint8; got {a.dtype} {a.shape}")
    return a


_FFMPEG_EXTS = (".mp4", ".mov", ".mkv", ".webm")


def _needs_ffmpeg(path: str) -> ValueError:
    return ValueError(f"cannot write '{path}': video encoding needs imageio / ffmpeg, which this package does not depend "
                      f"on; write .avi (Motion-JPEG) instead, or .gif, .webp (lossless, animated), .npy, JPEG or PNG frames (a "
                      f"%03d.jpg / %03d.png pattern or a directory)")


def _unknown_format(path: str, ext: str) -> ValueError:
    return ValueError(f"'{path}': unknown output format {ext!r} (.avi, .gif, .apng, .webp, .npy, %03d.jpg / %03d.png / "
                      f"%03d.webp pattern or a directory)")


def _check_target(path: str, ext: str, fps, quality) -> None:
    """What ``save_frames`` refuses about a target and its ``fps`` / ``quality``, with no look at the frames: asked before
    work is spent on frames that could not be written."""
    if ext in _FFMPEG_EXTS:
        raise _needs_ffmpeg(path)
    if ext not in (".avi", ".jpg", ".jpeg", ".gif", ".apng", ".webp", ".npy", ".png", ""):
        raise _unknown_format(path, ext)
    if ext in (".avi", ".jpg", ".jpeg"):
        _check_quality(quality)
    if ext == ".avi" and (isinstance(fps, bool) or not isinstance(fps, (int, np.integer)) or fps <= 0):
        raise ValueError("fps must be a positive integer")
    if ext in (".gif", ".apng") or (ext == ".webp" and "%" not in path):
        _check_fps(fps)
    if ext in (".jpg", ".jpeg", ".png") and "%" not in path:
        raise ValueError(f"'{path}': {'PNG' if ext == '.png' else 'JPEG'} output needs a frame pattern such as "
                         f"frame_%03d{ext}")


def save_frames(frames_u8, path: str, fps: int = 7, quality: int = 90, interpolate: int = 1, interp_range: int = 16,
                interp_penalty: int = 4) -> list[str]:
    """Write one video's (F, H, W, 3) uint8 frames and return the files written.  ``*.avi``: Motion-JPEG at ``fps`` frames
    per second, the video file of the reference's ``save_video`` (ref :198-209) in a container that needs no ffmpeg;
    ``*.gif``: an animated GIF that loops for ever, ``1000 / fps`` ms per frame (ref ``save_gif`` :212-222); ``*.npy``:
    the raw array; a ``%03d``-style ``*.jpg`` / ``*.jpeg`` pattern: one JPEG per frame; a directory or a ``%03d``-style
    ``*.png`` pattern: one PNG per frame.  ``quality`` (1..100) is that of the JPEG frames; a tensor on a GPU is compressed
    there and only the compressed bytes are copied.  The same holds for ``*.gif``: a tensor on a GPU is quantised and
    LZW-coded there (``GifEncoder``: a palette per frame, strips of 8 rows, delays in whole centiseconds), while an array in
    host memory goes through Pillow as before, byte for byte.  PNG frames (a directory or a ``%03d.png`` pattern) and
    ``*.apng`` (one animated PNG, lossless, ``1 / fps`` s per frame) of a tensor on a GPU are filtered and deflated there
    (``PngEncoder``); an array in host memory goes through Pillow.  ``*.webp`` is lossless WebP: one animated file
    (``round(1000 / fps)`` ms per frame, looping for ever), or with a ``%03d``-style pattern one still per frame; a tensor on
    a GPU is transformed and entropy-coded there (``WebpEncoder``), an array in host memory, or frames the kernels refuse, go
    through Pillow (``lossless=True``).  ``*.mp4`` is refused: imageio / ffmpeg are not dependencies.

    ``interpolate`` 2 or 4 puts motion-compensated frames between the frames first (``FrameInterpolator`` with
    ``interp_range`` and ``interp_penalty``) and writes at ``fps * interpolate``, so the video lasts as long as before
    (to within one frame time).  That runs on the device only: the frames must be a tensor on a GPU, of a height and width
    that are multiples of 8."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if _check_interpolate(interpolate) > 1:
        if not (isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda):
            raise ValueError(f"interpolate={interpolate} runs on the device (image_io.FrameInterpolator): pass the frames as a "
                             f"uint8 tensor on a GPU, or interpolate=1 for frames in host memory")
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or 0 in frames_u8.shape:
            raise ValueError(f"frames must be (F, H, W, 3) uint8; got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        # (a frame size that is not a multiple of 8 is refused here, by the interpolator); no kernel runs before the
        # target and its arguments are accepted
        interpolator = FrameInterpolator(frames_u8.device, frames_u8.shape[1], frames_u8.shape[2], interpolate, interp_range,
                                         interp_penalty)
        _check_target(path, ext, fps, quality)
        frames_u8, fps = interpolator(frames_u8), fps * interpolate
    # frames on a GPU stay there for the targets that are compressed there; everything else is host work on an array
    on_gpu = isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda and ext in (".avi", ".jpg", ".jpeg", ".gif", ".apng", "")
    if on_gpu and ext == ".gif" and frames_u8.dim() == 4 and frames_u8.shape[1] * frames_u8.shape[2] > 2 ** 24:
        on_gpu = False                 # beyond what sp_gif_quantise_u8 takes: the route such frames always had
    if isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda and ext == ".png" and "%" in path:
        on_gpu = True                  # (a bare x.png is refused below, as it always was)
    if on_gpu and ext in (".png", ".apng", ""):
        # frames the PNG kernels do not take (or that are no frames at all) keep the host route and its messages
        on_gpu = (frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[3] == 3 and frames_u8.shape[0] > 0
                  and ops.png_stream_bytes(frames_u8.shape[1], frames_u8.shape[2], PNG_STRIP_ROWS) > 0)
    if isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda and ext == ".webp":
        # likewise for the WebP kernels
        on_gpu = (frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[3] == 3 and frames_u8.shape[0] > 0
                  and ops.webp_stream_bytes(frames_u8.shape[1], frames_u8.shape[2], WEBP_PRED_BITS, WEBP_GROUP_BITS) > 0)
    a = None if on_gpu else _frames_array(frames_u8)
    if ext in _FFMPEG_EXTS:
        raise _needs_ffmpeg(path)
    if ext in (".avi", ".jpg", ".jpeg"):
        _check_quality(quality)
        if ext == ".avi" and (not isinstance(fps, (int, np.integer)) or fps <= 0):
            raise ValueError("fps must be a positive integer")
        if ext != ".avi" and "%" not in path:
            raise ValueError(f"'{path}': JPEG output needs a frame pattern such as frame_%03d.jpg")
        jpegs, h, w = _jpeg_frames(frames_u8 if on_gpu else a, quality)
        if ext == ".avi":
            write_avi(path, jpegs, w, h, fps)
            return [path]
        return _write_numbered(path, len(jpegs), jpegs)
    if ext == ".npy":
        np.save(path, a)
        return [path]
    if ext == ".gif" and on_gpu:
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or 0 in frames_u8.shape:
            raise ValueError(f"frames must be (F, H, W, 3) uint8; got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        _check_fps(fps)
        _write(path, GifEncoder(frames_u8.device, frames_u8.shape[1], frames_u8.shape[2], fps=fps).encode(frames_u8))
        return [path]
    if on_gpu and ext in (".png", ".apng", ""):
        enc = PngEncoder(frames_u8.device, frames_u8.shape[1], frames_u8.shape[2])
        if ext == ".apng":
            _write(path, enc.encode_apng(frames_u8, fps))
            return [path]
        if ext == "":
            os.makedirs(path, exist_ok=True)
        pattern = path if ext == ".png" else os.path.join(path, "%03d.png")
        return _write_numbered(pattern, frames_u8.shape[0], enc.encode(frames_u8))
    if ext == ".webp" and on_gpu:
        enc = WebpEncoder(frames_u8.device, frames_u8.shape[1], frames_u8.shape[2])
        if "%" not in path:
            _write(path, enc.encode_animation(frames_u8, fps))
            return [path]
        return _write_numbered(path, frames_u8.shape[0], enc.encode(frames_u8))
    from PIL import Image

    if ext == ".webp":
        if "%" not in path:
            ms = round(1000 / _check_fps(fps))
            ims = [Image.fromarray(f) for f in a]
            ims[0].save(path, format="WEBP", save_all=True, append_images=ims[1:], lossless=True, loop=0, duration=ms)
            return [path]
        return _write_numbered(path, len(a), (_pillow_bytes(f, "WEBP", lossless=True) for f in a))
    if ext == ".apng":
        _check_fps(fps)
        ims = [Image.fromarray(f) for f in a]
        ims[0].save(path, format="PNG", save_all=True, append_images=ims[1:], loop=0, duration=1000.0 / fps)
        return [path]
    if ext == ".gif":
        if fps <= 0:
            raise ValueError("fps must be positive")
        ims = [Image.fromarray(f) for f in a]
        ims[0].save(path, save_all=True, append_images=ims[1:], loop=0, duration=1000.0 / fps)
        return [path]
    if ext == ".png":
        if "%" not in path:
            raise ValueError(f"'{path}': PNG output needs a frame pattern such as frame_%03d.png (or pass a directory)")
        pattern = path
    elif ext == "":
        os.makedirs(path, exist_ok=True)
        pattern = os.path.join(path, "%03d.png")
    else:
        raise _unknown_format(path, ext)
    return _write_numbered(pattern, len(a), (_pillow_bytes(f, "PNG") for f in a))
