"""Picture in, 8-bit frames out: the host-side image handling of the reference's demo
(``/root/reference/scripts/generate_video_demo.py``) around the edge stages of ``edge_stages.py``.

  * ``ImageFrontEnd``: ``load_and_preprocess_image`` (ref ``:71-89``: Lanczos cover-resize + centre crop) followed by what
    ``encode_image`` does to the cropped picture before the two encoders run (ref ``:108-126``: the ``CLIPImageProcessor``
    -- bicubic shortest-edge resize, centre crop, rescale, normalise -- and ``ToTensor`` + ``Normalize([0.5], [0.5])``), on
    the device with the kernels of ``csrc/image.hip``.  Pillow's resize is reproduced to within one 8-bit level (its
    weights are 22-bit fixed point, the kernel's fp32); the geometry rules below are the reference's exactly.
  * ``frames_to_uint8`` / ``save_frames``: ``save_video`` / ``save_gif`` (ref ``:198-222``) without imageio.
  * ``load_image``: the decode half of ``load_and_preprocess_image`` (Pillow; a file format is host work).
"""

from __future__ import annotations

import os

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


def save_frames(frames_u8, path: str, fps: int = 7) -> list[str]:
    """Write one video's (F, H, W, 3) uint8 frames and return the files written.  ``*.gif``: an animated GIF that loops
    for ever, ``1000 / fps`` ms per frame (ref ``save_gif`` :212-222); ``*.npy``: the raw array; a directory or a
    ``%03d``-style ``*.png`` pattern: one PNG per frame.  ``*.mp4`` is refused: imageio / ffmpeg are not dependencies."""
    a = frames_u8.cpu().numpy() if isinstance(frames_u8, torch.Tensor) else np.asarray(frames_u8)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"frames must be (F, H, W, 3) uint8; got {a.dtype} {a.shape}")
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext in (".mp4", ".mov", ".mkv", ".webm", ".avi"):
        raise ValueError(f"cannot write '{path}': video encoding needs imageio / ffmpeg, which this package does not depend "
                         f"on; write .gif, .npy or PNG frames (a directory or a %03d.png pattern)")
    if ext == ".npy":
        np.save(path, a)
        return [path]
    from PIL import Image

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
        raise ValueError(f"'{path}': unknown output format {ext!r} (.gif, .npy, %03d.png pattern or a directory)")
    files = []
    for i, f in enumerate(a):
        files.append(pattern % i)
        Image.fromarray(f).save(files[-1])
    return files
