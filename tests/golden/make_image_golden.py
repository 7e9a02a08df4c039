"""Mint the image front end's golden vectors by running the reference's own host-side image handling.

The reference's demo turns a picture file into conditioning with Pillow and the CLIP feature extractor
(``/root/reference/scripts/generate_video_demo.py``: ``load_and_preprocess_image`` :71-89 -- Lanczos cover-resize and
centre crop -- and ``encode_image`` :108-126 -- ``CLIPImageProcessor`` plus ``ToTensor`` / ``Normalize([0.5], [0.5])``).
Pillow and transformers are installed in this image, so the vectors are minted by the real third-party code:

    python tests/golden/make_image_golden.py        # Pillow / transformers versions are recorded in the file

``load_and_preprocess_image`` is imported from the reference script by path.  Without torchvision
``transformers.CLIPImageProcessor`` runs its PIL backend (Pillow's BICUBIC resize, numpy crop / rescale / normalise): that
is the path pinned here.  torchvision's two transforms are stated with the torch calls they are made of
(``ToTensor``: ``permute(2, 0, 1).float().div(255)``; ``Normalize``: ``sub(mean).div(std)``).

Output (committed, data only): ``image_io.npz``.  Source images are synthetic and are NOT stored: ``source_image``
regenerates them from a seed (a CRC of every source is stored, so a platform that generates other pixels is noticed).

  raw resample cases   ``RAW_CASES`` x ``KINDS``: Pillow's ``Image.resize`` output, and the share of values at which the
                       fp64 numpy statement of the algorithm (``resample_model``; include/svdpipe.h states it) differs
                       from Pillow by one level.  Pillow's weights are 22-bit fixed point, so a floating-point
                       evaluation cannot be bit-exact; the minter refuses a case whose model differs by more than one
                       level or at more than 1.5 % of the values, so the tests' cap (1 level, 2 %) is never filled by
                       the reference's own noise.
  whole-chain cases    ``CHAIN_CASES`` at 64x128 / CLIP size 56: the reference's cropped uint8 image, ``pixel_values``,
                       the normalised image tensor and the geometry both resizes arrived at.
  geometry table       what the real functions do for ``COVER_PAIRS`` / ``CLIP_PAIRS`` (recorded from the reference
                       function's own ``resize`` / ``crop`` calls and from transformers' size and crop helpers).

``tests/test_image_io_cpu.py`` re-mints all of it in memory against the stored file (version drift shows there);
``tests/test_image_io_gpu.py`` checks the HIP kernels against the stored outputs.
"""

from __future__ import annotations

import importlib.util
import os
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "image_io.npz")
REFERENCE_SCRIPT = "/root/reference/scripts/generate_video_demo.py"

KINDS = ("noise", "mix", "smooth")
# ((src_h, src_w), (dst_h, dst_w), filter): "L" = Lanczos (support 3), "B" = bicubic (a = -0.5, support 2)
RAW_CASES = [
    ((37, 53), (75, 109), "L"),          # enlarge, odd sizes
    ((97, 131), (32, 64), "L"),          # reduce by different factors per axis
    ((200, 150), (28, 28), "B"),
    ((5, 7), (64, 128), "L"),            # every tap window is cut by a border
    ((5, 7), (64, 128), "B"),
    ((8, 1024), (4, 16), "L"),           # 64x reduction: 385 taps
    ((1024, 16), (16, 16), "L"),         # the same vertically; the horizontal pass is a copy
    ((33, 33), (32, 32), "L"),           # scale just above 1
    ((33, 33), (34, 34), "B"),           # scale just below 1
    ((1, 1), (8, 8), "L"),
    ((2, 300), (2, 7), "L"),             # the vertical pass is a copy
]
TARGET_H, TARGET_W, CLIP_SIZE = 64, 128, 56
# ((src_h, src_w), kind): 64x128 takes no resize (the crop must be the input itself), 50x70 is enlarged
CHAIN_CASES = [((90, 200), "noise"), ((300, 170), "mix"), ((301, 171), "smooth"), ((64, 128), "noise"), ((50, 70), "mix")]
MAX_MODEL_SHARE = 0.015

# (src_h, src_w, height, width) for the cover rule; several land on .5 ties of Python's round (half to even)
COVER_PAIRS = [
    (90, 200, 64, 128), (300, 170, 64, 128), (301, 171, 64, 128), (64, 128, 64, 128), (50, 70, 64, 128),
    (3, 4, 4, 6), (5, 4, 4, 6), (101, 200, 50, 100), (103, 200, 50, 100), (200, 101, 100, 50), (200, 103, 100, 50),
    (7, 10, 10, 25), (9, 10, 10, 25), (25, 2, 31, 5), (27, 2, 31, 5), (3000, 4000, 576, 1024), (4000, 3000, 576, 1024),
    (1080, 1920, 576, 1024), (1920, 1080, 576, 1024), (576, 1024, 576, 1024), (577, 1024, 576, 1024), (576, 1025, 576, 1024),
    (575, 1023, 576, 1024), (1152, 2048, 576, 1024), (1153, 2048, 576, 1024), (1155, 2048, 576, 1024), (768, 768, 576, 1024),
    (512, 512, 576, 1024), (333, 500, 576, 1024), (1, 1, 64, 128), (2, 300, 64, 128), (1000, 3, 64, 128), (720, 1280, 320, 512),
    (721, 1283, 320, 512), (1365, 2048, 576, 1024), (2048, 1365, 576, 1024), (683, 1024, 576, 1024), (1024, 683, 576, 1024),
    (480, 640, 576, 1024), (640, 480, 576, 1024),
]
# (height, width, clip_size) for the CLIP processor's shortest-edge resize + centre crop
CLIP_PAIRS = [
    (576, 1024, 224), (1024, 576, 224), (64, 128, 56), (128, 64, 56), (320, 512, 224), (224, 224, 224), (225, 224, 224),
    (224, 225, 224), (223, 224, 224), (576, 1024, 56), (100, 301, 56), (301, 100, 56), (57, 56, 56), (56, 57, 56), (55, 110, 56),
    (7, 9, 224), (448, 449, 224), (1000, 1001, 224), (333, 500, 224), (500, 333, 224), (512, 512, 224), (720, 1280, 224),
    (90, 200, 56), (65, 129, 56), (63, 127, 56), (1, 3, 56), (2, 2, 56), (1080, 1920, 224), (143, 256, 56), (144, 256, 56),
    (257, 144, 56), (96, 97, 14), (97, 96, 14), (13, 40, 14), (576, 1023, 224), (575, 1024, 224), (600, 800, 224), (800, 600, 224),
    (48, 64, 56), (64, 48, 56),
]


def source_image(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    """(h, w, 3) uint8: uniform noise; "mix" = a sinusoid plus Gaussian noise; "smooth" = three linear ramps."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == "mix":
        ph = np.array([0.0, 1.3, 2.9]).reshape(1, 1, 3)
        wave = 127.5 + 80.0 * np.sin(2.0 * np.pi * (3.0 * x / max(w, 1) + 2.0 * y / max(h, 1))[..., None] + ph)
        return np.clip(np.floor(wave + 20.0 * rs.randn(h, w, 3) + 0.5), 0, 255).astype(np.uint8)
    if kind == "smooth":
        r = (255 * x) // max(w - 1, 1)
        g = (255 * y) // max(h - 1, 1)
        b = 255 - (255 * (x + y)) // max(w + h - 2, 1)
        return np.stack([r, g, b], axis=-1).astype(np.uint8)
    raise ValueError(kind)


def case_seed(group: int, index: int, kind: str) -> int:
    return 20261017 + 1000 * group + 10 * index + KINDS.index(kind)


def crc(a: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# ------------------------------------------------------------------ the algorithm, in numpy (fp64 unless told otherwise)
def _filter(x, filt):
    if filt == "B":
        a = -0.5
        x = np.abs(x)
        return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                        np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))
    inside = (x >= -3.0) & (x < 3.0)
    return np.where(inside, np.sinc(x) * np.sinc(x / 3.0), 0.0)


def _axis_weights(n_in: int, n_out: int, filt: str) -> np.ndarray:
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = (3.0 if filt == "L" else 2.0) * fs
    wm = np.zeros((n_out, n_in))
    for i in range(n_out):
        centre = (i + 0.5) * scale
        lo = max(0, int(centre - support + 0.5))
        hi = min(n_in, int(centre + support + 0.5))
        k = np.arange(lo, hi)
        wk = _filter((k - centre + 0.5) / fs, filt)
        wm[i, lo:hi] = wk / wk.sum()
    return wm


def resample_model(img: np.ndarray, dst_h: int, dst_w: int, filt: str, dtype=np.float64) -> np.ndarray:
    """Pillow's antialiased separable resize as include/svdpipe.h states it: horizontal pass, uint8, vertical pass."""
    h, w, _ = img.shape
    out = img
    if dst_w != w:
        wm = _axis_weights(w, dst_w, filt).astype(dtype)
        out = np.clip(np.floor(np.einsum("ok,hkc->hoc", wm, out.astype(dtype)) + dtype(0.5)), 0, 255).astype(np.uint8)
    if dst_h != h:
        wm = _axis_weights(h, dst_h, filt).astype(dtype)
        out = np.clip(np.floor(np.einsum("ok,kwc->owc", wm, out.astype(dtype)) + dtype(0.5)), 0, 255).astype(np.uint8)
    return out


def compare_levels(got: np.ndarray, want: np.ndarray) -> tuple[int, float]:
    """(largest difference in levels, share of values that differ)."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d != 0).mean())


# ------------------------------------------------------------------ the real functions
def _reference_module():
    spec = importlib.util.spec_from_file_location("reference_generate_video_demo", REFERENCE_SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _clip_processor(size: int):
    from transformers import CLIPImageProcessor

    return CLIPImageProcessor(size={"shortest_edge": size}, crop_size={"height": size, "width": size})


def _recorded_cover_geometry(ref, src_h, src_w, height, width):
    """(new_h, new_w, top, left) out of the reference function's own resize / crop calls (on blank stand-in images)."""
    from PIL import Image

    seen = {"size": (src_w, src_h)}
    real_open, real_resize, real_crop = Image.open, Image.Image.resize, Image.Image.crop

    def fake_resize(self, size, *a, **k):
        seen["size"] = tuple(size)
        return Image.new("RGB", tuple(size))

    def fake_crop(self, box=None):
        seen["box"] = tuple(box)
        return real_crop(self, box)

    Image.open = lambda *_a, **_k: Image.new("RGB", (src_w, src_h))
    Image.Image.resize, Image.Image.crop = fake_resize, fake_crop
    try:
        out = ref.load_and_preprocess_image("unused", height, width)
    finally:
        Image.open, Image.Image.resize, Image.Image.crop = real_open, real_resize, real_crop
    assert out.size == (width, height)
    return seen["size"][1], seen["size"][0], seen["box"][1], seen["box"][0]


def _recorded_clip_geometry(h, w, size):
    """(new_h, new_w, top, left) from transformers' own size rule and its crop of an image that holds its coordinates."""
    from transformers.image_transforms import center_crop, get_resize_output_image_size
    from transformers.image_utils import ChannelDimension

    new_h, new_w = get_resize_output_image_size(np.zeros((3, h, w), np.uint8), size=size, default_to_square=False,
                                                input_data_format=ChannelDimension.FIRST)
    yy, xx = np.mgrid[0:new_h, 0:new_w]
    coords = np.stack([yy, xx, yy]).astype(np.int32)
    c = center_crop(coords, size=(size, size), data_format=ChannelDimension.FIRST, input_data_format=ChannelDimension.FIRST)
    return int(new_h), int(new_w), int(c[0, 0, 0]), int(c[1, 0, 0])


def build() -> dict:
    import PIL
    import torch
    import transformers
    from PIL import Image

    ref = _reference_module()
    arrays: dict = {"pillow_version": np.array(PIL.__version__), "transformers_version": np.array(transformers.__version__)}
    pil_filter = {"L": Image.LANCZOS, "B": Image.BICUBIC}

    shares = np.zeros((len(RAW_CASES), len(KINDS)))
    crcs = np.zeros((len(RAW_CASES), len(KINDS)), np.int64)
    for i, ((sh, sw), (dh, dw), filt) in enumerate(RAW_CASES):
        for j, kind in enumerate(KINDS):
            src = source_image(kind, sh, sw, case_seed(0, i, kind))
            want = np.asarray(Image.fromarray(src).resize((dw, dh), pil_filter[filt]))
            worst, share = compare_levels(resample_model(src, dh, dw, filt), want)
            if worst > 1 or share > MAX_MODEL_SHARE:
                raise SystemExit(f"raw case {i} ({sh}x{sw} -> {dh}x{dw} {filt}, {kind}): the fp64 model is {worst} levels / "
                                 f"{share:.2%} off Pillow -- not a case the 1-level / 2 % cap can carry")
            arrays[f"raw{i}_{kind}"] = want
            shares[i, j], crcs[i, j] = share, crc(src)
    arrays["raw_model_share"], arrays["raw_source_crc"] = shares, crcs

    proc = _clip_processor(CLIP_SIZE)
    arrays["clip_mean"] = np.array(proc.image_mean, np.float64)
    arrays["clip_std"] = np.array(proc.image_std, np.float64)
    chain_share = np.zeros((len(CHAIN_CASES), 2))
    chain_crc = np.zeros(len(CHAIN_CASES), np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        for i, ((sh, sw), kind) in enumerate(CHAIN_CASES):
            src = source_image(kind, sh, sw, case_seed(1, i, kind))
            path = os.path.join(tmp, f"src{i}.png")
            Image.fromarray(src).save(path)
            image = ref.load_and_preprocess_image(path, TARGET_H, TARGET_W)
            cropped = np.asarray(image)
            pixel_values = proc(images=image, return_tensors="np").pixel_values[0].astype(np.float32)
            tensor = torch.from_numpy(cropped.copy()).permute(2, 0, 1).float().div(255)        # ToTensor
            tensor = tensor.sub(0.5).div(0.5).numpy()                                          # Normalize([0.5], [0.5])
            new_h, new_w, top, left = _recorded_cover_geometry(ref, sh, sw, TARGET_H, TARGET_W)
            ch, cw, ctop, cleft = _recorded_clip_geometry(TARGET_H, TARGET_W, CLIP_SIZE)
            # the model of the whole chain: cover-resize, crop, bicubic shortest-edge resize of the CROPPED image, crop
            m = src if (new_h, new_w) == (sh, sw) else resample_model(src, new_h, new_w, "L")
            m = m[top:top + TARGET_H, left:left + TARGET_W]
            worst, share = compare_levels(m, cropped)
            mc = resample_model(cropped, ch, cw, "B")[ctop:ctop + CLIP_SIZE, cleft:cleft + CLIP_SIZE]
            mean, std = np.array(proc.image_mean, np.float32), np.array(proc.image_std, np.float32)
            lv = np.abs((mc.astype(np.float32) / 255.0 - mean) / std - pixel_values.transpose(1, 2, 0)) * 255.0 * std
            worst_c, share_c = float(lv.max()), float((lv > 0.5).mean())
            if worst > 1 or share > MAX_MODEL_SHARE or worst_c > 1.001 or share_c > MAX_MODEL_SHARE:
                raise SystemExit(f"chain case {i}: the fp64 model is off by {worst} / {worst_c:.3f} levels at "
                                 f"{share:.2%} / {share_c:.2%} of the values")
            arrays[f"chain{i}_cropped"], arrays[f"chain{i}_pixel_values"] = cropped, pixel_values
            arrays[f"chain{i}_image_tensor"] = tensor
            arrays[f"chain{i}_geometry"] = np.array([new_h, new_w, top, left, ch, cw, ctop, cleft], np.int64)
            chain_share[i], chain_crc[i] = (share, share_c), crc(src)
    arrays["chain_model_share"], arrays["chain_source_crc"] = chain_share, chain_crc

    arrays["cover_pairs"] = np.array(COVER_PAIRS, np.int64)
    arrays["cover_geometry"] = np.array([_recorded_cover_geometry(ref, *p) for p in COVER_PAIRS], np.int64)
    arrays["clip_pairs"] = np.array(CLIP_PAIRS, np.int64)
    arrays["clip_geometry"] = np.array([_recorded_clip_geometry(*p) for p in CLIP_PAIRS], np.int64)
    return arrays


def main():
    arrays = build()
    np.savez_compressed(PATH, **arrays)
    print(f"wrote {PATH} ({os.path.getsize(PATH) / 1e6:.2f} MB), Pillow {arrays['pillow_version']}, "
          f"transformers {arrays['transformers_version']}")
    print("share of values where the fp64 model is one level off Pillow, raw cases (noise, mix, smooth):")
    for case, row in zip(RAW_CASES, arrays["raw_model_share"]):
        print(f"  {case}: " + "  ".join(f"{v:.3%}" for v in row))
    print("whole chain (cropped image, pixel_values):")
    for case, row in zip(CHAIN_CASES, arrays["chain_model_share"]):
        print(f"  {case}: " + "  ".join(f"{v:.3%}" for v in row))


if __name__ == "__main__":
    main()
