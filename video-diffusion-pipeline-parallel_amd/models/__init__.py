"""Models behind the pipeline's ``model(latent, step)`` protocol (ref ``src/models/__init__.py``)."""

from .dummy_unet import DummyUNet

__all__ = ["DummyUNet", "StableVideoUNet", "VideoConditioning"]


def __getattr__(name):  # lazy: svd_unet pulls in the HIP binding
    if name in ("StableVideoUNet", "VideoConditioning"):
        from . import svd_unet
        return getattr(svd_unet, name)
    raise AttributeError(name)
