from .pixel_set import PixelSet  # noqa: F401
