"""Ground-truth images: decoded 8-bit texels on the device -> the planar fp32 image the loss reads (csrc/image_io.hip).

    decode_u8(path)                                         -> uint8 [H][W][3|4] numpy array, the file's own mode
    image_from_u8(src, height, width, flip, background)     -> float32 [3][height][width] in [0, 1] on src's device

The contract of the kernel is in include/c3dgs_hip.h (c3dgs_image_from_u8); tests/image_ref.py restates it in numpy.
"""
import os

import numpy as np
import torch

from . import _lib


def decode_u8(path):
    """Decode an image file once, on the host, in the file's own mode: RGB or RGBA with 8 bits per channel. Anything else
    (greyscale, palette, 16 bits per channel, ...) raises ValueError naming the file."""
    from PIL import Image
    path = os.fspath(path)
    with Image.open(path) as im:
        raw = getattr(getattr(im, "png", None), "im_rawmode", None) or im.mode     # PIL itself narrows 16-bit RGB PNGs to "RGB"
        if im.mode not in ("RGB", "RGBA") or "16" in str(raw):
            raise ValueError(f"{path}: unsupported image mode {raw!r}: only 8-bit RGB and RGBA images are read")
        a = np.asarray(im, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{path}: decoded to shape {a.shape}, expected [H][W][3|4]")
    return np.ascontiguousarray(a)


def image_from_u8(src, height, width, flip=False, background=None, out=None):
    """src: uint8 [Hs][Ws][C] on the GPU, C in (3, 4). background: None (premultiply onto black) or 3 floats (needs C == 4).
    One launch on the current stream; no host synchronisation."""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3):
        raise ValueError("image_from_u8: src must be a uint8 [H][W][C] GPU tensor")
    src = src.contiguous()
    Hs, Ws, Cn = src.shape
    dev = src.device
    bg = None
    if background is not None:
        bg = torch.as_tensor(background, dtype=torch.float32).to(dev).contiguous()
        if bg.numel() != 3:
            raise ValueError("image_from_u8: background must have 3 elements")
    if out is None:
        out = torch.empty((3, int(height), int(width)), dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (3, height, width)):
        raise ValueError("image_from_u8: out must be a contiguous float32 [3][height][width] GPU tensor")
    with torch.cuda.device(dev):
        rc = _lib.lib().c3dgs_image_from_u8(Hs, Ws, Cn, src.data_ptr(), 1 if flip else 0, bg.data_ptr() if bg is not None else None,
                                            int(height), int(width), out.data_ptr(), _lib.stream(dev))
    _lib.check(rc)
    return out
