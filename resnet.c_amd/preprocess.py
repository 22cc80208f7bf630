"""JPEG -> ``test_bins/<stem>.bin`` (raw fp32 [1,3,224,224] NCHW).

Build-owned equivalent of the reference's ``convert_imgs_to_bin.py:12-23``,
which applies torchvision's ``ResNet152_Weights.IMAGENET1K_V1.transforms()``
and dumps the tensor with ``struct.pack('f', ...)``.  torchvision is not
available offline, so the preset is restated with PIL + numpy:

    resize so the short side is 256 (bilinear, PIL's antialiased reducer),
    long side = int(256 * long / short); centre-crop 224x224 with
    round((size - 224) / 2) offsets; uint8 -> fp32 / 255;
    (x - mean) / std with mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225).

The real-weights top-1 of the reference's test image is not recorded anywhere
in the reference, so this restatement is "parity unpinned" against torchvision
itself; what is pinned is every downstream result on the tensor it produces.

The preset is two halves: ``preprocess_image_u8`` (decode, resize, crop: the
[224,224,3] uint8 RGB crop a decoder hands over) and ``normalize_u8`` (the
arithmetic).  The library takes either: the fp32 tensor, or the bytes, which it
normalises on the device to the same bits (rn_image_u8_to_nhwc_pad_dt).
"""
from __future__ import annotations

import os

import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def preprocess_image_u8(path: str, resize: int = 256, crop: int = 224) -> np.ndarray:
    """JPEG -> the [crop,crop,3] uint8 RGB centre crop (no arithmetic on the samples yet)."""
    from PIL import Image

    with Image.open(path) as im:
        im = im.convert("RGB")
        w, h = im.size
        if w <= h:
            nw, nh = resize, int(resize * h / w)
        else:
            nw, nh = int(resize * w / h), resize
        im = im.resize((nw, nh), Image.BILINEAR)
        left = int(round((nw - crop) / 2.0))
        top = int(round((nh - crop) / 2.0))
        im = im.crop((left, top, left + crop, top + crop))
        px = np.asarray(im, dtype=np.uint8)
    return np.ascontiguousarray(px)


def decode_image_u8(path: str) -> np.ndarray:
    """Image file -> [H,W,3] uint8 RGB at the size the file has: the decode and nothing else.  The resize
    and the crop are ``resize_crop_u8``, or the device's (``NativeModel.forward_images``)."""
    from PIL import Image

    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def resize_crop_geometry(h: int, w: int, resize: int = 256, crop: int = 224):
    """(nh, nw, top, left) of the preset: short side to ``resize``, long side truncated, centre crop
    with Python's round (halves to even)."""
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nw, nh = int(resize * w / h), resize
    return nh, nw, int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))


def resize_coefficients(in_size: int, out_size: int, first: int = 0, count=None):
    """PIL's 8-bit bilinear resample of one axis, outputs [first, first + count): (bounds [count,2] of
    (xmin, xmax), coefficients [count,ksize] int32 with 22 fraction bits, ksize).  Doubles, in PIL's
    order of operations."""
    import math

    count = out_size - first if count is None else count
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((count, 2), dtype=np.int32)
    kk = np.zeros((count, ksize), dtype=np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            kk[i, x] = int(0.5 + (w[x] / ww if ww != 0.0 else w[x]) * (1 << 22))
        bounds[i] = (xmin, xmax)
    return bounds, kk, ksize


def _resample_axis0(px: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """One pass along axis 0: out[i] = clip8((2^21 + sum px[xmin + x] * k[i, x]) >> 22), int32."""
    out = np.empty((bounds.shape[0],) + px.shape[1:], dtype=np.uint8)
    for i, (xmin, xmax) in enumerate(bounds):
        acc = np.tensordot(kk[i, :xmax].astype(np.int64), px[xmin:xmin + xmax].astype(np.int64), axes=(0, 0))
        out[i] = np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return out


def resize_crop_u8(px: np.ndarray, resize: int = 256, crop: int = 224) -> np.ndarray:
    """[H,W,3] uint8 RGB of any size -> the [crop,crop,3] centre crop of the image resized so that its
    short side is ``resize``: what ``preprocess_image_u8`` gets from PIL, byte for byte, restated in
    integer numpy.  Horizontal pass first, rounded to 8 bits; the vertical pass runs on that result.
    Only the columns and rows the crop reads are computed.  This is the contract of the device resize
    (rn_image_u8_resize_crop), as ``normalize_u8`` is for the arithmetic."""
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim == 3 and px.shape[2] == 3, (px.dtype, px.shape)
    h, w = px.shape[:2]
    nh, nw, top, left = resize_crop_geometry(h, w, resize, crop)
    assert 0 < crop <= min(nh, nw), (nh, nw, crop)
    hb, hk, _ = resize_coefficients(w, nw, left, crop)
    vb, vk, _ = resize_coefficients(h, nh, top, crop)
    rows = slice(int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1]))      # the source rows the crop's rows touch
    part = px[rows]
    hor = _resample_axis0(np.ascontiguousarray(part.transpose(1, 0, 2)), hb, hk).transpose(1, 0, 2)
    vb = vb.copy()
    vb[:, 0] -= rows.start
    return np.ascontiguousarray(_resample_axis0(np.ascontiguousarray(hor), vb, vk))


def normalize_u8(px: np.ndarray, mean=MEAN, std=STD) -> np.ndarray:
    """uint8 RGB [H,W,3] or [B,H,W,3] -> fp32 NCHW [B,3,H,W]: ``(px / 255 - mean) / std`` in fp32,
    every step correctly rounded.  This is the arithmetic contract of the byte route: the device
    (rn_image_u8_to_nhwc_pad_dt) produces these bits."""
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim in (3, 4) and px.shape[-1] == 3, (px.dtype, px.shape)
    if px.ndim == 3:
        px = px[None]
    x = px.astype(np.float32) / np.float32(255.0)
    x = (x - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2), dtype=np.float32)


def preprocess_image(path: str, resize: int = 256, crop: int = 224) -> np.ndarray:
    return normalize_u8(preprocess_image_u8(path, resize, crop))


def convert_dir(input_dir: str, out_dir: str, u8: bool = False) -> list:
    """Every ``*.jpeg`` in input_dir -> ``out_dir/<stem>.bin`` (fp32 NCHW), or with ``u8``
    ``out_dir/<stem>.u8`` (the 150,528 raw bytes of the RGB crop, what ``rn_infer --u8`` reads);
    returns the paths."""
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for name in sorted(os.listdir(input_dir)):
        if name.endswith(".jpeg") and os.path.isfile(os.path.join(input_dir, name)):
            src = os.path.join(input_dir, name)
            dst = os.path.join(out_dir, os.path.splitext(name)[0] + (".u8" if u8 else ".bin"))
            (preprocess_image_u8(src) if u8 else preprocess_image(src)).tofile(dst)
            written.append(dst)
    return written


def load_bin(path: str, batch: int = 1, hw: int = 224) -> np.ndarray:
    """Read a test_bins file back as [batch,3,hw,hw] (main.cu:236-237)."""
    x = np.fromfile(path, dtype=np.float32)
    return x.reshape(batch, 3, hw, hw)


def load_u8(path: str, batch: int = 1, hw: int = 224) -> np.ndarray:
    """Read a ``.u8`` file back as [batch,hw,hw,3] uint8."""
    return np.fromfile(path, dtype=np.uint8).reshape(batch, hw, hw, 3)
