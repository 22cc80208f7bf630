"""Byte input, the host side: the two halves of the preprocessing preset (decode + crop to uint8 RGB,
then the arithmetic) and the C-ABI surface of the byte route.  No GPU."""
import os
import re
import subprocess

import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
JPEG = os.path.join(GOLDEN, "ILSVRC2012_val_00004749.jpeg")

NEW_SYMBOLS = ["rn_image_u8_to_nhwc_pad_dt", "rn_model_forward_u8", "rn_pipeline_create_u8",
               "rn_pipeline_input_buffer_u8", "rn_pipeline_submit_u8_n", "rn_shard_forward_u8",
               "rn_shard_stream_open_u8", "rn_shard_stream_buffer_u8", "rn_shard_submit_u8"]


def test_crop_then_normalize_is_the_committed_fixture(finch):
    px = P.preprocess_image_u8(JPEG)
    assert px.shape == (224, 224, 3) and px.dtype == np.uint8 and px.flags["C_CONTIGUOUS"]
    x = P.normalize_u8(px)
    assert x.shape == (1, 3, 224, 224) and x.dtype == np.float32
    assert np.array_equal(x.view(np.uint32), finch.view(np.uint32))
    assert np.array_equal(P.preprocess_image(JPEG).view(np.uint32), finch.view(np.uint32))


def test_normalize_u8_is_the_formula_on_every_sample_value():
    """(px / 255 - mean) / std in numpy fp32, for all 3 x 256 values, bit for bit; batched and
    single images agree; another mean / std goes through."""
    px = np.zeros((16, 16, 3), dtype=np.uint8)
    px[...] = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    got = P.normalize_u8(px)
    assert got.shape == (1, 3, 16, 16)
    v = np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255.0)
    for c in range(3):
        want = (v - np.float32(P.MEAN[c])) / np.float32(P.STD[c])
        assert want.dtype == np.float32
        assert np.array_equal(got[0, c].reshape(-1).view(np.uint32), want.view(np.uint32))
    both = P.normalize_u8(np.stack([px, px[::-1]]))
    assert both.shape == (2, 3, 16, 16) and np.array_equal(both[0], got[0]) and np.array_equal(both[1], got[0][:, ::-1])
    mean, std = (0.5, 0.25, 0.125), (0.5, 2.0, 0.3)
    other = P.normalize_u8(px, mean, std)
    for c in range(3):
        want = (v - np.float32(mean[c])) / np.float32(std[c])
        assert np.array_equal(other[0, c].reshape(-1).view(np.uint32), want.view(np.uint32))


def test_convert_dir_writes_byte_crops_that_round_trip(tmp_path, finch):
    src = tmp_path / "imgs"
    src.mkdir()
    os.symlink(JPEG, src / "finch.jpeg")
    (src / "notes.txt").write_text("not an image")
    written = P.convert_dir(str(src), str(tmp_path / "out"), u8=True)
    assert [os.path.basename(w) for w in written] == ["finch.u8"]
    assert os.path.getsize(written[0]) == 224 * 224 * 3 == 150528
    px = P.load_u8(written[0])
    assert px.shape == (1, 224, 224, 3) and np.array_equal(px[0], P.preprocess_image_u8(JPEG))
    assert np.array_equal(P.normalize_u8(px), finch)
    plain = P.convert_dir(str(src), str(tmp_path / "out"))       # the fp32 form is what it was
    assert [os.path.basename(w) for w in plain] == ["finch.bin"]
    assert np.array_equal(P.load_bin(plain[0]), finch)


def test_byte_route_symbols_are_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rn_[a-z0-9_]+)", out))
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"RN_API\s+int\s+" + name + r"\s*\(", header), f"{name} is not declared in rn_hip.h"
        assert name in exported, f"{name} is not exported by librn_hip.so"
        assert name in L.SIGNATURES and hasattr(lib, name)


def test_python_surface_of_the_byte_route():
    assert callable(R.ops.image_u8_to_nhwc_pad)
    for cls, names in ((R.NativeModel, ("forward_u8", "forward_u8_ptr")),
                       (R.model.Pipeline, ("submit_u8",)),
                       (R.model.ShardedModel, ("forward_u8", "submit_u8"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)
