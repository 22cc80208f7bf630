"""The head (softmax / top-k / model outputs / class count) on the host: the exported surface, the layer
table under rn_model_set_classes, and the contract of the ordering restated in numpy."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rn_softmax_forward", "rn_topk_forward", "rn_softmax_topk_forward", "rn_model_set_classes",
       "rn_model_classes", "rn_model_features", "rn_model_forward_outputs", "rn_model_forward_outputs_u8"]


def test_new_symbols_are_declared_exported_and_typed():
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rn_[a-z0-9_]+)", out))
    for n in NEW:
        assert re.search(r"RN_API[^;(]*?\b%s\s*\(" % n, header), n
        assert n in exported and hasattr(lib, n) and n in L.SIGNATURES, n
    assert "rn_widen_bf16_forward" not in exported and "rn_linear_direct_forward" not in exported  # library-internal
    assert ctypes.sizeof(L.ModelOutputs) == 6 * 8
    for f in ("softmax", "topk", "softmax_topk", "topk_reference", "softmax_reference"):
        assert callable(getattr(ops, f))
    assert "classes" in R.NativeModel.__init__.__code__.co_varnames
    assert isinstance(R.NativeModel.classes, property) and isinstance(R.NativeModel.features, property)


class _HostModel:
    """A model whose context is never used: rn_model_create only keeps the pointer, and the layer table,
    rn_model_set_classes and rn_model_tensor_key are pure host code.  The block stands in for an rn_ctx (zeroed:
    device 0, no stream of its own); calls that would reach the device fail with a status, or, where a device
    exists, run on its default stream."""

    def __init__(self, arch):
        self.ctx = ctypes.create_string_buffer(1 << 16)
        self.h = ctypes.c_void_p()
        assert L.lib().rn_model_create(ctypes.addressof(self.ctx), ctypes.byref(self.h), arch) == L.RN_OK

    def keys(self):
        out, i, n = {}, 0, ctypes.c_uint64()
        while True:
            k = L.lib().rn_model_tensor_key(self.h, i, ctypes.byref(n))
            if k is None:
                return out
            out[k.decode()] = n.value
            i += 1

    def close(self):
        L.lib().rn_model_destroy(self.h)


@pytest.mark.parametrize("arch,feat", [(18, 512), (50, 2048)])
def test_set_classes_resizes_the_fc_entries(arch, feat):
    lib = L.lib()
    m = _HostModel(arch)
    try:
        assert lib.rn_model_classes(m.h) == 1000 and lib.rn_model_features(m.h) == feat
        before = m.keys()
        assert before["fc.weight"] == 1000 * feat and before["fc.bias"] == 1000
        for bad in (0, 65537):
            assert lib.rn_model_set_classes(m.h, bad) == L.RN_ERR_INVALID
            assert lib.rn_model_classes(m.h) == 1000 and m.keys() == before
        assert lib.rn_model_set_classes(m.h, 65536) == L.RN_OK and lib.rn_model_classes(m.h) == 65536
        assert lib.rn_model_set_classes(m.h, 10) == L.RN_OK
        after = m.keys()
        assert lib.rn_model_classes(m.h) == 10
        assert after["fc.weight"] == 10 * feat and after["fc.bias"] == 10
        assert {k: v for k, v in after.items() if not k.startswith("fc.")} == \
               {k: v for k, v in before.items() if not k.startswith("fc.")}
        # the first rn_model_set_tensor fixes the count (whether or not its upload finds a device)
        w = np.zeros(10, dtype=np.float32)
        assert lib.rn_model_set_tensor(m.h, b"fc.bias", w.ctypes.data, 1000) == L.RN_ERR_INVALID  # the old numel
        assert lib.rn_model_set_classes(m.h, 12) == L.RN_OK and lib.rn_model_set_classes(m.h, 10) == L.RN_OK
        lib.rn_model_set_tensor(m.h, b"fc.bias", w.ctypes.data, 10)
        assert lib.rn_model_set_classes(m.h, 1000) == L.RN_ERR_INVALID
        assert lib.rn_model_classes(m.h) == 10 and m.keys() == after
    finally:
        m.close()
    assert lib.rn_model_set_classes(None, 10) == L.RN_ERR_INVALID
    assert lib.rn_model_classes(None) == 0 and lib.rn_model_features(None) == 0


def test_null_context_is_refused_by_the_three_ops():
    """(the other refusals need a context, which needs a device: tests/test_head_gpu.py)"""
    lib = L.lib()
    assert lib.rn_softmax_forward(None, None, None, 1, 10) == L.RN_ERR_INVALID
    assert lib.rn_topk_forward(None, None, None, None, 1, 10, 1) == L.RN_ERR_INVALID
    assert lib.rn_softmax_topk_forward(None, None, None, None, None, 1, 10, 1) == L.RN_ERR_INVALID
    assert lib.rn_model_forward_outputs(None, None, 1, None, L.RN_FWD_FUSED) == L.RN_ERR_INVALID


def _order_by_definition(row, k):
    """(v_i, i) precedes (v_j, j) when v_i > v_j, or v_i == v_j and i < j: a selection sort on that rule."""
    left, out = list(range(len(row))), []
    for _ in range(k):
        best = left[0]
        for i in left[1:]:
            if row[i] > row[best] or (row[i] == row[best] and i < best):
                best = i
        out.append(best)
        left.remove(best)
    return out


def test_contract_in_numpy_is_the_stable_argsort():
    g = np.random.default_rng(5)
    rows = [g.standard_normal(40).astype(np.float32),
            g.integers(0, 4, 64).astype(np.float32),                    # four distinct values: many ties
            np.full(17, 2.5, np.float32),                               # constant
            np.array([0.0, -0.0, 0.0, -0.0, -1.0, 1.0], np.float32),    # -0.0 == +0.0: the index decides
            np.array([-np.inf, 3.0, -np.inf, 3.0, np.inf], np.float32)]
    for row in rows:
        for k in (1, 2, 5, len(row)):
            k = min(k, len(row))
            val, idx = ops.topk_reference(row[None], k)
            assert idx[0].tolist() == _order_by_definition(row, k)
            assert np.array_equal(idx[0], np.argsort(-row, kind="stable")[:k])
            assert np.array_equal(val[0].view(np.uint32), row[idx[0]].view(np.uint32))   # the element's own bits
    zeros = np.array([-0.0, 0.0, -0.0], np.float32)
    val, idx = ops.topk_reference(zeros[None], 3)
    assert idx[0].tolist() == [0, 1, 2] and np.signbit(val[0]).tolist() == [True, False, True]
    # k = 1 is the host argmax of the reference's main() (strict '<': the first maximum wins)
    for row in rows:
        assert ops.topk_reference(row[None], 1)[1][0, 0] == R.model.argmax(row[None])[0]


def test_softmax_reference_and_the_fp32_restatement_stay_inside_the_gpu_tests_bound():
    """|p - p64| <= 2e-5 p64 + 1e-9 for a plain numpy fp32 softmax (max, exp, sum, divide in fp32) of the
    kinds of rows tests/test_head_gpu.py uses: the bound is reachable by fp32 arithmetic."""
    g = np.random.default_rng(11)
    rows = [g.standard_normal((3, 1000)).astype(np.float32), 10 * g.standard_normal((3, 4097)).astype(np.float32),
            (g.standard_normal((2, 65536)) + 1e4).astype(np.float32), np.linspace(-80, 0, 1001, dtype=np.float32)[None]]
    masked = g.standard_normal((2, 129)).astype(np.float32)
    masked[:, ::3] = -np.inf
    for x in rows + [masked]:
        p64 = ops.softmax_reference(x)
        e = np.exp(x - x.max(axis=1, keepdims=True), dtype=np.float32)
        p32 = e / e.sum(axis=1, keepdims=True, dtype=np.float32)
        assert np.all(np.abs(p32 - p64) <= 2e-5 * p64 + 1e-9)
        assert np.all(np.abs(p64.sum(axis=1) - 1) < 1e-12)
        assert np.all(p64[np.isneginf(x)] == 0)
