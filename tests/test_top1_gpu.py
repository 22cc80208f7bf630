"""Top-1 of the bottleneck networks (ResNet-50 / 101 / 152) on inputs that differ, on every route that
prints or returns a class index.

The generated weights give almost every input class 112, so the index checks of the other files cannot
fail on a convolution bug.  Here the fc is re-centred on 16 structured images (oracle/netref.py; W as
generated, bias = -W . mean of the fp64 pooled features): the fp64 reference spreads them over 9 / 10 / 11
classes, and tests/test_discriminative_fixture.py shows on the host that a mid-network convolution bug
moves these logits past the 1e-4 bound.  Every route must then agree with the fp64 logits to 1e-4 (fp32)
and give the fp64 top-1 wherever the fp64 top-2 gap exceeds 10 x 1e-4; bf16 within a bound stated as a
fraction of the input-dependent logit spread."""
import functools
import os
import subprocess

import numpy as np
import pytest

import resnet_c_amd as R
from oracle import netref as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4           # fp32 whole-network bound, as test_model_gpu.py
ARCHS = ["resnet50", "resnet101", "resnet152"]
DEPTH = {"resnet50": 50, "resnet101": 101, "resnet152": 152}

# bf16 against fp64, max |dlogit| / spread.  Measured on the MI355X: 0.087 / 0.067 / 0.080 (ResNet-50 / 101 /
# 152, spreads 0.26 / 0.27 / 0.29); the host emulation of the bf16 storage lands 0.071 from fp64 on ResNet-50.
# The bound leaves 1.7x room and stays below a fifth of the spread that tells the inputs apart.
BF16_FRAC = 0.15
# ResNet-50 bf16 against the host emulation of its roundings, max |dlogit| / spread: measured 0.024 on the
# MI355X, 3.6x closer than fp64.  The bound leaves 3x room and is half of BF16_FRAC.
BF16_EMUL_FRAC = 0.075


@functools.lru_cache(maxsize=None)
def _finch():
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "finch_224.bin"), np.float32).reshape(1, 3, 224, 224)


@functools.lru_cache(maxsize=None)
def _x16():
    return N.structured_inputs(_finch())


@functools.lru_cache(maxsize=None)
def recentred(arch):
    """(generated state, state with the fc re-centred on the 16 images, their fp64 logits under it)"""
    state = R.weights.generate_state(arch, seed=0)
    st, want = N.recentre_fc(state, N.features_f64(arch, state, _x16()))
    return state, st, want


def separated(want, margin):
    """the images whose fp64 top-2 gap exceeds margin; the fixture must keep at least 8 classes and 12 of
    these, or a top-1 check on it would be vacuous"""
    top = want.argmax(1)
    assert len(set(top.tolist())) >= 8, top
    sep = N.top2_gap(want) > margin
    return top, sep


def check_fp32(got, want, label):
    """logits within TOL of fp64, the fp64 top-1 wherever the gap exceeds 10 TOL"""
    top, sep = separated(want, 10 * TOL)
    assert sep.sum() >= 12
    err = float(np.abs(got - want).max())
    print(f"\n{label}: {len(set(top.tolist()))} distinct fp64 classes, max |fp32 - fp64| {err:.2e}")
    assert err <= TOL, (label, err)
    assert np.array_equal(got.argmax(1)[sep], top[sep]), (label, got.argmax(1), top)


def pick_image(want):
    """a structured image whose fp64 top-1 is not 112 (the class of every input under the generated fc),
    with the widest top-2 gap among those"""
    gap, top = N.top2_gap(want), want.argmax(1)
    gap = np.where(top != 112, gap, -1.0)
    i = int(gap.argmax())
    assert top[i] != 112 and gap[i] > 10 * TOL, (top[i], gap[i])
    return i


def max_index_lines(stdout):
    return [int(l.split()[-1]) for l in stdout.splitlines() if l.startswith("max index is")]


# ---------------------------------------------------------------------------
# fp32: the model driver, fused and op by op
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_fp32_top1_follows_the_image(arch):
    _, st, want = recentred(arch)
    m = R.NativeModel(arch, state=st)
    try:
        for fused in (True, False):
            check_fp32(m.forward(_x16(), fused=fused), want, f"{arch} fp32 {'fused' if fused else 'ops'}")
    finally:
        m.close()


# ---------------------------------------------------------------------------
# the reference-shaped op API (createResnet / resnetForward), deferred and literal
# ---------------------------------------------------------------------------
@pytest.fixture()
def dctx():
    ctx = R.get_ctx()
    yield ctx
    ctx.set_deferred(False)
    assert ctx.deferred_stats()["pending_ops"] == 0 and ctx.deferred_stats()["nhwc_buffers"] == 0


@pytest.mark.parametrize("arch", ARCHS)
def test_op_api_deferred_and_literal_top1_follow_the_image(arch, dctx):
    """tests/test_defer_gpu.py's route: one C-ABI call per reference op on NCHW tensors, run literally and
    deferred (fused launches into the caller's buffers); both against fp64, and to 5e-5 of each other"""
    _, st, want = recentred(arch)
    m = R.createResnet(arch, st)
    xd = R.FloatTensor.from_numpy(_x16(), R.Device.GPU)
    dctx.set_deferred(False)
    literal = R.resnetForward(m, xd).numpy().copy()
    dctx.set_deferred(True)
    s0 = dctx.deferred_stats()
    deferred = R.resnetForward(m, xd).numpy().copy()
    assert dctx.deferred_stats()["fused_launches"] > s0["fused_launches"]      # the deferred route ran
    check_fp32(literal, want, f"{arch} op API literal")
    check_fp32(deferred, want, f"{arch} op API deferred")
    assert np.abs(deferred - literal).max() <= 5e-5
    assert np.array_equal(deferred.argmax(1), literal.argmax(1))


# ---------------------------------------------------------------------------
# programs that print 'max index is N': the C++ veneer, rn_infer, the reference's own main
# ---------------------------------------------------------------------------
def _build_veneer(tmp_path):
    exe = str(tmp_path / "resnet_veneer")
    libdir = os.path.dirname(R._lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/include", f"{ROOT}/examples/resnet_veneer.cpp",
                    f"-L{libdir}", "-lrn_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


@pytest.mark.parametrize("arch", ARCHS)
def test_cpp_veneer_top1_follows_the_image(arch, tmp_path):
    """examples/resnet_veneer.cpp (reference-named C++ classes over weights_bin/ written from the re-centred
    state), deferred (its default) and literal: logits against fp64, and the 'max index is N' lines"""
    _, st, want = recentred(arch)
    exe = _build_veneer(tmp_path)
    os.mkdir(tmp_path / "weights_bin")
    R.weights.save_weights_bin(st, str(tmp_path / "weights_bin"))
    _x16().tofile(tmp_path / "input.bin")
    top, sep = separated(want, 10 * TOL)
    for mode, env in (("deferred", {}), ("literal", {"RN_VENEER_LITERAL": "1"})):
        r = subprocess.run([exe, str(DEPTH[arch]), "input.bin", f"logits_{mode}.bin"], cwd=tmp_path,
                           capture_output=True, text=True, timeout=300, env={**os.environ, **env})
        assert r.returncode == 0, r.stderr
        got = np.fromfile(tmp_path / f"logits_{mode}.bin", dtype=np.float32).reshape(16, 1000)
        check_fp32(got, want, f"{arch} C++ veneer {mode}")
        lines = np.array(max_index_lines(r.stdout))
        assert np.array_equal(lines, got.argmax(1))
        assert np.array_equal(lines[sep], top[sep])


@pytest.mark.parametrize("arch", ARCHS)
def test_rn_infer_top1_follows_the_image(arch, tmp_path):
    """rn_infer (plain C over the C-ABI) with --batch 16, fused and op by op: one 'max index is N' line per
    image, the fp64 top-1 wherever the gap exceeds 10 TOL; alone, the picked image that is not class 112"""
    _, st, want = recentred(arch)
    wdir = tmp_path / "weights_bin"
    R.weights.save_weights_bin(st, str(wdir))
    x = _x16()
    x.tofile(tmp_path / "x16.bin")
    i = pick_image(want)
    x[i:i + 1].tofile(tmp_path / "one.bin")
    top, sep = separated(want, 10 * TOL)
    exe = os.path.join(os.path.dirname(R._lib.LIB_PATH), "rn_infer")
    for mode in ("fused", "ops"):
        base = [exe, "--arch", str(DEPTH[arch]), "--weights", str(wdir), "--mode", mode]
        r = subprocess.run(base + ["--input", str(tmp_path / "x16.bin"), "--batch", "16"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = np.array(max_index_lines(r.stdout))
        assert len(lines) == 16 and np.array_equal(lines[sep], top[sep]), (mode, lines, top)
        r = subprocess.run(base + ["--input", str(tmp_path / "one.bin")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert max_index_lines(r.stdout) == [int(top[i])] and top[i] != 112


MAIN_REF = os.path.join(ROOT, "oracle", "_ref", "main_ref")


@pytest.mark.skipif(not os.path.exists(MAIN_REF),
                    reason="oracle/_ref/main_ref is built from the reference tree by `make -C oracle`")
def test_reference_main_top1_follows_the_image(tmp_path):
    """The reference's own program (ResNet-152, weights_bin/ and test_bins/ in its cwd) on the re-centred
    weights and a structured image whose fp64 top-1 is not 112: it must print that class"""
    _, st, want = recentred("resnet152")
    i = pick_image(want)
    os.mkdir(tmp_path / "weights_bin")
    os.mkdir(tmp_path / "test_bins")
    R.weights.save_weights_bin(st, str(tmp_path / "weights_bin"))
    _x16()[i].tofile(tmp_path / "test_bins" / "ILSVRC2012_val_00004749.bin")
    r = subprocess.run([MAIN_REF], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want_top = int(want[i].argmax())
    print(f"\nmain_ref: image {i}, fp64 top-1 {want_top} (gap {N.top2_gap(want)[i]:.2e}); {r.stdout.splitlines()[-1]}")
    assert want_top != 112 and r.stdout.splitlines()[-1] == f"max index is {want_top}", r.stdout


# ---------------------------------------------------------------------------
# bf16 storage, fused
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_bf16_top1_follows_the_image(arch):
    """bf16 logits within BF16_FRAC of the input-dependent logit spread from fp64; the spread is more than
    5x that bound, and the top-1 is fp64's wherever the gap clears twice the bound.  ResNet-50 also against a
    CPU emulation of the driver's bf16 roundings (oracle/netref.py), to BF16_EMUL_FRAC of the spread."""
    state, st, want = recentred(arch)
    m = R.NativeModel(arch, state=st, dtype="bf16")
    try:
        got = m.forward(_x16(), fused=True)
    finally:
        m.close()
    spread = N.logit_spread(want)
    tol = BF16_FRAC * spread
    err = float(np.abs(got - want).max())
    msg = f"\n{arch} bf16: spread {spread:.4f}, max |bf16 - fp64| {err:.4f} = {err / spread:.4f} spread"
    if arch == "resnet50":
        emul = N.logits_bf16_emulated(st, N.features_bf16_emulated(arch, state, _x16()))
        err_e = float(np.abs(got - emul).max())
        msg += (f"; max |bf16 - emulation| {err_e:.4f} = {err_e / spread:.4f} spread "
                f"(emulation - fp64: {np.abs(emul - want).max() / spread:.4f} spread)")
    top, sep = separated(want, 2 * tol)
    print(msg + f"; {int(sep.sum())} images with a gap above twice the bound")
    assert spread > 5 * tol
    assert err <= tol, (err, tol)
    assert sep.sum() >= 4
    assert np.array_equal(got.argmax(1)[sep], top[sep]), (got.argmax(1), top)
    if arch == "resnet50":
        assert err_e <= BF16_EMUL_FRAC * spread, (err_e, spread)
