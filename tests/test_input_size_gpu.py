"""The model driver at input sizes other than 224 x 224 (rn_model_set_input_size): logits against the float64
reference of oracle/netref.py on both stem routes, bf16 against the CPU emulation's own distance, 224 x 224
unchanged bit for bit, independence of batch / part / sub-batch, the byte route, the lifecycle rules and
rn_infer --size."""
import os
import subprocess

import numpy as np
import pytest

import resnet_c_amd as R
from oracle import netref as N
from resnet_c_amd import _lib as L
from resnet_c_amd import preprocess
from test_grouped_host import bottleneck_features_f64

pytestmark = pytest.mark.gpu

TOL = 1e-4  # as test_model_gpu.py
# (32, 32): final map 1 x 1.  (64, 96): fused stem, final map 2 x 3.  (44, 64): stem height 22, pooled height 11,
# the fused stem's last partial item.  (104, 72): stem width 36, unfused; 13 -> 7 and 9 -> 5 under stride 2; 468
# rows per image.  (40, 272): stem width 136 > 128, unfused; final map 2 x 9.
SIZES = [(32, 32), (64, 96), (44, 64), (104, 72), (40, 272)]
FUSED_STEM = {(32, 32): True, (64, 96): True, (44, 64): True, (104, 72): False, (40, 272): False}
B = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def states(state50):
    return {"resnet18": R.weights.generate_state("resnet18", seed=0), "resnet50": state50,
            "resnext50_32x4d": R.weights.generate_state("resnext50_32x4d", seed=0)}


@pytest.fixture(scope="module")
def models(states):
    made = {}

    def get(arch, dtype="f32"):
        if (arch, dtype) not in made:
            made[(arch, dtype)] = R.NativeModel(arch, state=states[arch], dtype=dtype)
        return made[(arch, dtype)]
    yield get
    for m in made.values():
        m.close()


_INPUTS, _REFS = {}, {}


def inputs(size, n=B):
    if (size, n) not in _INPUTS:
        x = R.weights.generate_input(n, seed=100 + size[0] + size[1], hw=size)
        x.setflags(write=False)
        _INPUTS[(size, n)] = x
    return _INPUTS[(size, n)]


def ref_logits(arch, state, size):
    """float64 logits of inputs(size): computed once per (arch, size), shared, never changed"""
    if (arch, size) not in _REFS:
        # netref.features_f64 knows the ResNets; ResNeXt's float64 features are test_grouped_host.py's
        feats = (bottleneck_features_f64 if arch in R.weights.FAMILY else N.features_f64)(arch, state, inputs(size))
        want = N.ref_logits(state, feats)
        want.setflags(write=False)
        _REFS[(arch, size)] = want
    return _REFS[(arch, size)]


def stem_ops(m, x):
    """the ops of a profiled fused forward in front of the first block"""
    m.set_profiling(True)
    try:
        m.forward(x, fused=True)
        recs = m.profile()
    finally:
        m.set_profiling(False)
    return [r["op"] for r in recs if r["layer"] in ("input", "conv1", "conv1+maxpool", "maxpool")]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_logits_vs_fp64(arch, size, states, models):
    m, x, want = models(arch), inputs(size), ref_logits(arch, states[arch], size)
    m.set_input_size(*size)
    assert m.input_size == size
    got = {"fused": m.forward(x, fused=True), "ops": m.forward(x, fused=False)}
    if arch == "resnet50":
        m.set_pair_fusion(False)
        got["fused, pair fusion off"] = m.forward(x, fused=True)
        m.set_pair_fusion(True)
        m.set_chain(False)
        got["fused, chains off"] = m.forward(x, fused=True)
        m.set_chain(True)
        assert np.array_equal(bits(got["fused, chains off"]), bits(got["fused"]))  # chains change no bit
    for what, g in got.items():
        err = float(np.abs(g - want).max())
        print(f"{arch} {size} {what}: max|gpu - fp64| = {err:.3e}")
        assert g.shape == (B, 1000) and err <= TOL, (what, err)
    # the route is the documented one: one fused launch, or stem and max-pool on their own
    ops_seen = stem_ops(m, x)
    assert ("conv2d+epilogue+maxpool" in ops_seen) == FUSED_STEM[size], ops_seen
    assert ("maxpool2d" in ops_seen) == (not FUSED_STEM[size]), ops_seen


def test_resnext_at_104x72(states, models):
    arch, size = "resnext50_32x4d", (104, 72)
    m, x, want = models(arch), inputs(size), ref_logits(arch, states[arch], size)
    m.set_input_size(*size)
    for fused in (True, False):
        err = float(np.abs(m.forward(x, fused=fused) - want).max())
        print(f"{arch} {size} fused={fused}: max|gpu - fp64| = {err:.3e}")
        assert err <= TOL, (fused, err)


def structured(finch, size):
    """Four images with content at `size`: the finch, one of its shifted crops and two low-frequency colour fields
    (images 0, 5, 8, 12 of netref.structured_inputs), resampled to H x W by nearest neighbour.  Images of uniform
    noise will not do here: their pooled features are nearly the same vector, so an fc re-centred and scaled to a
    logit spread of 1 on them magnifies every rounding (the emulation alone lands 0.11-0.25 from float64 on three
    noise images) and no bound below a fifth of the spread exists."""
    x = N.structured_inputs(finch)[[0, 5, 8, 12]]
    ih = np.rint(np.linspace(0, 223, size[0])).astype(int)
    iw = np.rint(np.linspace(0, 223, size[1])).astype(int)
    return np.ascontiguousarray(x[:, :, ih][:, :, :, iw])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bf16_within_the_emulations_distance(size, state50, finch):
    """bf16 storage, resnet50, fc re-centred to a logit spread of 1 (as test_basic_arch_gpu.py).  The bound is
    not a constant: 2.3 times the distance of the CPU emulation of the driver's roundings (oracle/netref.py,
    float64 sums) from the float64 logits on these very inputs -- the room test_basic_arch_gpu.py documents
    for 224 x 224 -- and it must stay below a fifth of the logit spread.  Emulation distances on these inputs:
    0.074 (32 x 32), 0.072 (64 x 96), 0.075 (44 x 64), 0.079 (104 x 72), 0.062 (40 x 272); the GPU's are in
    profiles/input_size/README.md."""
    arch, x = "resnet50", structured(finch, size)
    st, want = N.recentre_fc(state50, N.features_f64(arch, state50, x), spread=1.0)
    emu = N.logits_bf16_emulated(st, N.features_bf16_emulated(arch, st, x))
    dist = float(np.abs(emu - want).max())
    spread = N.logit_spread(want)
    bound = 2.3 * dist
    m = R.NativeModel(arch, state=st, dtype="bf16", input_size=size)
    try:
        got = m.forward(x, fused=True)
    finally:
        m.close()
    err = float(np.abs(got - want).max())
    print(f"bf16 {size}: emulation {dist:.4f}, bound {bound:.4f}, spread {spread:.3f}, gpu {err:.4f}")
    assert bound < spread / 5, (bound, spread)  # otherwise the check says nothing
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_224_is_unchanged_bit_for_bit(dtype, state50, models, finch):
    x = np.concatenate([finch, R.weights.generate_input(1, seed=7)])
    default = models("resnet50", dtype)
    default.set_input_size(224, 224)  # the shared model may come from another size
    want = default.forward(x, fused=True)
    m = R.NativeModel("resnet50", state=state50, dtype=dtype, input_size=(224, 224))
    try:
        assert m.input_size == (224, 224) and m.max_sub_batch() == 512
        assert np.array_equal(bits(m.forward(x, fused=True)), bits(want))
        if dtype == "f32":
            assert np.array_equal(bits(m.forward(x, fused=False)), bits(default.forward(x, fused=False)))
        # the default model's tuning table keeps its format and imports
        xd = R.FloatTensor.from_numpy(x, R.Device.GPU)
        out = R.FloatTensor((2, 1000), R.Device.GPU)
        default.tune(xd.data(), 2, out.data(), True)
        words = default.export_tuning()
        assert words.size == 10 + 4 * (53 + 16)  # the header of before: no size word at 224 x 224
        m.import_tuning(words)
        assert np.array_equal(m.export_tuning(), words)
        assert np.array_equal(bits(m.forward(x, fused=True)), bits(want))
    finally:
        m.close()


@pytest.mark.parametrize("arch,n", [("resnet18", 5), ("resnet50", 129)])
def test_logits_do_not_depend_on_the_split(arch, n, models):
    """(104, 72): B = 5, and B = 129 where two streams (parts of 64 and 65) and a two-slice front really run,
    against B = 1 runs of the same images"""
    size = (104, 72)
    m, x = models(arch), inputs(size, n)
    m.set_input_size(*size)
    alone = {i: m.forward(x[i:i + 1], fused=True) for i in sorted({0, n // 2, n - 1})}
    m.set_streams(2)
    m.set_front_parts(2)
    try:
        assert m.parts(n) == (2 if n >= 128 else 1)
        got = m.forward(x, fused=True)
    finally:
        m.set_streams(0)
        m.set_front_parts(1)
    for i, want in alone.items():
        assert np.array_equal(bits(got[i:i + 1]), bits(want)), i


def test_sub_batch_cap(models):
    m = models("resnet18")
    m.set_input_size(224, 224)
    assert m.max_sub_batch() == 512
    size = (1024, 1024)
    m.set_input_size(*size)
    try:
        # the rule: the largest power of two <= 512 with (largest per-image arena tensor) * cap < 2^29.  At 1024 x
        # 1024 that tensor is the stem's, 512 * 512 * 64 = 2^24 elements (the padded input has 1030 * 1030 * 4, the
        # first stage of a basic-block network 256 * 256 * 64): 32 of them are exactly 2^29, not below it
        largest = max(512 * 512 * 64, 1030 * 1030 * 4, 256 * 256 * 64)
        cap = 512
        while largest * cap >= 1 << 29:
            cap //= 2
        assert cap == 16 and m.max_sub_batch() == cap
        one = R.weights.generate_input(1, seed=11, hw=size)
        want = m.forward(one, fused=True)
        got = m.forward(np.repeat(one, cap + 1, axis=0), fused=True)  # a full sub-batch and one image of the next
        assert got.shape == (cap + 1, 1000)
        assert np.array_equal(bits(got), np.repeat(bits(want), cap + 1, axis=0))
    finally:
        m.set_input_size(224, 224)  # frees the 1024 x 1024 arenas


def test_byte_route(models):
    size = (64, 96)
    px = np.random.default_rng(3).integers(0, 256, (B,) + size + (3,), dtype=np.uint8)
    for arch, dtype in (("resnet18", "f32"), ("resnet50", "bf16")):
        m = models(arch, dtype)
        m.set_input_size(*size)
        want = m.forward(preprocess.normalize_u8(px), fused=True)
        assert np.array_equal(bits(m.forward_u8(px, fused=True)), bits(want)), (arch, dtype)
        out = m.forward_outputs(px, logits=True, features=True)
        assert np.array_equal(bits(out["logits"]), bits(want)) and out["features"].shape == (B, m.features)


def test_lifecycle(states):
    state = states["resnet18"]
    m = R.NativeModel("resnet18", state=state)
    small = (64, 96)
    x224, xs = R.weights.generate_input(2, seed=21), inputs(small)
    try:
        first = m.forward(x224, fused=True)
        bytes224 = m.activation_bytes()
        m.set_input_size(*small)
        assert m.activation_bytes() == 0  # the arenas are gone until the next forward
        want_small = m.forward(xs[:2], fused=True)
        assert 0 < m.activation_bytes() < bytes224 / 4  # 64 * 96 against 224 * 224 pixels, the same batch
        with pytest.raises(AssertionError):
            m.forward(x224)  # the Python surface follows the model
        m.set_input_size(224, 224)
        assert np.array_equal(bits(m.forward(x224, fused=True)), bits(first))
        assert m.activation_bytes() == bytes224

        # out of range: refused, nothing changes
        for bad in [(31, 64), (64, 2049), (0, 0)]:
            with pytest.raises(R.RnError):
                m.set_input_size(*bad)
            assert m.input_size == (224, 224)
        assert np.array_equal(bits(m.forward(x224, fused=True)), bits(first))

        # refused while a graph or a pipeline of the model lives, accepted after they close
        xd = R.FloatTensor.from_numpy(x224, R.Device.GPU)
        out = R.FloatTensor((2, 1000), R.Device.GPU)
        g = R.Graph(m, xd.data(), 2, out.data(), True)
        with pytest.raises(R.RnError):
            m.set_input_size(*small)
        assert m.input_size == (224, 224)
        g.launch()
        m.ctx.sync()
        assert np.array_equal(bits(out.numpy()), bits(first))
        g.close()
        m.set_input_size(*small)
        pipe = R.Pipeline(m, 2, fused=True)
        with pytest.raises(R.RnError):
            m.set_input_size(224, 224)
        assert m.input_size == small and pipe.input_buffer().shape == (2, 3) + small
        pipe.close()
        m.set_input_size(224, 224)

        # tuning tables carry the size
        m.set_input_size(*small)
        xsd = R.FloatTensor.from_numpy(xs[:2], R.Device.GPU)
        m.tune(xsd.data(), 2, out.data(), True)
        t_small = m.export_tuning()
        assert np.array_equal(bits(out.numpy()), bits(want_small))  # tiles change no bit
        m.set_input_size(224, 224)
        with pytest.raises(R.RnError):
            m.export_tuning()  # resizing dropped the tiles
        with pytest.raises(R.RnError):
            m.import_tuning(t_small)
        m.tune(xd.data(), 2, out.data(), True)
        t224 = m.export_tuning()
        assert t_small.size == t224.size + 1
        m.set_input_size(*small)
        with pytest.raises(R.RnError):
            m.import_tuning(t224)
        m.import_tuning(t_small)
        assert np.array_equal(bits(m.forward(xs[:2], fused=True)), bits(want_small))
        m.set_input_size(96, 64)
        with pytest.raises(R.RnError):
            m.import_tuning(t_small)  # 64 x 96 is not 96 x 64

        # decoded images stay at 224 x 224
        img = np.random.default_rng(5).integers(0, 256, (300, 280, 3), dtype=np.uint8)
        with pytest.raises(R.RnError) as e:
            m.forward_images([img])
        assert e.value.status == L.RN_ERR_UNSUPPORTED and "224" in str(e.value)
        with pytest.raises(R.RnError) as e:
            R.Pipeline(m, 2, input="images")
        assert e.value.status == L.RN_ERR_UNSUPPORTED
        m.set_input_size(224, 224)  # the refused pipeline left nothing behind
        assert m.forward_images([img]).shape == (1, 1000)
    finally:
        m.close()


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_pipeline_at_another_size(kind, models):
    """a pipeline sized at (64, 96): two whole batches and a ragged last one give forward's logits"""
    size = (64, 96)
    m = models("resnet18")
    m.set_input_size(*size)
    if kind == "u8":
        x = np.random.default_rng(9).integers(0, 256, (5,) + size + (3,), dtype=np.uint8)
        want = m.forward_u8(x, fused=True)
    else:
        x = inputs(size, 5)
        want = m.forward(x, fused=True)
    pipe = R.Pipeline(m, 2, fused=True, input=kind)
    try:
        got = list(pipe.run([x[0:2], x[2:4], x[4:5]]))
    finally:
        pipe.close()
    assert [g.shape[0] for g in got] == [2, 2, 1]
    assert np.array_equal(bits(np.concatenate(got)), bits(want))


def test_rn_infer_size(states, models, tmp_path):
    size = (64, 96)
    wdir = tmp_path / "weights_bin"
    os.mkdir(wdir)
    R.weights.save_weights_bin(states["resnet18"], str(wdir))
    x = inputs(size, 2)
    good, bad = tmp_path / "in_64x96.bin", tmp_path / "in_224.bin"
    x.tofile(good)
    R.weights.generate_input(2, seed=1).tofile(bad)
    m = models("resnet18")
    m.set_input_size(*size)
    want = m.forward(x, fused=True).argmax(1)
    exe = os.path.join(os.path.dirname(L.LIB_PATH), "rn_infer")
    base = [exe, "--arch", "18", "--weights", str(wdir), "--batch", "2", "--size", "64,96", "--input"]
    r = subprocess.run(base + [str(good)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [int(l.split()[-1]) for l in r.stdout.splitlines() if l.startswith("max index is")] == want.tolist()
    r = subprocess.run(base + [str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "3 x 64 x 96" in r.stderr and "unsupported" in r.stderr, r.stderr
    r = subprocess.run(base[:-3] + ["--size", "16,96", "--input", str(good)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "32..2048" in r.stderr, r.stderr
