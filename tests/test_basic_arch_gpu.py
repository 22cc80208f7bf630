"""ResNet-18 / ResNet-34 through the C model driver (rn_model_create(ctx, &m, 18 | 34)) and the residual
epilogue of the bf16 strip kernels that their conv2 layers need.  The reference ships bottleneck networks
only, so the yardstick here is a BasicBlock forward written with torch.nn.functional in float64."""
import ctypes

import numpy as np
import pytest

import resnet_c_amd as R
from oracle import netref as N
from oracle import oracle as O
from resnet_c_amd import _lib as L
from resnet_c_amd import ops

pytestmark = pytest.mark.gpu

TOL = 1e-4  # as test_model_gpu.py
ARCHS = ["resnet18", "resnet34"]


# ---------------------------------------------------------------------------
# fp64 reference (oracle/netref.py: torchvision BasicBlock semantics, eval-mode batch-norm) and inputs
# ---------------------------------------------------------------------------
ref_features, ref_logits, structured_inputs, top2_gap = N.features_f64, N.ref_logits, N.structured_inputs, N.top2_gap


@pytest.fixture(scope="module", params=ARCHS)
def arch_state(request):
    return request.param, R.weights.generate_state(request.param, seed=0)


@pytest.fixture(scope="module")
def state18():
    return R.weights.generate_state("resnet18", seed=0)


def recentred(arch, state, x):
    """The state with fc re-centred on the fp64 pooled features of x (bias = -W f_mean, W scaled to a
    logit spread of about 1), and the fp64 logits of x under it.  The synthetic fc gives every input the
    same top-1; re-centred, the top-1 follows the image."""
    return N.recentre_fc(state, ref_features(arch, state, x), spread=1.0)


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_key_list_is_the_weights_table(arch):
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, seed=1))
    try:
        keys = m.tensor_keys()
        want = [(k, int(np.prod(s))) for k, s in R.weights.tensor_specs(arch)]
        assert keys == want and len(keys) == {"resnet18": 102, "resnet34": 182}[arch]
    finally:
        m.close()


def test_other_arch_numbers_stay_unsupported():
    lib, ctx = L.lib(), R.get_ctx()
    for arch in (0, 17, 26, 200):
        h = ctypes.c_void_p()
        assert lib.rn_model_create(ctx.handle, ctypes.byref(h), arch) == L.RN_ERR_UNSUPPORTED


def test_logits_vs_fp64_reference(arch_state, finch):
    """B = 2 (the finch and a generated image): op-by-op, fused, fused without pair fusion."""
    arch, state = arch_state
    x = np.concatenate([finch, R.weights.generate_input(1, seed=3)])
    want = ref_logits(state, ref_features(arch, state, x))
    m = R.NativeModel(arch, state=state)
    try:
        ops_mode = m.forward(x, fused=False)
        fused = m.forward(x, fused=True)
        m.set_pair_fusion(False)
        unpaired = m.forward(x, fused=True)
        m.set_pair_fusion(True)
    finally:
        m.close()
    for got in (ops_mode, fused, unpaired):
        assert np.abs(got - want).max() <= TOL
    assert np.abs(fused - unpaired).max() <= 2e-5


def test_top1_follows_the_image(arch_state, finch):
    """A top-1 check that can fail: fc re-centred so that the fp64 reference spreads 16 structured inputs
    over at least 8 classes; the GPU's fp32 top-1 must equal it wherever the reference's top-2 gap exceeds
    10 TOL, in both modes.  bf16: logits within a bound well below the input-dependent logit spread, the
    same top-1 wherever the gap clears twice that bound."""
    arch, state = arch_state
    x = structured_inputs(finch)
    st, want = recentred(arch, state, x)
    top = want.argmax(1)
    assert len(set(top.tolist())) >= 8, top
    sep = top2_gap(want) > 10 * TOL
    assert sep.sum() >= 12
    m = R.NativeModel(arch, state=st)
    try:
        for fused in (False, True):
            got = m.forward(x, fused=fused)
            assert np.abs(got - want).max() <= TOL
            assert np.array_equal(got.argmax(1)[sep], top[sep])
    finally:
        m.close()
    mb = R.NativeModel(arch, state=st, dtype="bf16")
    try:
        got = mb.forward(x, fused=True)
    finally:
        mb.close()
    spread = float((want - want.mean(0)).std())     # about 1 by construction
    # bf16 storage rounds every activation tensor and weight panel (2^-9 relative); a CPU emulation of those
    # roundings lands 0.05-0.065 from the fp64 logits on these inputs: the bound leaves 2.3x room and is still
    # a fraction of the spread that tells the inputs apart
    tol_bf16 = 0.15
    err = np.abs(got - want).max()
    assert spread > 5 * tol_bf16, spread             # the inputs differ by far more than the bound
    assert err <= tol_bf16, (err, spread)
    sep16 = top2_gap(want) > 2 * tol_bf16
    assert sep16.sum() >= 2
    assert np.array_equal(got.argmax(1)[sep16], top[sep16])


@pytest.mark.parametrize("arch,counts", [("resnet18", (20, 20, 17, 8)), ("resnet34", (36, 36, 33, 16))])
def test_profile_accounts_for_every_reference_op(arch, counts, finch):
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, seed=0))
    try:
        m.set_profiling(True)
        m.forward(finch, fused=False)
        recs = m.profile()
    finally:
        m.close()
    count = lambda op: sum(r["op"] == op for r in recs)
    assert (count("conv2d"), count("batchnorm2d"), count("relu"), count("add")) == counts
    assert count("maxpool2d") == count("avgpool2d") == count("linear") == 1
    named = sum(counts) + 3
    assert named == {"resnet18": 68, "resnet34": 124}[arch]
    assert len([r for r in recs if r["layer"] != "input"]) == named
    flops = sum(r["flops"] for r in recs)
    assert abs(flops - R.weights.forward_flops(arch)) < 1.0
    assert abs(flops - {"resnet18": 3.628146688e9, "resnet34": 7.327522816e9}[arch]) < 1.0
    assert all(r["ms"] >= 0 for r in recs)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rescheduling_changes_no_bit(state18, finch, dtype):
    """ResNet-18: batch position, streams, depth-first front, tuning, graph capture, the host pipeline and a
    shard group (device 0 twice) only reschedule the same arithmetic."""
    m = R.NativeModel("resnet18", state=state18, dtype=dtype)
    try:
        x5 = R.weights.generate_input(5, seed=41)
        x5[2] = finch[0]
        base5 = m.forward(x5, fused=True)
        for i in (0, 2, 4):
            assert np.array_equal(m.forward(x5[i:i + 1], fused=True), base5[i:i + 1])
        B = 256
        x = R.weights.generate_input(B, seed=42)
        x[7] = finch[0]
        m.set_streams(1)
        want = m.forward(x, fused=True)
        assert np.array_equal(want[7:8], base5[2:3])
        m.set_streams(2)
        assert m.parts(B) == 2
        assert np.array_equal(m.forward(x, fused=True), want)
        m.set_front_parts(4)
        assert np.array_equal(m.forward(x, fused=True), want)
        m.set_front_parts(1)
        # tuned tiles at a small batch
        xin = R.FloatTensor.from_numpy(x5, R.Device.GPU)
        out = R.FloatTensor((5, 1000), R.Device.GPU)
        m.tune(xin.data(), 5, out.data(), True)
        m.ctx.sync()
        assert np.array_equal(out.numpy(), base5)
        assert np.array_equal(m.forward(x5, fused=True), base5)
        # captured graph
        xd = R.FloatTensor.from_numpy(x[:8], R.Device.GPU)
        o8 = R.FloatTensor((8, 1000), R.Device.GPU)
        g = R.Graph(m, xd.data(), 8, o8.data(), fused=True)
        L.check(L.lib().rn_memset(m.ctx.handle, o8.data(), 0, 8 * 4000), "memset", m.ctx.handle)
        g.launch(); g.launch(); m.ctx.sync()
        assert np.array_equal(o8.numpy(), want[:8])
        g.close()
        # host pipeline
        pipe = R.Pipeline(m, 16, fused=True)
        got = list(pipe.run([x[:16], x[16:32]]))
        pipe.close()
        assert np.array_equal(got[0], want[:16]) and np.array_equal(got[1], want[16:32])
    finally:
        m.close()
    sh = R.ShardedModel([0, 0], "resnet18", state=state18, dtype=dtype)
    try:
        logits, top1 = sh.forward(x[:10], fused=True)
        assert np.array_equal(logits, want[:10])
        assert np.array_equal(top1, want[:10].argmax(1).astype(np.uint64))
    finally:
        sh.close()


def test_weights_dir_and_activation_bytes(state18, finch, tmp_path):
    """torchvision-named weights_bin/ directory through rn_model_load_dir; the arenas are sized for the
    basic-block network (well under ResNet-50's)."""
    R.weights.save_weights_bin(state18, str(tmp_path))
    (tmp_path / "layer1.0.bn1.num_batches_tracked").write_bytes(np.zeros(1, np.int64).tobytes())
    a = R.NativeModel("resnet18", weights_dir=str(tmp_path))
    b = R.NativeModel("resnet18", state=state18)
    try:
        assert np.array_equal(a.forward(finch), b.forward(finch))
        lib = L.lib()
        per_img = lib.rn_model_activation_bytes(a.handle)
        assert per_img == 4 * (230 * 230 * 4 + 2 * 112 * 112 * 64 + 28 * 28 * 128 + 56 * 56 * 64 + 512)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------
# the strip kernels' residual epilogue
# ---------------------------------------------------------------------------
STRIP_RES_CASES = [(3, 20, 20, 64), (1, 6, 6, 64), (2, 56, 56, 64), (5, 7, 61, 64), (4, 1, 9, 64),
                   (37, 28, 28, 64), (256, 56, 56, 64), (3, 12, 12, 128), (1, 6, 6, 128), (2, 28, 28, 128),
                   (5, 7, 29, 128), (4, 1, 9, 128), (41, 14, 14, 128)]


@pytest.mark.parametrize("case", STRIP_RES_CASES)
def test_strip_kernel_residual_epilogue(case):
    """conv_strip_kernel / conv_strip128_kernel with a residual (conv2 of a basic block: bn2 + shortcut +
    ReLU): forced as the strip candidate, the same bits as 4-wave tile candidate 4, and the oracle's values
    on bf16-rounded operands.  The strip kernels alone write debug-stamp slot 10 (tile and wide kernels use
    0-9): the slot proves that the strip kernel ran and the forced candidate did not fall back."""
    from resnet_c_amd.tensor import _DeviceBuffer
    B, H, W, C = case
    x, w = rnd((B, C, H, W), 700 + sum(case)), rnd((C, C, 3, 3), 701 + sum(case)) / np.sqrt(9.0 * C)
    res = rnd((B, C, H, W), 703 + sum(case))
    g = np.random.default_rng(702 + sum(case))
    sc, sh = g.random(C, dtype=np.float32) + 0.5, g.standard_normal(C, dtype=np.float32)
    ctx, lib = R.get_ctx(), L.lib()
    strip = lib.rn_conv_tile_candidates()
    # every contraction kernel stamps its blocks while a buffer is attached: room for any grid a fallback could
    # launch (the smallest tile is 64 x 64, one block per tile; tools/conv_stamps.py sizes it the same way)
    nblk = 1 << 16
    assert -(-B * H * W // 64) * -(-C // 64) <= nblk
    stamps = _DeviceBuffer(ctx, nblk * 16 * 8)

    def slot10():
        v = np.zeros(nblk * 16, np.uint64)
        L.check(lib.rn_memcpy_d2h(ctx.handle, v.ctypes.data, stamps.ptr, v.nbytes), "d2h", ctx.handle)
        return int((v.reshape(nblk, 16)[:, 10] != 0).sum())

    try:
        lib.rn_ctx_set_conv_tile(ctx.handle, 4)
        want = ops.conv2d_nhwc_bf16(x, w, 1, 1, sc, sh, res, True)
        want_norelu = ops.conv2d_nhwc_bf16(x, w, 1, 1, None, None, res, False)
        lib.rn_ctx_set_conv_tile(ctx.handle, strip)
        L.check(lib.rn_memset(ctx.handle, stamps.ptr, 0, nblk * 128), "memset", ctx.handle)
        L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, stamps.ptr), "stamps", ctx.handle)
        got = ops.conv2d_nhwc_bf16(x, w, 1, 1, sc, sh, res, True)
        L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, None), "stamps", ctx.handle)
        ran = slot10()
        got_norelu = ops.conv2d_nhwc_bf16(x, w, 1, 1, None, None, res, False)
    finally:
        lib.rn_ctx_set_debug_stamps(ctx.handle, None)
        lib.rn_ctx_set_conv_tile(ctx.handle, 0)
    assert ran > 0, "the forced strip candidate fell back to another kernel"
    assert np.array_equal(got, want) and np.array_equal(got_norelu, want_norelu)
    assert not np.array_equal(got, ops.conv2d_nhwc_bf16(x, w, 1, 1, sc, sh, None, True))  # the residual counts
    if B * H * W <= 8000:
        y = O.conv2d(ops.bf16_round(x), ops.bf16_round(w), 1, 1)
        ref = np.maximum(y * sc[None, :, None, None] + sh[None, :, None, None] + ops.bf16_round(res), 0)
        assert np.abs(got - ref).max() <= 2 ** -8 * np.abs(ref).max() + 1e-5


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


# ---------------------------------------------------------------------------
# the deferred route on a basic block's op sequence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,stride", [(64, 1), (128, 2)])
def test_deferred_basic_block_matches_the_literal_route(C, stride):
    """conv, bn, relu, conv, bn, [downsample conv, bn], add, relu on NCHW tensors through the reference's
    entry points: deferred (fused launches into the caller's buffers) against literal (one launch per call),
    within the folded batch-norm's 2e-5 of the output's largest magnitude.  3x3 -> 3x3 has no chain kernel:
    the matcher must leave the two convolutions as two launches."""
    B, H = 2, 14
    cin = C if stride == 1 else C // 2
    ho = H // stride
    g = np.random.default_rng(C + stride)
    x = g.standard_normal((B, cin, H, H), dtype=np.float32)
    w1 = (g.standard_normal((C, cin, 3, 3), dtype=np.float32) / np.sqrt(9 * cin)).astype(np.float32)
    w2 = (g.standard_normal((C, C, 3, 3), dtype=np.float32) / np.sqrt(9 * C)).astype(np.float32)
    wd = (g.standard_normal((C, cin, 1, 1), dtype=np.float32) / np.sqrt(cin)).astype(np.float32)

    def bnp():
        return [(g.random(C, dtype=np.float32) + 0.5), g.standard_normal(C, dtype=np.float32) * 0.1,
                g.standard_normal(C, dtype=np.float32) * 0.1, g.random(C, dtype=np.float32) + 0.5]

    p1, p2, pd = bnp(), bnp(), bnp()
    up = lambda a: R.FloatTensor.from_numpy(np.ascontiguousarray(a, dtype=np.float32), R.Device.GPU)
    ctx = R.get_ctx()

    def run(deferred):
        ctx.set_deferred(deferred)
        try:
            D = {k: up(v) for k, v in dict(x=x, w1=w1, w2=w2, wd=wd).items()}
            P1, P2, PD = [up(v) for v in p1], [up(v) for v in p2], [up(v) for v in pd]
            t = R.FloatTensor((B, C, ho, ho), R.Device.GPU)
            y = R.FloatTensor((B, C, ho, ho), R.Device.GPU)
            s = R.FloatTensor((B, C, ho, ho), R.Device.GPU)
            n = B * C * ho * ho

            def call(name, *args):
                L.check(getattr(L.lib(), name)(ctx.handle, *args), name, ctx.handle)

            s0 = ctx.deferred_stats() if deferred else None
            call("rn_conv2d_forward", D["x"].data(), t.data(), D["w1"].data(), 3, stride, 1, ho, ho, B, cin, C, H, H)
            call("rn_batchnorm2d_forward", t.data(), t.data(), *(q.data() for q in P1), B, C, ho * ho)
            call("rn_relu_forward", t.data(), t.data(), n)
            call("rn_conv2d_forward", t.data(), y.data(), D["w2"].data(), 3, 1, 1, ho, ho, B, C, C, ho, ho)
            call("rn_batchnorm2d_forward", y.data(), y.data(), *(q.data() for q in P2), B, C, ho * ho)
            short = D["x"]
            if stride != 1:
                call("rn_conv2d_forward", D["x"].data(), s.data(), D["wd"].data(), 1, stride, 0, ho, ho, B, cin, C, H, H)
                call("rn_batchnorm2d_forward", s.data(), s.data(), *(q.data() for q in PD), B, C, ho * ho)
                short = s
            call("rn_add_forward", y.data(), short.data(), y.data(), n)
            call("rn_relu_forward", y.data(), y.data(), n)
            out = y.numpy().copy()
            if deferred:
                s1 = ctx.deferred_stats()
                assert s1["pending_ops"] == 0
                fused = s1["fused_launches"] - s0["fused_launches"]
                # stride 1: (conv1, bn, relu) and (conv2, bn, add, relu), not one chained launch
                assert fused == 2 if stride == 1 else fused >= 2
            return out
        finally:
            ctx.set_deferred(False)

    literal, deferred = run(False), run(True)
    assert np.abs(deferred - literal).max() <= 2e-5 * max(1.0, float(np.abs(literal).max()))
