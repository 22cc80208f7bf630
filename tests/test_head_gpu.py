"""The head on the device: rn_topk_forward / rn_softmax_forward / rn_softmax_topk_forward against their
contract, rn_model_forward_outputs against the op entry points and float64, and models whose class count
is not 1000 (rn_model_set_classes)."""
import ctypes

import numpy as np
import pytest

import resnet_c_amd as R
from oracle import netref as N
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd import preprocess as P
import views as V

pytestmark = pytest.mark.gpu

TOL = 1e-4       # logits against float64: tests/test_basic_arch_gpu.py, tests/test_model_gpu.py
CLASSES = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 1001, 4096, 4097, 65536]
KS = [1, 2, 5, 64]
BMAX = 257
N_SPECIAL = 12


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tie_rows(C, seed):
    """[257, C] N(0, 1) rows; the first N_SPECIAL carry the ties the ordering must resolve by index (each as far
    as C has room for it)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((BMAX, C)).astype(np.float32)
    top = np.float32(9.0)
    x[0] = 1.25                                             # a constant row
    x[1, [0, C - 1]] = top                                  # the maximum at both ends
    if C > 64:
        x[2, [63, 64]] = top                                # across the first two waves' lanes
    for r, lane in ((3, 0), (4, 5), (5, 63)):               # the same lane of a thread's first two elements
        if C > lane + 64:
            x[r, [lane, lane + 64]] = top
    x[6, g.permutation(C)[:min(C, 70)]] = top               # more than k copies of the maximum (k <= 64)
    x[7] = g.integers(0, 4, C).astype(np.float32)           # four distinct values
    x[8] = g.integers(0, 4, C).astype(np.float32) - 2.0
    x[9, g.random(C) < 0.5] = -np.inf                       # masked classes
    x[10] = -np.abs(x[10]) - 1.0                            # +0.0 / -0.0 as the two largest, -0.0 first
    if C >= 2:
        x[10, C // 2], x[10, C - 1] = -0.0, 0.0
    x[11, :] = -np.inf                                      # nothing but masked classes, one survivor
    x[11, C // 3] = -3.0
    return x


@pytest.mark.parametrize("C", CLASSES)
def test_topk_is_the_stable_argsort(C):
    """Indices and values bit-equal to np.argsort(-x, kind="stable") of the same fp32 rows, for every k in
    {1, 2, 5, 64} (clipped to the class count) and B in {1, 3, 257}: the B = 1 and B = 3 launches run on the
    tie rows one by one and three by three, so every tie meets every B.  The reference is computed once."""
    x = tie_rows(C, 100 + C)
    order = np.argsort(-x, axis=1, kind="stable")[:, :min(64, C)]
    for k in sorted({min(k, C) for k in KS}):
        want_i = order[:, :k]
        want_v = np.take_along_axis(x, want_i, axis=1)
        launches = [slice(0, BMAX)] + [slice(r, r + 3) for r in range(0, N_SPECIAL, 3)] + \
                   [slice(r, r + 1) for r in range(N_SPECIAL)]
        for rows in launches:
            val, idx = ops.topk(x[rows], k)
            assert np.array_equal(idx, want_i[rows]), (C, k, rows)
            assert np.array_equal(bits(val), bits(want_v[rows])), (C, k, rows)
        if k == 1:
            assert np.array_equal(ops.argmax(x), want_i[:, 0])
            assert np.array_equal(ops.topk(x, 1)[1][:, 0], ops.argmax(x))


def run_view(name, x, k, offs, inplace=False, probs=True):
    """One call of a head entry point on offset views between guard bands; returns (probs, values, indices)."""
    B, C = x.shape
    what = f"{name} {x.shape} k={k} offs={offs}"
    vx = V.place(x, offs.get("x", 0))
    vp = vx if inplace else (V.place_out(x.nbytes, offs.get("probs", 0)) if probs else None)
    vv = V.place_out(B * k * 4, offs.get("values", 0)) if k else None
    vi = V.place_out(B * k * 8, offs.get("indices", 0)) if k else None
    if name == "rn_softmax_forward":
        V.must(name, vx.ptr, vp.ptr, B, C)
    elif name == "rn_topk_forward":
        V.must(name, vx.ptr, vv.ptr, vi.ptr, B, C, k)
        vp = None
    else:
        V.must(name, vx.ptr, vp.ptr if vp else None, vv.ptr, vi.ptr, B, C, k)
    if not inplace:
        V.check_guards(what, vx)
    return (V.fetch(vp, np.float32, what).reshape(B, C) if vp else None,
            V.fetch(vv, np.float32, what).reshape(B, k) if k else None,
            V.fetch(vi, np.uint64, what).astype(np.int64).reshape(B, k) if k else None)


@pytest.mark.parametrize("C,k", [(129, 5), (1001, 64), (4097, 2)])
def test_offset_views_and_guard_bands(C, k):
    """Float operands on 4-byte-only boundaries (+4, +12), the indices on an 8-byte-only one (+8): the same
    bits as on 16-byte boundaries, and not a byte outside the outputs."""
    x = tie_rows(C, 7 + C)[:5]
    base = run_view("rn_softmax_topk_forward", x, k, {})
    assert np.array_equal(base[2], np.argsort(-x, axis=1, kind="stable")[:, :k])
    for offs in ({"x": 4, "probs": 12, "values": 4, "indices": 8}, {"x": 12}, {"probs": 4}, {"values": 12},
                 {"indices": 8}):
        got = run_view("rn_softmax_topk_forward", x, k, offs)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, base)), offs
        _, tv, ti = run_view("rn_topk_forward", x, k, offs)
        assert np.array_equal(ti, base[2]) and np.array_equal(bits(tv), bits(np.take_along_axis(x, ti, axis=1)))
        sp, _, _ = run_view("rn_softmax_forward", x, 0, offs)
        assert np.array_equal(bits(sp), bits(base[0])), offs
        ip, _, _ = run_view("rn_softmax_forward", x, 0, offs, inplace=True)
        assert np.array_equal(bits(ip), bits(base[0])), offs


def test_refusals_launch_nothing():
    ctx, lib = R.get_ctx(), L.lib()
    x = np.zeros((2, 10), np.float32)
    vx, vp = V.place(x), V.place_out(x.nbytes)
    vv, vi = V.place_out(2 * 3 * 4), V.place_out(2 * 3 * 8)
    n0 = lib.rn_ctx_launch_count(ctx.handle)
    bad = [("rn_softmax_forward", (None, vp.ptr, 2, 10), "logits"), ("rn_softmax_forward", (vx.ptr, None, 2, 10), "probs"),
           ("rn_softmax_forward", (vx.ptr, vp.ptr, 2, 0), "classes"), ("rn_softmax_forward", (vx.ptr, vp.ptr, 2, 65537), "classes"),
           ("rn_softmax_forward", (vx.ptr + 2, vp.ptr, 2, 10), "4-byte"),
           ("rn_topk_forward", (vx.ptr, vv.ptr, vi.ptr, 2, 10, 0), "k"), ("rn_topk_forward", (vx.ptr, vv.ptr, vi.ptr, 2, 10, 11), "k"),
           ("rn_topk_forward", (vx.ptr, vv.ptr, vi.ptr, 2, 100, 65), "k"), ("rn_topk_forward", (vx.ptr, vv.ptr, vi.ptr + 4, 2, 10, 3), "8-byte"),
           ("rn_topk_forward", (vx.ptr, None, vi.ptr, 2, 10, 3), "values"), ("rn_topk_forward", (vx.ptr, vv.ptr, None, 2, 10, 3), "indices"),
           ("rn_softmax_topk_forward", (vx.ptr, vp.ptr, None, vi.ptr, 2, 10, 3), "topk_prob"),
           ("rn_softmax_topk_forward", (vx.ptr, vp.ptr, vv.ptr, None, 2, 10, 3), "topk_idx"),
           ("rn_softmax_topk_forward", (vx.ptr, vp.ptr, vv.ptr, vi.ptr + 4, 2, 10, 3), "8-byte"),
           ("rn_softmax_topk_forward", (vx.ptr, vp.ptr, vv.ptr, vi.ptr, 2, 10, 11), "k")]
    for name, args, word in bad:
        st, msg = V.call(name, *args)
        assert st == L.RN_ERR_INVALID and word in msg and name in msg, (name, args, msg)
    for name, args in (("rn_softmax_forward", (None, None, 0, 10)), ("rn_topk_forward", (None, None, None, 0, 10, 3)),
                       ("rn_softmax_topk_forward", (None, None, None, None, 0, 10, 3))):
        assert V.call(name, *args)[0] == L.RN_OK                      # B == 0
    assert lib.rn_ctx_launch_count(ctx.handle) == n0
    for v in (vx, vp, vv, vi):
        V.assert_untouched(v)
    V.must("rn_softmax_topk_forward", vx.ptr, vp.ptr, vv.ptr, vi.ptr, 2, 10, 3)
    assert lib.rn_ctx_launch_count(ctx.handle) == n0 + 1                # one launch, counted


def softmax_inputs():
    g = np.random.default_rng(21)
    out = []
    for C in (1, 2, 63, 65, 1000, 4096, 4097, 65536):
        for scale in (1.0, 10.0):
            out.append((scale * g.standard_normal((3, C))).astype(np.float32))
    out.append((g.standard_normal((2, 1000)) + 1e4).astype(np.float32))          # a naive exp overflows
    out.append((g.standard_normal((2, 5000)) + 1e4).astype(np.float32))
    out.append(np.stack([np.linspace(-80, 0, 1001), np.linspace(0, -80, 1001)]).astype(np.float32))
    out.append(np.linspace(-80, 0, 4099, dtype=np.float32)[None])
    for C in (129, 4200):
        m = g.standard_normal((3, C)).astype(np.float32)
        m[:, ::3] = -np.inf
        out.append(m)
    return out


def test_softmax_against_float64():
    """|p - p64| <= 2e-5 p64 + 1e-9 and |sum - 1| <= 1e-5, p64 the float64 softmax of the same fp32 logits.
    2e-5: x - max rounds to at most 2^-24 * 88 = 5.2e-6 absolute before the result underflows (the same
    relative error in exp), expf is within 2 ulp (2.4e-7), a sum of at most 65536 non-negative terms by tree
    or wave reduction adds at most 17 * 2^-24 = 1e-6, the division 6e-8: below 7e-6, with a 3x margin; 1e-9
    covers flushed subnormals.  A plain numpy fp32 softmax of these kinds of rows stays inside the bound
    (tests/test_head_host.py checks that on the host).  -inf entries give exactly 0; in place gives the same
    bits."""
    for x in softmax_inputs():
        p64 = ops.softmax_reference(x)
        got = ops.softmax(x)
        err = np.abs(got - p64) - (2e-5 * p64 + 1e-9)
        print(f"softmax {x.shape}: max |p - p64| / p64 = {np.max(np.abs(got - p64) / np.maximum(p64, 1e-30)):.3e}, "
              f"max |sum - 1| = {np.abs(got.astype(np.float64).sum(1) - 1).max():.3e}")
        assert np.all(err <= 0), (x.shape, float(err.max()))
        assert np.all(np.abs(got.astype(np.float64).sum(axis=1) - 1) <= 1e-5)
        assert np.all(got[np.isneginf(x)] == 0)
        inplace, _, _ = run_view("rn_softmax_forward", x, 0, {}, inplace=True)
        assert np.array_equal(bits(inplace), bits(got))


@pytest.mark.parametrize("C", [5, 1000, 4097])
def test_fused_ranks_by_logit_and_shares_the_probabilities(C):
    g = np.random.default_rng(31 + C)
    x = (3 * g.standard_normal((4, C))).astype(np.float32)
    # row 0: two distinct logits whose probabilities are equal -- exp(-1e-8) rounds to exp(0) = 1 -- with the
    # SMALLER logit at the lower index: ranked by probability (ties by index) it would come first
    x[0] = -np.abs(x[0]) - 2.0
    x[0, 0], x[0, C - 1] = np.float32(-1e-8), np.float32(0.0)
    k = min(5, C)
    tv, ti = ops.topk(x, k)
    soft = ops.softmax(x)
    fp, fi, probs = ops.softmax_topk(x, k, return_probs=True)
    fp2, fi2 = ops.softmax_topk(x, k)                      # probs == NULL
    assert soft[0, 0] == soft[0, C - 1] and x[0, 0] != x[0, C - 1]
    assert fi[0, :2].tolist() == [C - 1, 0]
    assert np.array_equal(fi, ti) and np.array_equal(fi2, ti)
    assert np.array_equal(fi, np.argsort(-x, axis=1, kind="stable")[:, :k])
    assert np.array_equal(bits(probs), bits(soft))
    assert np.array_equal(bits(fp), bits(np.take_along_axis(probs, fi, axis=1)))
    assert np.array_equal(bits(fp2), bits(fp))


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
def make_state(arch, classes, seed):
    """Every tensor of `arch` with a `classes`-row classifier, drawn from np.random.default_rng(seed) in
    weights.generate_tensor's ranges (He-uniform convolutions, batch-norm gamma and variance in [0.5, 1.5),
    beta and mean in +-0.1, a damped last batch-norm per block, fc in +-1/sqrt(in))."""
    g = np.random.default_rng(seed)
    last_bn = ".bn2." if R.weights.block_kind(arch) == "basic" else ".bn3."
    u = lambda lo, hi, shape: g.uniform(lo, hi, shape).astype(np.float32)
    st = {}
    for key, shape in R.weights.tensor_specs(arch):
        if key.startswith("fc."):
            shape = (classes,) + tuple(shape[1:])
            bound = 1.0 / np.sqrt(R.weights.feature_width(arch))
            st[key] = u(-bound, bound, shape)
        elif len(shape) == 4:
            bound = np.sqrt(6.0 / (shape[1] * shape[2] * shape[3]))
            st[key] = u(-bound, bound, shape)
        elif key.endswith("running_var"):
            st[key] = u(0.5, 1.5, shape)
        elif key.endswith("weight"):
            st[key] = u(0.02, 0.1, shape) if last_bn in key else u(0.5, 1.5, shape)
        else:
            st[key] = u(-0.1, 0.1, shape)
    return st


@pytest.fixture(scope="module")
def x3():
    return R.weights.generate_input(3, seed=77)


@pytest.fixture(scope="module")
def default18(x3):
    state = make_state("resnet18", 1000, 1)
    feats = N.features_f64("resnet18", state, x3)
    return state, feats


def test_model_outputs_default(default18, x3):
    """resnet18, 1000 classes, B = 3, fp32, both modes."""
    state, f64 = default18
    want = N.ref_logits(state, f64)
    m = R.NativeModel("resnet18", state=state)
    try:
        assert m.classes == 1000 and m.features == 512
        for fused in (True, False):
            base = m.forward(x3, fused=fused)
            o = m.forward_outputs(x3, logits=True, features=True, probs=True, topk=5, fused=fused)
            assert np.array_equal(bits(o["logits"]), bits(base))
            assert np.abs(base - want).max() <= TOL
            fp, fi, probs = ops.softmax_topk(base, 5, return_probs=True)
            assert np.array_equal(bits(o["probs"]), bits(probs)) and np.array_equal(bits(o["probs"]), bits(ops.softmax(base)))
            assert np.array_equal(o["topk_idx"], fi) and np.array_equal(o["topk_idx"], ops.topk(base, 5)[1])
            assert np.array_equal(bits(o["topk_prob"]), bits(fp))
            f = o["features"].astype(np.float64)
            assert np.abs(N.ref_logits(state, f) - base).max() <= TOL
            assert np.abs(f - f64).max() <= TOL * np.abs(f64).max()
            # the logits left out: they go to the model's own buffer, the other outputs keep their bits
            q = m.forward_outputs(x3, logits=False, probs=True, topk=5, fused=fused)
            assert "logits" not in q and np.array_equal(bits(q["probs"]), bits(o["probs"]))
            assert np.array_equal(q["topk_idx"], o["topk_idx"]) and np.array_equal(bits(q["topk_prob"]), bits(o["topk_prob"]))
            p = m.forward_outputs(x3, logits=False, probs=True, fused=fused)          # k == 0: rn_softmax_forward
            assert list(p) == ["probs"] and np.array_equal(bits(p["probs"]), bits(o["probs"]))
            only_f = m.forward_outputs(x3, logits=False, features=True, fused=fused)
            assert np.array_equal(bits(only_f["features"]), bits(o["features"]))
        with pytest.raises(L.RnError) as e:
            m.forward_outputs(x3, logits=False)                                        # nothing to write
        assert e.value.status == L.RN_ERR_INVALID
        with pytest.raises(L.RnError):
            m.forward_outputs(x3, topk=65)
        # profile: the launches of a forward, then the head's
        m.set_profiling(True)
        m.forward(x3)
        plain = [(r["op"], r["layer"]) for r in m.profile()]
        m.forward_outputs(x3, features=True, probs=True, topk=5)
        recs = [(r["op"], r["layer"]) for r in m.profile()]
        m.forward_outputs(x3, probs=True)
        recs0 = [(r["op"], r["layer"]) for r in m.profile()]
        m.set_profiling(False)
        assert recs == plain + [("features", "head"), ("softmax_topk", "head")]
        assert recs0 == plain + [("softmax", "head")]
    finally:
        m.close()


def test_model_outputs_u8_route(default18):
    state, _ = default18
    px = np.random.default_rng(5).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    m = R.NativeModel("resnet18", state=state)
    try:
        a = m.forward_outputs(px, features=True, probs=True, topk=5)
        b = m.forward_outputs(P.normalize_u8(px), features=True, probs=True, topk=5)
        assert np.array_equal(bits(a["logits"]), bits(m.forward_u8(px)))
    finally:
        m.close()
    assert sorted(a) == sorted(b) == ["features", "logits", "probs", "topk_idx", "topk_prob"]
    for key in a:
        assert np.array_equal(a[key].view(np.uint32 if a[key].dtype == np.float32 else np.int64),
                              b[key].view(np.uint32 if b[key].dtype == np.float32 else np.int64)), key


def test_model_outputs_bf16(default18, x3):
    """bf16 storage.  The features are the bf16 pooled values, widened exactly.  The logits are the bf16 model's
    classifier on exactly those features -- bf16-rounded fc.weight (oracle.netref.logits_bf16_emulated's rule)
    times the features plus the fp32 bias, in float64 -- within the fp32 bound TOL: the emulation of the head
    has no rounding of its own left.  The features against float64: ResNet-18's deepest path stores 20 tensors
    (stem + pool, 16 block convolutions ... the average pool), each rounded to bf16 at 2^-9 of its magnitude,
    and the damped last batch-norm of a block keeps the residual stream O(1), so at most 20 * 2^-9 of the
    largest feature.  (The existing whole-network bf16 bound, 0.15 at a logit spread of 1, is tied to fc
    re-centred on 16 structured inputs; it says nothing about three generated images.)"""
    state, f64 = default18
    m = R.NativeModel("resnet18", state=state, dtype="bf16")
    try:
        base = m.forward(x3)
        o = m.forward_outputs(x3, features=True, probs=True, topk=5)
    finally:
        m.close()
    assert np.array_equal(bits(o["logits"]), bits(base))
    assert np.array_equal(bits(o["features"]), bits(ops.bf16_round(o["features"])))
    emul = N.logits_bf16_emulated(state, o["features"].astype(np.float64))
    print(f"bf16: max |logits - fc(features)| = {np.abs(base - emul).max():.3e}, "
          f"max |features - f64| / max |f64| = {np.abs(o['features'] - f64).max() / np.abs(f64).max():.3e}")
    assert np.abs(base - emul).max() <= TOL
    assert np.abs(o["features"] - f64).max() <= 20 * 2.0 ** -9 * np.abs(f64).max()
    fp, fi, probs = ops.softmax_topk(base, 5, return_probs=True)
    assert np.array_equal(bits(o["probs"]), bits(probs)) and np.array_equal(o["topk_idx"], fi)
    assert np.array_equal(bits(o["topk_prob"]), bits(fp))


@pytest.mark.parametrize("arch,classes", [("resnet18", 10), ("resnet18", 1001), ("resnet50", 8)])
def test_class_count_against_float64(arch, classes, x3):
    state = make_state(arch, classes, 2)
    want = N.ref_logits(state, N.features_f64(arch, state, x3))     # netref's features, a float64 matmul
    m = R.NativeModel(arch, state=state)                             # classes from fc.weight's rows
    try:
        assert m.classes == classes and dict(m.tensor_keys())["fc.weight"] == classes * m.features
        for fused in (True, False):
            got = m.forward(x3, fused=fused)
            assert got.shape == (3, classes)
            print(f"{arch} classes={classes} fused={fused}: max |logits - f64| = {np.abs(got - want).max():.3e}")
            assert np.abs(got - want).max() <= TOL
        k = min(5, classes)
        o = m.forward_outputs(x3, probs=True, topk=k)
        assert np.array_equal(bits(o["logits"]), bits(m.forward(x3)))
        assert np.array_equal(o["topk_idx"], np.argsort(-o["logits"], axis=1, kind="stable")[:, :k])
        assert L.lib().rn_model_set_classes(m.handle, 1000) == L.RN_ERR_INVALID      # after finalize
        assert m.classes == classes
    finally:
        m.close()


def test_ten_classes_on_two_streams_and_through_the_pipeline():
    """B = 130, 10 classes, two streams: the second part's logits start 65 * 40 bytes in, off a 16-byte
    boundary.  Every image's logits are those of the image alone."""
    state = make_state("resnet18", 10, 3)
    x = R.weights.generate_input(130, seed=9)
    m = R.NativeModel("resnet18", state=state)
    try:
        m.set_streams(2)
        assert m.parts(130) == 2
        got = m.forward(x)
        assert got.shape == (130, 10)
        for i in (0, 1, 64, 65, 66, 129):
            assert np.array_equal(bits(m.forward(x[i:i + 1])), bits(got[i:i + 1])), i
        pipe = R.Pipeline(m, 4)
        try:
            pipe.submit(x[:4])
            pipe.submit(x[64:67])
            l0, t0 = pipe.collect_top1()
            l1 = pipe.collect()
        finally:
            pipe.close()
        assert l0.shape == (4, 10) and l1.shape == (3, 10)
        assert np.array_equal(bits(l0), bits(got[:4])) and np.array_equal(bits(l1), bits(got[64:67]))
        assert np.array_equal(t0.astype(np.int64), R.model.argmax(l0)) and np.array_equal(t0.astype(np.int64), ops.argmax(l0))
    finally:
        m.close()


def test_bf16_refuses_a_class_count_that_is_no_multiple_of_four():
    """(documented next to rn_model_set_classes: the bf16 classifier cannot write rows off a 16-byte boundary)"""
    with pytest.raises(L.RnError) as e:
        R.NativeModel("resnet18", state=make_state("resnet18", 10, 4), dtype="bf16")
    assert e.value.status == L.RN_ERR_UNSUPPORTED
    m = R.NativeModel("resnet18", state=make_state("resnet18", 12, 4), dtype="bf16")
    try:
        assert m.forward(R.weights.generate_input(2, seed=1)).shape == (2, 12)
    finally:
        m.close()
