"""What a deferred context (rn_ctx_set_deferred, rn_defer.hip) leaves behind, on the host: every program, input and
parameter update test_defer_state_gpu.py runs is built here -- each shape and seed in one place, cached, so the GPU file
runs what this file vetted -- and the oracle alone is run on it.  What is asserted are the CONDITIONS under which the
GPU cases can tell right from wrong: an output read in the wrong layout is far from the output, an output computed
from a stale fold or panel is far from the one computed from the updated parameter.  No GPU.
profiles/defer_state/README.md lists which case is there for which path."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

F = np.float32


def cached(fn):
    """one computation per argument tuple for both files; the arrays are shared and never written to"""
    return functools.lru_cache(maxsize=None)(fn)


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape, dtype=F) * F(scale)).astype(F)


def bn_params(C, seed):
    g = np.random.default_rng(seed)
    return (g.random(C, dtype=F) + F(0.5), g.standard_normal(C, dtype=F) * F(0.1),
            g.standard_normal(C, dtype=F) * F(0.1), g.random(C, dtype=F) + F(0.5))


def bound(want, terms):
    """the value bound of test_defer_gpu.test_fused_chain_against_the_oracle; terms = Cin * k * k of the convolution"""
    return 3e-6 * np.sqrt(terms) * float(np.abs(want).max()) + 1e-5


def nhwc_image(y):
    """what a buffer holds while the route keeps tensor y in it as NHWC, under y's own (NCHW) shape"""
    return np.ascontiguousarray(y.transpose(0, 2, 3, 1)).reshape(y.shape)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# =====================================================================================================================
# 1. The programs.  A program is a list of steps over named buffers, so that the oracle (run_host) and a context
#    (test_defer_state_gpu.record) run the same calls:
#        ("conv", in, out, weight, k, stride, pad)   ("bn", t, prefix)   ("add", t, residual)   ("relu", t)
#        ("maxpool", in, out, k, stride, pad)
#    bn / add / relu are in place on t, as the reference's callers write them (main.cu:127-166).
# =====================================================================================================================
NAMES = ("fold", "panel", "plain", "exact", "stem", "chain")


def _bn_into(params, prefix, C, seed):
    for key, v in zip("wbmv", bn_params(C, seed)):
        params[f"{prefix}_{key}"] = v


@cached
def case(name):
    """inputs: buffers no step writes and no update touches; params: weights and batch-norm buffers; outputs: name ->
    (shape, Cin * k * k of the convolution that writes it); launches: fused launches one run of the program is"""
    inputs, params, steps, outputs = {}, {}, [], {}
    if name in ("fold", "plain"):
        inputs["x"] = rnd((2, 64, 6, 5), 11)
        params["w"] = rnd((64, 64, 1, 1), 12, 0.125)
        steps.append(("conv", "x", "y", "w", 1, 1, 0))
        if name == "fold":
            _bn_into(params, "bn", 64, 13)
            steps.append(("bn", "y", "bn"))
        steps.append(("relu", "y"))
        outputs["y"] = ((2, 64, 6, 5), 64)
        launches = 1
    elif name == "panel":
        inputs["x"], inputs["res"] = rnd((2, 64, 6, 5), 21), rnd((2, 96, 6, 5), 22)
        params["w"] = rnd((96, 64, 3, 3), 23, 1.0 / 24)
        _bn_into(params, "bn", 96, 24)
        steps += [("conv", "x", "y", "w", 3, 1, 1), ("bn", "y", "bn"), ("add", "y", "res"), ("relu", "y")]
        outputs["y"] = ((2, 96, 6, 5), 576)
        launches = 1
    elif name == "exact":
        inputs["x"] = rnd((2, 3, 10, 12), 31)
        params["w"] = rnd((8, 3, 3, 3), 32, 1.0 / np.sqrt(27))
        _bn_into(params, "bn", 8, 33)
        steps += [("conv", "x", "y", "w", 3, 1, 1), ("bn", "y", "bn"), ("relu", "y")]
        outputs["y"] = ((2, 8, 10, 12), 27)
        launches = 1
    elif name == "stem":
        inputs["x"] = rnd((2, 3, 32, 32), 41)
        params["w"] = rnd((64, 3, 7, 7), 42, 1.0 / np.sqrt(147))
        _bn_into(params, "bn", 64, 43)
        steps += [("conv", "x", "y", "w", 7, 2, 3), ("bn", "y", "bn"), ("relu", "y"), ("maxpool", "y", "pool", 3, 2, 1)]
        outputs["y"], outputs["pool"] = ((2, 64, 16, 16), 147), ((2, 64, 8, 8), 147)
        launches = 1
    elif name == "chain":
        # both inputs of the block boundary come out of deferred convolutions, so that they are NHWC in their buffers
        # when conv3 + bn + add + relu and conv1 + bn + relu run as one launch (rn_chain.hip)
        inputs["x0"], inputs["x1"] = rnd((2, 64, 6, 5), 51), rnd((2, 64, 6, 5), 52)
        params["wa"], params["wb"] = rnd((64, 64, 1, 1), 53, 0.125), rnd((256, 64, 1, 1), 54, 0.125)
        params["w3"], params["w1"] = rnd((256, 64, 1, 1), 55, 0.125), rnd((64, 256, 1, 1), 56, 1.0 / 16)
        _bn_into(params, "bn3", 256, 57)
        _bn_into(params, "bn1", 64, 58)
        steps += [("conv", "x0", "t2", "wa", 1, 1, 0), ("conv", "x1", "r", "wb", 1, 1, 0),
                  ("conv", "t2", "y", "w3", 1, 1, 0), ("bn", "y", "bn3"), ("add", "y", "r"), ("relu", "y"),
                  ("conv", "y", "t1", "w1", 1, 1, 0), ("bn", "t1", "bn1"), ("relu", "t1")]
        outputs.update(t2=((2, 64, 6, 5), 64), r=((2, 256, 6, 5), 64), y=((2, 256, 6, 5), 64), t1=((2, 64, 6, 5), 256))
        launches = 3
    else:
        raise KeyError(name)
    return {"name": name, "inputs": inputs, "params": params, "steps": steps, "outputs": outputs, "launches": launches}


def run_host(c, params, out=None):
    """the oracle's ops in call order; returns {output name: array}.  `out` renames output buffers (the in-list case
    runs a program twice into different tensors)."""
    out = out or {}
    T = dict(c["inputs"])
    for st in c["steps"]:
        if st[0] == "conv":
            _, a, y, w, k, s, p = st
            T[out.get(y, y)] = O.conv2d(T[out.get(a, a)], params[w], s, p)
        elif st[0] == "bn":
            t = out.get(st[1], st[1])
            T[t] = O.batchnorm2d(T[t], *(params[f"{st[2]}_{key}"] for key in "wbmv"))
        elif st[0] == "add":
            t = out.get(st[1], st[1])
            T[t] = O.add(T[t], T[out.get(st[2], st[2])])
        elif st[0] == "relu":
            t = out.get(st[1], st[1])
            T[t] = O.relu(T[t])
        elif st[0] == "maxpool":
            _, a, y, k, s, p = st
            T[out.get(y, y)] = O.maxpool2d(T[out.get(a, a)], k, s, p)
        else:
            raise KeyError(st[0])
    return {out.get(n, n): T[out.get(n, n)] for n in c["outputs"]}


# =====================================================================================================================
# 2. Parameter updates: p_new = p + d in float32 -- rn_add_forward is one IEEE add, so the device holds the same bits.
#    Every p_new is positive throughout, so that rn_relu_forward(src = p_new, p) writes the same bits as well (the
#    out-of-place writer of the GPU file).
# =====================================================================================================================
# (program, target): each batch-norm buffer alone; a weight as a whole (the packed panel, the exact-K panel, the fused
# stem's panel); the second half of a weight alone
UPDATES = (("fold", "bn_w"), ("fold", "bn_b"), ("fold", "bn_m"), ("fold", "bn_v"),
           ("panel", "w"), ("panel", "w_half"), ("exact", "w"), ("stem", "w"))
TOGGLED = (("panel", "w"), ("fold", "bn_w"))   # the two the GPU file's toggle case (C1) updates literally


@cached
def update(name, target):
    """param: the buffer written; lo, n: the elements [lo, lo + n) the writer covers; d: the n addends; new: the whole
    buffer afterwards"""
    c = case(name)
    param = "w" if target == "w_half" else target
    p = c["params"][param].reshape(-1)
    lo = p.size // 2 if target == "w_half" else 0
    n = p.size - lo
    g = np.random.default_rng(1000 + 7 * NAMES.index(name) + len(target) + sum(map(ord, target)))
    # a weight moves by 1 .. 2 (its values are a few tenths at most), a batch-norm buffer by 0.5 .. 1 (var: positive)
    d = (g.random(n, dtype=F) + F(1.0 if param == "w" else 0.5)).astype(F)
    new = p.copy()
    new[lo:] = (p[lo:] + d).astype(F)
    return {"param": param, "lo": lo, "n": n, "d": d, "new": new.reshape(c["params"][param].shape)}


@cached
def want(name, target=None):
    """the oracle's outputs of the program, with the parameters as generated or after update(name, target)"""
    c = case(name)
    params = dict(c["params"])
    if target is not None:
        u = update(name, target)
        params[u["param"]] = u["new"]
    return run_host(c, params)


# =====================================================================================================================
# 3. The conditions
# =====================================================================================================================
@pytest.mark.parametrize("name", NAMES)
def test_an_output_left_nhwc_is_far_from_the_output(name):
    """destroy, sync, flush and the layout switch are told apart by WHICH of the two images a raw read returns: they
    must be far apart for every output of every program.  (No tensor has one channel or one pixel, where the two
    coincide and the route sets no tag; the stem's pooled tensor has C == H * W and is still not its own image.)"""
    c = case(name)
    for out, (shape, terms) in c["outputs"].items():
        y = want(name)[out]
        assert y.shape == shape and y.dtype == F
        B, C, H, W = shape
        assert C != 1 and H * W != 1 and (C != H * W or (name, out) == ("stem", "pool"))
        gap = float(np.abs(nhwc_image(y) - y).max())
        assert gap >= 100 * bound(y, terms), (name, out, gap, bound(y, terms))
        assert np.abs(y).max() > 0.5 and (y != 0).mean() > 0.3, "a dead tensor would be its own image"


def test_programs_take_the_routes_they_are_named_for():
    """what rn_defer.hip's fusable_conv / run_conv / try_chain decide by, restated on the shapes"""
    for name in NAMES:
        for st in case(name)["steps"]:
            if st[0] != "conv":
                continue
            Cout, Cin, k, _ = case(name)["params"][st[3]].shape
            assert Cout % 4 == 0
            assert (Cin % 32 == 0) != (name in ("exact", "stem")), "whole 128-byte channel segments, or the exact-K form"
            if Cin % 32:
                assert Cin <= 4 and k <= 8
    assert not any(st[0] == "bn" for st in case("plain")["steps"]), "nothing folded: bit for bit the literal route's"
    x, w = case("stem")["inputs"]["x"], case("stem")["params"]["w"]
    assert w.shape == (64, 3, 7, 7) and x.shape[3] % 4 == 0 and case("stem")["outputs"]["y"][0][3] % 8 == 0
    ch = case("chain")
    assert ch["params"]["w3"].shape == (256, 64, 1, 1) and ch["params"]["w1"].shape == (64, 256, 1, 1)
    assert [s[2] for s in ch["steps"] if s[0] == "conv"][:2] == ["t2", "r"], "conv3's input and residual: deferred outputs"


@pytest.mark.parametrize("name,target", UPDATES)
def test_an_update_moves_the_output_far(name, target):
    """with the old fold or panel the route gives want(name); with the new one want(name, target): 100 bounds apart, so
    a stale cache is the only way to the old answer"""
    c, u = case(name), update(name, target)
    p = c["params"][u["param"]]
    assert u["new"].dtype == F and u["new"].shape == p.shape and u["d"].shape == (u["n"],)
    flat_old, flat_new = p.reshape(-1), u["new"].reshape(-1)
    assert same_bits(flat_new[:u["lo"]], flat_old[:u["lo"]]), "nothing in front of the written range moves"
    assert same_bits(flat_new[u["lo"]:], flat_old[u["lo"]:] + u["d"])
    assert (u["d"] > 0).all() and (flat_new[u["lo"]:] > 0).all(), "a ReLU of the new values is the identity"
    assert (u["lo"] * 4) % 16 == 0, "the writer's pointer keeps the entry points' alignment"
    if target == "w_half":
        assert 0 < u["lo"] == p.size - u["n"], "the write starts INSIDE the weight buffer"
    for out, (_, terms) in c["outputs"].items():
        old, new = want(name)[out], want(name, target)[out]
        gap = float(np.abs(new - old).max())
        assert gap >= 100 * max(bound(old, terms), bound(new, terms)), (name, target, out, gap)


@pytest.mark.parametrize("name,target", UPDATES)
def test_in_list_case_has_an_old_and_a_new_answer(name, target):
    """program into out1, the update, program into out2, as ONE list: out1 is the old-parameter reference, out2 the
    new-parameter one, and they differ -- a cache dropped at the start of the flush, or never, fails one of them"""
    c, u = case(name), update(name, target)
    first = {n: n + "1" for n in c["outputs"]}
    second = {n: n + "2" for n in c["outputs"]}
    params = dict(c["params"])
    got1 = run_host(c, params, first)
    flat = params[u["param"]].reshape(-1).copy()
    flat[u["lo"]:] = O.add(flat[u["lo"]:], u["d"])           # the recorded rn_add_forward(p, d, p, n)
    params[u["param"]] = flat.reshape(params[u["param"]].shape)
    got2 = run_host(c, params, second)
    for n in c["outputs"]:
        assert same_bits(got1[n + "1"], want(name)[n])
        assert same_bits(got2[n + "2"], want(name, target)[n])
        assert not np.array_equal(got1[n + "1"], got2[n + "2"])


def test_toggle_updates_are_among_the_updates():
    assert set(TOGGLED) <= set(UPDATES)
