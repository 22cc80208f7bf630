"""What a deferred context (rn_ctx_set_deferred, rn_defer.hip) leaves behind: the caller buffers it holds as NHWC when
it is destroyed, the folds and packed panels it made from parameters that a recorded op -- or a literal one, while the
route is switched off -- writes afterwards, and what a sync does and does not do to the buffers.

Every program, input and update comes from test_defer_state_host.py, which vets them on the oracle alone.  Tensors are
allocated on the shared context R.get_ctx(), which is never deferred here: a read through it (FloatTensor.numpy) copies
the bytes as they lie -- the RAW read.  The context under test is the test's own R.Context(), closed in try / finally.
Every tensor a deferred context has named stays referenced until that context is closed: destroy rewrites the buffers
it holds as NHWC, and a buffer freed behind its back would be written after its free.  Values are held to the oracle
within the bound of test_fused_chain_against_the_oracle, and bit for bit to the literal route where no batch-norm is
folded.  profiles/defer_state/README.md lists which case is there for which path."""
import ctypes
import functools

import numpy as np
import pytest

import resnet_c_amd as R
import test_defer_state_host as H
from resnet_c_amd import _lib as L

pytestmark = pytest.mark.gpu

KEYS = "wbmv"


def call(ctx, name, *args):
    L.check(getattr(L.lib(), name)(ctx.handle, *args), name, ctx.handle)


def gpu(a):
    return R.FloatTensor.from_numpy(np.ascontiguousarray(a, dtype=np.float32), R.Device.GPU)


def upload(c):
    """the program's inputs and parameters on the device (through the shared context, synchronously)"""
    return {k: gpu(v) for k, v in {**c["inputs"], **c["params"]}.items()}


def outputs(c):
    return {n: R.FloatTensor(shape, R.Device.GPU) for n, (shape, _) in c["outputs"].items()}


def record(ctx, c, D, T):
    """the program's calls on ctx: D the inputs and parameters, T the output tensors"""
    def buf(n):
        return (T[n] if n in T else D[n]).data()

    for st in c["steps"]:
        if st[0] == "conv":
            _, a, y, w, k, s, p = st
            Cout, Cin = c["params"][w].shape[:2]
            src = c["inputs"][a].shape if a in c["inputs"] else c["outputs"][a][0]
            B, _, ho, wo = c["outputs"][y][0]
            call(ctx, "rn_conv2d_forward", buf(a), buf(y), buf(w), k, s, p, ho, wo, B, Cin, Cout, src[2], src[3])
        elif st[0] == "bn":
            B, C, ho, wo = c["outputs"][st[1]][0]
            call(ctx, "rn_batchnorm2d_forward", buf(st[1]), buf(st[1]), *(buf(f"{st[2]}_{k}") for k in KEYS), B, C, ho * wo)
        elif st[0] == "add":
            call(ctx, "rn_add_forward", buf(st[1]), buf(st[2]), buf(st[1]), int(np.prod(c["outputs"][st[1]][0])))
        elif st[0] == "relu":
            call(ctx, "rn_relu_forward", buf(st[1]), buf(st[1]), int(np.prod(c["outputs"][st[1]][0])))
        elif st[0] == "maxpool":
            _, a, y, k, s, p = st
            B, C, Hi, Wi = c["outputs"][a][0]
            _, _, ho, wo = c["outputs"][y][0]
            call(ctx, "rn_maxpool2d_forward", buf(a), buf(y), k, s, p, ho, wo, B, C, Hi, Wi)
        else:
            raise KeyError(st[0])


def read_through(ctx, t):
    """rn_memcpy_d2h of the whole tensor through ctx: NCHW whatever the buffer holds (a tagged buffer stays NHWC)"""
    host = np.empty(tuple(t.shape()), dtype=np.float32)
    call(ctx, "rn_memcpy_d2h", host.ctypes.data, t.data(), host.nbytes)
    return host


def raw(t):
    return t.numpy()


def within_bound(got, want, terms):
    err = float(np.abs(got - want).max())
    assert err <= H.bound(want, terms), (err, H.bound(want, terms))


def fused(ctx):
    return ctx.deferred_stats()["fused_launches"]


@functools.lru_cache(maxsize=None)
def literal(name):
    """the program's calls one launch each on the shared context, into buffers of its own: the parity baseline"""
    c = H.case(name)
    D, T = upload(c), outputs(c)
    assert not R.get_ctx().deferred_stats()["nhwc_buffers"]
    record(R.get_ctx(), c, D, T)
    return {n: t.numpy() for n, t in T.items()}


# =====================================================================================================================
# A. rn_ctx_destroy gives every buffer its NCHW content back
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def flushed(name):
    """record, rn_sync, look, close, look again; shared by the two states (the arrays are never written to)"""
    c = H.case(name)
    D, T = upload(c), outputs(c)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        s0 = ctx.deferred_stats()
        record(ctx, c, D, T)
        ctx.sync()
        s1 = ctx.deferred_stats()
        whole = {n: read_through(ctx, t) for n, t in T.items()}
        before = {n: raw(t) for n, t in T.items()}
    finally:
        ctx.close()
    after = {n: raw(t) for n, t in T.items()}
    return {"s0": s0, "s1": s1, "whole": whole, "before": before, "after": after}


@pytest.mark.parametrize("name", H.NAMES)
def test_destroy_after_a_sync_gives_every_buffer_its_nchw_content(name):
    c, r = H.case(name), flushed(name)
    # not vacuous: the program ran fused, and until the context went the buffers held NHWC
    assert r["s1"]["fused_launches"] - r["s0"]["fused_launches"] == c["launches"] and r["s1"]["pending_ops"] == 0
    assert r["s1"]["nhwc_buffers"] >= 1
    for n, (_, terms) in c["outputs"].items():
        assert H.same_bits(r["before"][n], H.nhwc_image(r["whole"][n])), n
        assert not np.array_equal(r["before"][n], r["whole"][n]), n
    for n, (_, terms) in c["outputs"].items():
        assert H.same_bits(r["after"][n], r["whole"][n]), n
        within_bound(r["after"][n], H.want(name)[n], terms)
        if name == "plain":
            assert H.same_bits(r["after"][n], literal(name)[n])


@pytest.mark.parametrize("name", H.NAMES)
def test_destroy_with_ops_pending_runs_them_and_leaves_nchw(name):
    c = H.case(name)
    D, T = upload(c), outputs(c)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        record(ctx, c, D, T)
        assert ctx.deferred_stats()["pending_ops"] == len(c["steps"])
    finally:
        ctx.close()
    for n, (_, terms) in c["outputs"].items():
        assert H.same_bits(raw(T[n]), flushed(name)["whole"][n]), n
        within_bound(raw(T[n]), H.want(name)[n], terms)


class _Pointer:
    """a device address where record() expects a tensor"""

    def __init__(self, ptr):
        self.ptr = ptr

    def data(self):
        return self.ptr


def test_destroy_has_nothing_to_rewrite_after_a_free():
    """the output allocated and freed through the deferred context: the free runs the list and takes the tag"""
    c = H.case("fold")
    D = upload(c)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        p = ctypes.c_void_p()
        call(ctx, "rn_malloc", ctypes.byref(p), int(np.prod(c["outputs"]["y"][0])) * 4)
        f0 = fused(ctx)
        record(ctx, c, D, {"y": _Pointer(p.value)})
        assert ctx.deferred_stats()["pending_ops"] == len(c["steps"])
        call(ctx, "rn_free", p)
        s = ctx.deferred_stats()
        assert s["pending_ops"] == 0 and fused(ctx) - f0 == 1 and s["nhwc_buffers"] == 0
    finally:
        ctx.close()


# =====================================================================================================================
# B. folds and panels follow writes made by recorded ops
# =====================================================================================================================
def writer_operands(D, u):
    """(the written range's device address, the addends on the device, the new values on the device)"""
    dst = D[u["param"]].data() + 4 * u["lo"]
    return dst, gpu(u["d"]), gpu(u["new"].reshape(-1)[u["lo"]:])


def check_old_and_new(name, target, old, new):
    c = H.case(name)
    for n, (_, terms) in c["outputs"].items():
        if old is not None:
            within_bound(old[n], H.want(name)[n], terms)
        within_bound(new[n], H.want(name, target)[n], terms)


@pytest.mark.parametrize("writer", ["add", "relu"])
@pytest.mark.parametrize("name,target", H.UPDATES)
def test_caches_follow_a_recorded_write_between_two_lists(name, target, writer):
    """program, read, a recorded op that writes the parameter -- rn_add_forward in place, or the out-of-place
    rn_relu_forward(src, p) with src = the new values, all positive --, program, read: the second result is the new
    parameter's.  Both programs ran fused."""
    c, u = H.case(name), H.update(name, target)
    D, T = upload(c), outputs(c)
    dst, d, src = writer_operands(D, u)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        f0 = fused(ctx)
        record(ctx, c, D, T)
        old = {n: read_through(ctx, t) for n, t in T.items()}
        if writer == "add":
            call(ctx, "rn_add_forward", dst, d.data(), dst, u["n"])
        else:
            call(ctx, "rn_relu_forward", src.data(), dst, u["n"])
        record(ctx, c, D, T)
        new = {n: read_through(ctx, t) for n, t in T.items()}
        assert fused(ctx) - f0 == 2 * c["launches"]
        assert H.same_bits(read_through(ctx, D[u["param"]]).reshape(-1), u["new"].reshape(-1)), "the write itself"
    finally:
        ctx.close()
    check_old_and_new(name, target, old, new)


@pytest.mark.parametrize("name,target", H.UPDATES)
def test_caches_follow_a_recorded_write_inside_one_list(name, target):
    """program into out1, rn_add_forward into the parameter, program into out2, nothing observed until out2 is read:
    out1 was computed from the old fold / panel, out2 from a new one"""
    c, u = H.case(name), H.update(name, target)
    D, T1, T2 = upload(c), outputs(c), outputs(c)
    dst, d, _ = writer_operands(D, u)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        f0 = fused(ctx)
        record(ctx, c, D, T1)
        call(ctx, "rn_add_forward", dst, d.data(), dst, u["n"])
        record(ctx, c, D, T2)
        assert ctx.deferred_stats()["pending_ops"] == 2 * len(c["steps"]) + 1 and fused(ctx) == f0
        new = {n: read_through(ctx, t) for n, t in T2.items()}
        old = {n: read_through(ctx, t) for n, t in T1.items()}
        assert fused(ctx) - f0 == 2 * c["launches"]
    finally:
        ctx.close()
    check_old_and_new(name, target, old, new)


# =====================================================================================================================
# C. toggles
# =====================================================================================================================
@pytest.mark.parametrize("name,target", H.TOGGLED)
def test_caches_do_not_survive_a_literal_write_while_deferred_is_off(name, target):
    """C1: deferred run, deferred off, a literal rn_add_forward into the parameter, deferred on, deferred run"""
    c, u = H.case(name), H.update(name, target)
    D, T = upload(c), outputs(c)
    dst, d, _ = writer_operands(D, u)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        f0 = fused(ctx)
        record(ctx, c, D, T)
        old = {n: read_through(ctx, t) for n, t in T.items()}
        ctx.set_deferred(False)
        launches = L.lib().rn_ctx_launch_count(ctx.handle)
        call(ctx, "rn_add_forward", dst, d.data(), dst, u["n"])
        assert L.lib().rn_ctx_launch_count(ctx.handle) == launches + 1, "literal: launched at once"
        ctx.set_deferred(True)
        record(ctx, c, D, T)
        new = {n: read_through(ctx, t) for n, t in T.items()}
        assert fused(ctx) - f0 == 2 * c["launches"]
    finally:
        ctx.close()
    check_old_and_new(name, target, old, new)


def test_layout_switch_gives_tagged_buffers_back_and_the_route_goes_on():
    """C2: two buffers tagged (the stem launch writes both), rn_ctx_set_layout(NHWC): both NCHW again, no tag left;
    layout back, the program again: the same bits as before"""
    c = H.case("stem")
    D, T = upload(c), outputs(c)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        record(ctx, c, D, T)
        first = {n: read_through(ctx, t) for n, t in T.items()}
        assert ctx.deferred_stats()["nhwc_buffers"] == 2
        for n in T:
            assert H.same_bits(raw(T[n]), H.nhwc_image(first[n]))
        ctx.set_layout(L.RN_LAYOUT_NHWC)
        assert ctx.deferred_stats()["nhwc_buffers"] == 0
        ctx.sync()
        for n in T:
            assert H.same_bits(raw(T[n]), first[n]), n
        ctx.set_layout(L.RN_LAYOUT_NCHW)
        f0 = fused(ctx)
        record(ctx, c, D, T)
        again = {n: read_through(ctx, t) for n, t in T.items()}
        assert fused(ctx) - f0 == 1 and ctx.deferred_stats()["nhwc_buffers"] == 2
    finally:
        ctx.close()
    for n, (_, terms) in c["outputs"].items():
        assert H.same_bits(again[n], first[n])
        within_bound(again[n], H.want("stem")[n], terms)


# =====================================================================================================================
# D. what rn_hip.h says a sync does not do
# =====================================================================================================================
def _sync(ctx, ptr):
    ctx.sync()


def _flush_sync(ctx, ptr):
    ctx.flush()
    ctx.sync()


def _event_sync(ctx, ptr):
    ev = ctypes.c_void_p()
    call(ctx, "rn_event_create", ctypes.byref(ev))
    try:
        call(ctx, "rn_event_record", ev)
        ctx.sync()
    finally:
        L.lib().rn_event_destroy(ev)


def _observe_sync(ctx, ptr):
    ctx.observe(ptr)
    ctx.sync()


@pytest.mark.parametrize("name", ["plain", "fold"])
@pytest.mark.parametrize("how,nchw", [(_sync, False), (_flush_sync, False), (_event_sync, False), (_observe_sync, True)],
                         ids=["sync", "flush_sync", "event_sync", "observe_sync"])
def test_a_sync_runs_the_list_and_leaves_the_buffer_nhwc_until_it_is_observed(how, nchw, name):
    """rn_sync, rn_flush and rn_event_record run what is recorded; the buffer stays NHWC and tagged, and another
    stream or context that reads it sees the NHWC image.  rn_observe(ctx, ptr) first: NCHW."""
    c = H.case(name)
    D, T = upload(c), outputs(c)
    ctx = R.Context()
    try:
        ctx.set_deferred(True)
        f0 = fused(ctx)
        record(ctx, c, D, T)
        how(ctx, T["y"].data())
        s = ctx.deferred_stats()
        assert s["pending_ops"] == 0 and fused(ctx) - f0 == 1
        seen = raw(T["y"])
        assert s["nhwc_buffers"] == (0 if nchw else 1)
        whole = read_through(ctx, T["y"])
    finally:
        ctx.close()
    assert H.same_bits(seen, whole if nchw else H.nhwc_image(whole))
    within_bound(whole, H.want(name)["y"], c["outputs"]["y"][1])
    if name == "plain":
        assert H.same_bits(whole, literal(name)["y"])
