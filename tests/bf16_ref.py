"""A per-element reference for results that were rounded to bf16 (test infrastructure; used by
test_bf16_ref_host.py, test_bf16_rounding_gpu.py and test_bf16_gpu.py).

A bf16 kernel computes an fp32 value -- products of bf16 operands, exact in fp32, added in some order, then
scale, shift, residual and ReLU -- and stores it rounded to the nearest bf16.  `conv64` and `epilogue64`
evaluate the same expression in float64 on the operands as the kernel sees them (bf16-rounded activations,
weights and residual, fp32 scale and shift); `assert_bf16_rounded` then holds EVERY element of the kernel's
output to

    |got - ref64| <= half_step(ref64) + eps_sum

    half_step(v) = 2 ** (floor(log2 |v|) - 8)      half the spacing of bf16 in v's binade, 0 for v == 0
    eps_sum      = 3e-7 * sqrt(k_terms) * max|ref64| + 1e-6

eps_sum is what test_ops_gpu.py::assert_close allows the fp32 accumulation of k_terms products (any order);
half_step is the error of ONE round-to-nearest of that fp32 value.  A bound on the tensor's maximum
(2**-8 * max|ref|) is half a step of the LARGEST element and lets a typical element, binades smaller, be
several of its own steps off; this one does not: truncation, a second rounding before the residual add or a
residual taken at another precision all leave it (test_bf16_ref_host.py shows that on emulations)."""
import numpy as np

from resnet_c_amd.ops import bf16_round  # noqa: F401  (re-exported: the operands of every reference here)


def conv64(x, w, stride=1, pad=0, groups=1):
    """float64 convolution of NCHW x [B,Cin,H,W] with OIHW w [Cout,Cin/groups,k,k]: im2col + matmul per group."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, Cin, H, W = x.shape
    Cout, cg, k, k2 = w.shape
    assert k == k2 and Cin == cg * groups and Cout % groups == 0
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.zeros((B, Cin, H + 2 * pad, W + 2 * pad), dtype=np.float64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    # cols[b, c, kh, kw, oh, ow] = xp[b, c, oh * stride + kh, ow * stride + kw]
    cols = np.empty((B, Cin, k, k, ho, wo), dtype=np.float64)
    for kh in range(k):
        for kw in range(k):
            cols[:, :, kh, kw] = xp[:, :, kh:kh + (ho - 1) * stride + 1:stride, kw:kw + (wo - 1) * stride + 1:stride]
    out = np.empty((B, Cout, ho, wo), dtype=np.float64)
    og = Cout // groups
    for g in range(groups):
        a = cols[:, g * cg:(g + 1) * cg].transpose(0, 4, 5, 1, 2, 3).reshape(B * ho * wo, cg * k * k)
        y = a @ w[g * og:(g + 1) * og].reshape(og, cg * k * k).T
        out[:, g * og:(g + 1) * og] = y.reshape(B, ho, wo, og).transpose(0, 3, 1, 2)
    return out


def epilogue64(y64, scale=None, shift=None, residual=None, relu=False):
    """scale, shift, residual, ReLU in float64 on an NCHW float64 tensor; `residual` as the kernel reads it."""
    y = np.asarray(y64, dtype=np.float64)
    if scale is not None:
        y = y * np.asarray(scale, dtype=np.float64)[None, :, None, None]
    if shift is not None:
        y = y + np.asarray(shift, dtype=np.float64)[None, :, None, None]
    if residual is not None:
        y = y + np.asarray(residual, dtype=np.float64)
    return np.maximum(y, 0.0) if relu else y


def maxpool64(y, k, stride, pad):
    """max-pool of an NCHW float64 tensor, padding = -inf (every window of the callers holds a real pixel)"""
    B, C, H, W = y.shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    yp = np.full((B, C, H + 2 * pad, W + 2 * pad), -np.inf, dtype=np.float64)
    yp[:, :, pad:pad + H, pad:pad + W] = y
    out = np.full((B, C, ho, wo), -np.inf, dtype=np.float64)
    for kh in range(k):
        for kw in range(k):
            out = np.maximum(out, yp[:, :, kh:kh + (ho - 1) * stride + 1:stride, kw:kw + (wo - 1) * stride + 1:stride])
    return out


def half_step(v):
    """half the spacing of bf16 (8 significant bits) in the binade of each v; 0 where v == 0"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    out = np.zeros_like(a)
    nz = a > 0
    out[nz] = np.exp2(np.floor(np.log2(a[nz])) - 8)
    return out


def eps_sum(ref64, k_terms):
    return 3e-7 * np.sqrt(k_terms) * float(np.abs(ref64).max()) + 1e-6


def measure(got, ref64, k_terms):
    """The figures of one comparison, for the record: the largest error in units of the element's own bf16
    step, taken over the elements whose half step is at least eps_sum (below that the accumulation error, not
    the rounding, sets the bound, and a step count says nothing); the largest share of its bound any element
    used; and eps_sum's share of the bound at the median element with a non-zero reference (ReLU zeros have
    no rounding error to bound: eps_sum is their whole bound)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    hs, eps = half_step(ref64), eps_sum(ref64, k_terms)
    err = np.abs(got - ref64)
    big = hs >= eps
    steps = float((err[big] / (2 * hs[big])).max()) if big.any() else 0.0
    nz = hs > 0
    share = float(np.median(eps / (hs[nz] + eps))) if nz.any() else 1.0
    return {"max_err_steps": steps, "max_bound_used": float((err / (hs + eps)).max()),
            "eps_share_median": share, "eps_sum": eps, "elements": int(got.size)}


def assert_bf16_rounded(got, ref64, k_terms, what=""):
    """Every element of `got` (the kernel's bf16 output widened to fp32) within half a bf16 step of its own
    float64 reference, plus the fp32 accumulation error of k_terms products.  Returns `measure`'s figures."""
    got = np.asarray(got)
    ref64 = np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, f"{what}: shape {got.shape} against {ref64.shape}"
    assert np.isfinite(ref64).all(), f"{what}: the reference is not finite"
    g64 = got.astype(np.float64)
    hs, eps = half_step(ref64), eps_sum(ref64, k_terms)
    err = np.abs(g64 - ref64)
    bad = ~(err <= hs + eps)      # a NaN in got is bad
    if bad.any():
        excess = np.where(np.isnan(err), np.inf, err - (hs + eps))
        idx = np.unravel_index(int(np.argmax(excess)), ref64.shape)
        step = 2 * hs[idx]
        units = f"{err[idx] / step:.3f} steps of {step:.3e}" if step > 0 else "reference 0: no step"
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} elements outside half a bf16 step + eps_sum ({eps:.3e}); "
            f"worst at {tuple(int(i) for i in idx)}: got {float(g64[idx])!r}, ref {float(ref64[idx])!r}, "
            f"error {err[idx]:.3e} = {units}")
    return measure(got, ref64, k_terms)
