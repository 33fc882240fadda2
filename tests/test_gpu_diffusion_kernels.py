"""Kernel-level parity of csrc/diffusion.hip at its edges: groupnorm (the one-workgroup kernel and the chunked large-map path,
every activation and epilogue, the switch between the paths, the fall-backs of the dispatch guard, the 256-chunk cap),
mish, spatial_softmax, unfold1d, ddim_step and u8_to_nhwc4, each against a plain float64 reference on the CPU
(tests/helpers.py; test_kernel_refs_cpu.py proves those references against torch's own operators and proves that the hard
cases bite).  Copies are held to bit equality.  Every test prints its measured error next to its bound.

Bounds: the project's (2e-6 of the output's maximum on the one-workgroup GroupNorm, 3e-6 on the chunked path, 1e-6 absolute on
keypoint coordinates, 2e-6 of the maximum for fp32 elementwise work); for Mish 4 x the worst elementwise relative error of
torch's own float32 CPU F.mish on the same inputs, measured in the test.

Left uncovered on purpose: the `2048 / (n G) + 1` chunk cap of actmi_op_groupnorm.  It binds only when n * G is several hundred
with >= 65 536 values per group -- tens of millions of floats, not a unit test's size."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import helpers as Hh  # noqa: E402
from helpers import rel_err  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402

D = "cuda:0"
ACT_NAMES = [None, "relu", "mish"]


def _gn_data(n, P, C, seed, ramp=False):
    g = torch.Generator().manual_seed(seed)
    x = Hh.gn_ramp(n, P, C, g) if ramp else torch.randn(n, P, C, generator=g) * 3 + 1
    res = torch.randn(n, P, C, generator=g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    film = (torch.randn(n, C, generator=g), torch.randn(n, C, generator=g))
    return x, res, w, b, film


def _dev(kw):
    return {k: (tuple(t.to(D) for t in v) if isinstance(v, tuple) else v.to(D) if isinstance(v, torch.Tensor) else v)
            for k, v in kw.items()}


def _gn_raw(x, w, b, out, n, P, Cc, G, act=0, res=None, rm=0, fs=None, fb=None, ws=None, ws_floats=0):
    """actmi_op_groupnorm through the C entry (the wrapper always hands over a large workspace)"""
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
    L.check(L.load().actmi_op_groupnorm(p(x), p(res), p(fs), p(fb), p(w), p(b), p(out), n, P, Cc, G, 1e-5, act, rm, p(ws), ws_floats,
                                        L.current_stream_ptr()), None, "op_groupnorm")
    return out


# ---- A.1 the one-workgroup kernel ------------------------------------------------------------------------------------------
GN_SCALAR = [(1, 1, 8, 8), (2, 4, 256, 8), (2, 8, 512, 8), (3, 16, 1024, 8), (2, 5, 6, 3), (1, 300, 12, 4), (5, 77, 64, 1)]


@pytest.mark.parametrize("act", ACT_NAMES)
@pytest.mark.parametrize("n,P,C,G", GN_SCALAR)
def test_groupnorm_scalar_kernel(n, P, C, G, act):
    """the UNet's own (8 groups of 32 / 64 / 128 channels over 4 / 8 / 16 positions), a group width of 2, one group, and one
    value per group (variance 0: rstd = 1 / sqrt(eps), the normalised value is the bias -- judged absolutely against
    2e-6 max|bias|)"""
    assert P * (C // G) < 16384
    x, res, w, b, film = _gn_data(n, P, C, seed=P * 31 + C)
    for ep in Hh.GN_EPILOGUES:
        kw = Hh.gn_epilogue_args(ep, res, film)
        exp = Hh.groupnorm_ref(x, w, b, G, act=act, **kw)
        got = ops.groupnorm(x.to(D), w.to(D), b.to(D), G, act=act, **_dev(kw))
        if P == 1 and C == G:
            err, bound = float((got.cpu().double() - exp).abs().max()), 2e-6 * float(b.abs().max())
            what = "absolute"
        else:
            err, bound, what = rel_err(got, exp), 2e-6, "of max"
        print(f"A.1 groupnorm n={n} P={P} C={C} G={G} act={act} {ep}: {err:.2e} {what} (bound {bound:.2e})")
        assert err < bound


# ---- A.2 every branch of the chunked path -----------------------------------------------------------------------------------
GN_CHUNKED = [(2, 33 * 47, 128, 8), (1, 12289, 8, 2)]


@pytest.mark.parametrize("act", ACT_NAMES)
@pytest.mark.parametrize("n,P,C,G", GN_CHUNKED)
def test_groupnorm_chunked_path_every_branch(n, P, C, G, act):
    assert P * (C // G) >= 16384 and Hh.gn_chunks(n, G, P * (C // G)) == (1 if C == 128 else 3)
    x, res, w, b, film = _gn_data(n, P, C, seed=P + C)
    xd, wd, bd = x.to(D), w.to(D), b.to(D)
    for ep in Hh.GN_EPILOGUES:
        kw = Hh.gn_epilogue_args(ep, res, film)
        kd = _dev(kw)
        exp = Hh.groupnorm_ref(x, w, b, G, act=act, **kw)
        got = ops.groupnorm(xd, wd, bd, G, act=act, **kd)
        err = rel_err(got, exp)
        buf = torch.full((2, n, P, C), 123.0, device=D)
        into = ops.groupnorm(xd, wd, bd, G, act=act, out=buf[1], **kd)
        again = ops.groupnorm(xd, wd, bd, G, act=act, **kd)
        print(f"A.2 groupnorm chunked n={n} P={P} C={C} G={G} act={act} {ep}: {err:.2e} of max (bound 3.0e-06)")
        assert err < 3e-6
        assert into.data_ptr() == buf[1].data_ptr() and torch.equal(into, got) and bool((buf[0] == 123.0).all())
        assert torch.equal(again, got)


# ---- A.3 / A.6 chunk means that differ, and the 256-chunk cap ---------------------------------------------------------------
@pytest.mark.parametrize("n,P,C,G,nch", [(1, 12289, 8, 2, 3), (1, 1050001, 4, 1, 256)])
def test_groupnorm_chunked_ramp(n, P, C, G, nch):
    """x = randn + 40 p / P: the between-chunk term of Chan's update is the larger part of the variance (test_kernel_refs_cpu.py:
    without it the error is > 100 x this bound).  P = 1 050 001, C = 4, G = 1: per / 16384 = 256.3, capped to 256 chunks."""
    assert Hh.gn_chunks(n, G, P * (C // G)) == nch
    x, res, w, b, film = _gn_data(n, P, C, seed=P, ramp=True)
    exp = Hh.groupnorm_ref(x, w, b, G)
    err = rel_err(ops.groupnorm(x.to(D), w.to(D), b.to(D), G), exp)
    print(f"A.3/6 groupnorm ramp n={n} P={P} C={C} G={G} ({nch} chunks): {err:.2e} of max (bound 3.0e-06)")
    assert err < 3e-6


# ---- A.4 the switch between the two paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1023, 1024])
def test_groupnorm_path_boundary(P):
    """C = 64, G = 4: P = 1024 is the first chunked shape (per = 16384), P = 1023 the last one-workgroup shape"""
    n, Cc, G = 2, 64, 4
    x, res, w, b, film = _gn_data(n, P, Cc, seed=P)
    kw = Hh.gn_epilogue_args("film+res_after", res, film)
    exp = Hh.groupnorm_ref(x, w, b, G, act="mish", **kw)
    err = rel_err(ops.groupnorm(x.to(D), w.to(D), b.to(D), G, act="mish", **_dev(kw)), exp)
    bound = 3e-6 if P * (Cc // G) >= 16384 else 2e-6
    print(f"A.4 groupnorm boundary P={P} (per = {P * (Cc // G)}): {err:.2e} of max (bound {bound:.1e})")
    assert err < bound


# ---- A.5 the fall-backs of the dispatch guard ------------------------------------------------------------------------------
def _off4(t):
    """a contiguous copy of t on the device that starts 4 bytes into a larger buffer"""
    buf = torch.empty(t.numel() + 1, device=D)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("act", [None, "mish"])
def test_groupnorm_fallbacks_of_a_large_map(act):
    """a large map (33 x 47, C = 128, G = 8) that the guard of actmi_op_groupnorm keeps off the 16-byte path: x or res not
    16-byte aligned, no workspace, a workspace too small.  All of them take the one-workgroup kernel, so they agree bit for bit
    with each other, meet 3e-6 against float64 and lie within 3e-6 of the chunked result."""
    n, P, Cc, G = 2, 33 * 47, 128, 8
    x, res, w, b, film = _gn_data(n, P, Cc, seed=77)
    exp = Hh.groupnorm_ref(x, w, b, G, act=act, res=res)
    xd, rd, wd, bd = x.to(D), res.to(D), w.to(D), b.to(D)
    chunked = ops.groupnorm(xd, wd, bd, G, act=act, res=rd)
    a, rm = ops.ACT[act], 1
    no_ws = _gn_raw(xd, wd, bd, torch.empty_like(xd), n, P, Cc, G, a, rd, rm)
    ws2 = torch.zeros(2, device=D)
    small_ws = _gn_raw(xd, wd, bd, torch.empty_like(xd), n, P, Cc, G, a, rd, rm, ws=ws2, ws_floats=2)
    x_off = ops.groupnorm(_off4(x), wd, bd, G, act=act, res=rd)
    r_off = ops.groupnorm(xd, wd, bd, G, act=act, res=_off4(res))
    for name, got in (("chunked", chunked), ("ws = NULL", no_ws), ("ws_floats = 2", small_ws), ("x + 4 bytes", x_off),
                      ("res + 4 bytes", r_off)):
        e64, ech = rel_err(got, exp), rel_err(got, chunked)
        print(f"A.5 groupnorm act={act} {name}: {e64:.2e} of max against float64, {ech:.2e} against the chunked result (bound 3.0e-06)")
        assert e64 < 3e-6 and ech < 3e-6
    assert bool((ws2 == 0).all())                                               # a workspace too small is not written
    for got in (small_ws, x_off, r_off):
        assert torch.equal(got, no_ws)


# ---- A.8 rejections ----------------------------------------------------------------------------------------------------------
def test_groupnorm_rejections():
    x, w, b = torch.zeros(1, 4, 6, device=D), torch.ones(6, device=D), torch.zeros(6, device=D)
    with pytest.raises(RuntimeError):
        ops.groupnorm(x, w, b, 4)                                               # C % G
    out, fs = torch.empty_like(x), torch.ones(1, 6, device=D)
    _gn_raw(x, w, b, out, 1, 4, 6, 3)                                           # the same call, accepted
    with pytest.raises(RuntimeError):
        _gn_raw(x, w, b, out, 1, 4, 6, 3, fs=fs)                                # FiLM scale without bias
    with pytest.raises(RuntimeError):
        _gn_raw(x, w, b, out, 1, 4, 6, 3, fb=fs)
    for rm in (1, 2):
        with pytest.raises(RuntimeError):
            _gn_raw(x, w, b, out, 1, 4, 6, 3, rm=rm)                            # res_mode with a null res
    torch.cuda.synchronize()


# ---- B. mish -----------------------------------------------------------------------------------------------------------------
def _mish_bound(x):
    exp = F.mish(x.double())
    cpu32 = Hh.elem_rel_err(F.mish(x), exp)
    return exp, cpu32, 4 * cpu32


def test_mish_elementwise_relative():
    """elementwise relative error against float64 F.mish on the non-zero expectations; the bound is 4 x the same figure of torch's
    float32 CPU F.mish (about 2e-7, so about 8e-7): a softplus written log(1 + exp(x)) returns 0 below -17, relative error 1"""
    x = Hh.mish_inputs()
    exp, cpu32, bound = _mish_bound(x)
    got = ops.mish(x.to(D)).cpu()
    err = Hh.elem_rel_err(got, exp)
    print(f"B. mish on {x.numel()} values: worst elementwise relative error {err:.2e} (float32 CPU F.mish {cpu32:.2e}, bound {bound:.2e})")
    assert err < bound
    assert bool((got[exp == 0] == 0).all()) and int((exp == 0).sum()) == 2      # +-0 -> 0
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_mish_lengths(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 5
    exp, cpu32, bound = _mish_bound(x)
    got = ops.mish(x.to(D))
    err = Hh.elem_rel_err(got, exp)
    print(f"B. mish n={n}: {err:.2e} elementwise relative (bound {bound:.2e})")
    assert got.numel() == n and err < bound
    z = ops.mish(torch.zeros(n, device=D))
    assert bool((z == 0).all())


# ---- C. spatial_softmax ------------------------------------------------------------------------------------------------------
SS_SHAPES = [(1, 1, 1, 1), (2, 1, 9, 3), (2, 7, 1, 5), (3, 3, 4, 2), (1, 8, 8, 32), (2, 9, 13, 33)]


@pytest.mark.parametrize("temp", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("n,H,W,K", SS_SHAPES)
def test_spatial_softmax_shapes_and_temperature(n, H, W, K, temp):
    """fewer than 64 positions (idle lanes carry -inf into the max), H = 1 and W = 1 (their own grid branches), 64 positions, more"""
    g = torch.Generator().manual_seed(H * 100 + W)
    lg = torch.randn(n, H * W, K, generator=g) * 4
    exp = Hh.spatial_softmax_ref(lg, H, W, temp)
    got = ops.spatial_softmax(lg.to(D), H, W, temperature=temp)
    err = float((got.cpu().double() - exp).abs().max())
    print(f"C. spatial_softmax n={n} {H}x{W} K={K} T={temp}: {err:.2e} absolute (bound 1.0e-06)")
    assert tuple(got.shape) == (n, K, 2) and err < 1e-6
    if H == 1:
        assert bool((got[..., 1] == -1).all())
    if W == 1:
        assert bool((got[..., 0] == -1).all())


@pytest.mark.parametrize("kind", ["peaked", "offset"])
def test_spatial_softmax_peaked_and_offset_logits(kind):
    g = torch.Generator().manual_seed(11)
    n, H, W, K = 2, 9, 13, 33
    r = torch.randn(n, H * W, K, generator=g)
    lg = r * 30 if kind == "peaked" else r + 1e4
    exp = Hh.spatial_softmax_ref(lg, H, W)
    err = float((ops.spatial_softmax(lg.to(D), H, W).cpu().double() - exp).abs().max())
    print(f"C. spatial_softmax {kind} logits: {err:.2e} absolute (bound 1.0e-06)")
    assert err < 1e-6


@pytest.mark.parametrize("temp", [0.0, -1.0])
def test_spatial_softmax_rejects_temperature(temp):
    with pytest.raises(RuntimeError):
        ops.spatial_softmax(torch.zeros(1, 4, 2, device=D), 2, 2, temperature=temp)
    torch.cuda.synchronize()


# ---- D. unfold1d -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed,k,stride,pad,T", [(False,) + c for c in Hh.UNFOLD_FWD] + [(True,) + c for c in Hh.UNFOLD_TRANSPOSED])
def test_unfold1d_is_the_stated_gather(transposed, k, stride, pad, T):
    """a copy: bit for bit the index arithmetic of the header comment of diffusion.hip (test_kernel_refs_cpu.py contracts that
    reference to F.conv1d / F.conv_transpose1d)"""
    for Cc in (4, 36):
        for B in (1, 3):
            g = torch.Generator().manual_seed(k * 1000 + T * 10 + Cc + B)
            x = torch.randn(B, T, Cc, generator=g)
            exp = Hh.unfold1d_ref(x, k, stride, pad, transposed)
            got = ops.unfold1d(x.to(D), k, stride, pad, transposed=transposed).cpu()
            bad = int((got.view(torch.int32) != exp.view(torch.int32)).sum()) if got.shape == exp.shape else -1
            print(f"D. unfold1d {'transposed ' if transposed else ''}k={k} stride={stride} pad={pad} T={T} C={Cc} B={B}: "
                  f"{bad} of {exp.numel()} words differ (bound 0)")
            assert got.shape == exp.shape and bad == 0
            assert int((exp != 0).sum()) > 0


@pytest.mark.parametrize("Cc,k,stride", [(6, 3, 1), (2, 3, 1), (8, 0, 1), (8, 3, 0)])
def test_unfold1d_rejections(Cc, k, stride):
    x, out = torch.zeros(1, 8, 8, device=D), torch.zeros(1, 16, 64, device=D)   # room for every accepted form of these sizes
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    L.check(lib.actmi_op_unfold1d(p(x), p(out), 1, 8, 8, 3, 1, 1, 8, 0, L.current_stream_ptr()), None, "op_unfold1d")
    with pytest.raises(RuntimeError):
        L.check(lib.actmi_op_unfold1d(p(x), p(out), 1, 8, Cc, k, stride, 1, 8, 0, L.current_stream_ptr()), None, "op_unfold1d")
    torch.cuda.synchronize()


# ---- E. ddim_step and u8_to_nhwc4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_ddim_step(n):
    """DDIMScheduler.step (eta 0, epsilon prediction) in float64.  With alpha_prev = 1 (the last step) the noise term vanishes and
    the result is the clipped x0 itself: exactly +-1 wherever float64 clips, and nowhere beyond"""
    g = torch.Generator().manual_seed(n)
    x, e = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)
    for a_t, a_p in ((0.3, 0.7), (0.0064, 0.05), (0.9, 1.0)):
        for clip in (True, False):
            x0u = (x.double() - (1 - a_t) ** 0.5 * e.double()) / a_t ** 0.5
            x0 = x0u.clamp(-1, 1) if clip else x0u
            exp = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * e.double()
            buf = torch.full((n + 64,), 123.0, device=D)
            buf[:n] = x.to(D)
            got = ops.ddim_step(buf[:n], e.to(D), a_t, a_p, clip=clip).cpu()
            err = rel_err(got, exp)
            print(f"E. ddim_step n={n} alpha_t={a_t} alpha_prev={a_p} clip={clip}: {err:.2e} of max (bound 2.0e-06)")
            assert err < 2e-6
            assert bool((buf[n:] == 123.0).all())                               # nothing behind the n values is written
            if a_p == 1.0 and clip:
                far = x0u.abs() > 1 + 1e-5
                assert torch.equal(got[far].double(), torch.sign(x0u[far])) and float(got.abs().max()) <= 1.0
                if n >= 255:
                    assert bool(far.any()) and not bool(far.all())


@pytest.mark.parametrize("B,Cam,H,W", [(2, 3, 5, 7), (3, 2, 9, 31)])
def test_u8_to_nhwc4(B, Cam, H, W):
    g = torch.Generator().manual_seed(B * 10 + Cam)
    img = torch.randint(0, 256, (B, Cam, H, W, 3), generator=g, dtype=torch.uint8)
    img[0, 0, 0, 0] = torch.tensor([0, 255, 0], dtype=torch.uint8)
    img[-1, -1, -1, -1] = torch.tensor([255, 0, 255], dtype=torch.uint8)
    exp = torch.zeros(Cam, B, H, W, 4)
    exp[..., :3] = (img.double() / 255).float().permute(1, 0, 2, 3, 4)
    got = ops.u8_to_nhwc4(img.to(D)).cpu()
    bad = int((got.view(torch.int32) != exp.view(torch.int32)).sum())
    print(f"E. u8_to_nhwc4 B={B} Cam={Cam} {H}x{W}: {bad} of {exp.numel()} words differ (bound 0)")
    assert got.shape == exp.shape and bad == 0
    assert bool((got[..., 3] == 0).all()) and float(got.max()) == 1.0 and float(got.min()) == 0.0
