"""Kernel-level parity of the direct weight-gradient kernels (csrc/wgrad3.hip, csrc/wgrad7.hip) in the launch forms the training
step uses and no other kernel test reaches: persistent workgroups that walk SEVERAL (image, 32-column strip) units, re-run the
prologue and re-seed the LDS ring at every unit boundary and keep accumulating into the same registers; the uneven share; the
launcher's workspace-shrink loop; the accumulating combine.  Reference: torch.nn.grad.conv2d_weight in float64 on the CPU.

The launcher's rule for the workgroup count is restated once (`nwg_rule`); every case asserts the (units, nwg, units per
workgroup) it was written for, and the workspace, pre-filled with a NaN-payload sentinel, must come back with exactly the first
G * nwg partials overwritten in full and nothing behind them, which ties the restated rule to what the launcher did.

1. parity per case (WALK3 / WALK7 below), bitwise repeatable, dy_scale exact; dw is the in-order fp32 sum of the partials; for
   the workspace-limited cases every partial against the float64 result of exactly the units `wg, wg + nwg, ...`;
2. the same operands on the default launch (one unit per workgroup): the two walks differ in summation order only;
3. nothing crosses a unit boundary: with one workgroup walking all units in image order, an image with dy == 0 (or x == 0)
   appended or prepended leaves every bit of the result as it was, the images alternating between 64x and 1/16x unit scale;
4. accumulate=1 (the only form the engine launches): out = r + dw to the bits of an fp32 add, also with `out` 4 bytes into its
   allocation (the combine's scalar path), sentinels on both sides untouched;
5. workload-shaped operands (post-ReLU x with tiny dy under pow2_scale; normalised image with a zero fourth channel and a
   sparse dy), several units per workgroup;
6. rejections (workspace below one partial per group, misaligned dy / x / ws, B = 0): ACTMI_E_INVALID, nothing written;
7. the ops without the new arguments give the bits of the entries without `accumulate`.

Bound: max |got - float64| <= 2e-6 of the tensor's largest magnitude, the bound test_wgrad3x3_c64_matches_torch and
test_wgrad7x7s2_matches_torch hold at up to 2400 contraction pixels; no case here has more.  "Bitwise" is torch.equal.  Every
case prints its error with the bound.

(units, nwg, units per workgroup) reached, and the worst error against float64 measured on an MI355X (bound 2e-6):
  wgrad3 2x5x6x70   k 4: (15, 4, 3..4) 3.6e-7      wgrad7 2x3x9x130   k 3: (9, 3, 3)     4.4e-7
  wgrad3 2x5x6x70   k 7: (15, 7, 2..3) 2.8e-7      wgrad7 2x3x9x130   k 2: (9, 2, 4..5)  4.0e-7
  wgrad3 1x2x5x70   k 1: (6, 1, 6)     5.1e-7      wgrad7 1x3x9x130   k 1: (9, 1, 9)     7.4e-7
  wgrad3 1x7x1x33   k 4: (14, 4, 3..4) 2.6e-7      wgrad7 1x5x2x2     k 2: (5, 2, 2..3)  1.7e-7
  wgrad3 8x1x2x1056 dflt: (33, 32, 1..2) 3.2e-7    wgrad7 16x1x4x2112 dflt: (33, 32, 1..2) 2.6e-7
Worst partial against its own units 5.1e-7 (wgrad3), 7.4e-7 (wgrad7); 2. limited against default walk at most 5.5e-7 (wgrad3),
8.1e-7 (wgrad7, one workgroup against nine); 3. loud / quiet base batches 8.7e-7 and 6.0e-7, all eight zero-image runs bit-equal;
4. bit-equal throughout; 5. 3.4e-7 (wgrad3, pow2_scale 2^31), 2.7e-7 (wgrad7, 2^21), padding channel exactly 0.  The multi-unit
walk of both kernels was found correct: no kernel change came out of these tests.

That the tests bite, on a scratch build in which a workgroup's second and later units reuse its first unit's strip origin (w0 /
wo0 computed from wg instead of u; every address still inside a valid image): test_wgrad3x3_c64_matches_torch and
test_wgrad7x7s2_matches_torch still pass in all ten cases (one unit per workgroup: u == wg), while here 18 of 28 tests fail.
Test 1 against float64 / worst partial against its own units: wgrad3 k 4 5.8e-1 / 5.0e-1, k 7 5.4e-1 / 4.8e-1, k 1 1.4 / 1.4,
default workspace 3.1e-1; wgrad7 k 2 7.3e-1 / 1.0, k 1 1.6 / 1.6, default workspace 3.2e-1.  Test 2 shows the same figures
against the default walk; test 3's base batches 1.6 and 1.7; test 5 5.9e-1 and 6.1e-1; test 6 fails in its closing accepted
call (one workgroup), tests 4 and 7 pass (they compare launches of the same walk).  Three rows are blind to THIS change and
pass under it, because their workgroup count is a multiple of the strips per image, so that wg and u name the same strip:
wgrad3 1x7x1x33 k 4 (2 strips), wgrad7 2x3x9x130 k 3 (3 strips), wgrad7 1x5x2x2 (1 strip); they are kept for what WALK3 /
WALK7 say they cover.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402
from helpers import rel_err  # noqa: E402

BOUND = 2e-6
SENTINEL = 0x7FC12345                                              # a NaN payload: any write shows
E_INVALID = r"\(code -1\)"                                         # ACTMI_E_INVALID as actmi.lib.check reports it


def dev():
    return torch.device("cuda:0")


class Kern:
    """what the two kernels differ in, as the tests see them"""

    def __init__(self, name, op, entry, cap, taps, cin, stride, pad):
        self.name, self.op, self.entry, self.cap = name, op, entry, cap
        self.k, self.cin, self.stride, self.pad = taps, cin, stride, pad
        self.slice = 64 * taps * taps * cin                        # floats of one partial

    def out_hw(self, H, W):
        return (H + 2 * self.pad - self.k) // self.stride + 1, (W + 2 * self.pad - self.k) // self.stride + 1

    def strips(self, W):
        return (self.out_hw(1, W)[1] + 31) // 32

    def dw_shape(self, G):
        return (G, 64, self.k, self.k, self.cin)

    def ref(self, x, dy):
        """float64 dW [O][kh][kw][I] of one group: x [B][H][W][cin], dy [B][Ho][Wo][64]"""
        dw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double(), (64, self.cin, self.k, self.k),
                                         dy.permute(0, 3, 1, 2).double(), stride=self.stride, padding=self.pad)
        return dw.permute(0, 2, 3, 1)


K3 = Kern("wgrad3", ops.wgrad3x3_c64, "actmi_op_wgrad3x3_c64", 256, 3, 64, 1, 1)
K7 = Kern("wgrad7", ops.wgrad7x7s2, "actmi_op_wgrad7x7s2", 512, 7, 4, 2, 3)
KERNS = {"wgrad3": K3, "wgrad7": K7}


def nwg_rule(kern, G, B, W, ws_floats):
    """launch_wgrad3x3_c64 / launch_wgrad7x7s2 restated: -> (units, nwg, fewest, most units per workgroup), nwg None when the
    launch is refused.  cap / G workgroups at most one per unit; then the largest count within a quarter of that which divides
    the units evenly; then shrunk until G * nwg partials fit the workspace.  Workgroup wg walks units wg, wg + nwg, ..."""
    units = B * kern.strips(W)
    nwg = min(max(kern.cap // G, 1), units)
    for d in range(nwg, 0, -1):
        if d * 4 < nwg * 3:
            break
        if units % d == 0:
            nwg = d
            break
    while nwg > 1 and G * nwg * kern.slice > ws_floats:
        nwg -= 1
    if G * nwg * kern.slice > ws_floats:
        return units, None, None, None
    return units, nwg, units // nwg, -(-units // nwg)


def default_partials(kern, G, B, W):
    """the partials per group the ops size their own workspace for"""
    return max(1, min(kern.cap // G, B * kern.strips(W)))


@functools.lru_cache(maxsize=None)
def _case(name, G, B, H, W, seed=0):
    """x, dy ~ randn on the CPU and the float64 dW [G][O][kh][kw][I]; computed once, never modified"""
    kern = KERNS[name]
    g = torch.Generator().manual_seed(seed * 7919 + G * 1000 + B * 100 + H * 10 + W)
    Ho, Wo = kern.out_hw(H, W)
    x = torch.randn(G, B, H, W, kern.cin, generator=g)
    dy = torch.randn(G, B, Ho, Wo, 64, generator=g)
    return x, dy, torch.stack([kern.ref(x[c], dy[c]) for c in range(G)])


def sentinel_ws(kern, G, k):
    """a workspace view of exactly G * k partials inside a sentinel-filled allocation: 4 guard floats in front (the view stays
    16-byte aligned), two guard partials behind -> (whole allocation as int32, the fp32 view handed to the op)"""
    whole = torch.full((4 + (G * k + 2) * kern.slice,), SENTINEL, dtype=torch.int32, device=dev())
    return whole, whole[4:4 + G * k * kern.slice].view(torch.float32)


def written_partials(kern, whole, G, nwg):
    """asserts that exactly the first G * nwg partials behind the front guard were overwritten in full and nothing else was;
    -> the partials [G][nwg][O][kh][kw][I] on the CPU"""
    w = whole.cpu()
    assert bool((w[:4] == SENTINEL).all()), "the workspace was written in front of its first partial"
    body = w[4:].view(-1, kern.slice)
    touched = (body != SENTINEL)
    n = G * nwg
    assert bool(touched[:n].all()), f"{int((~touched[:n]).sum())} words of the first {n} partials were never written"
    behind = touched[n:].any(1).nonzero().flatten().tolist()
    assert not behind, f"partials behind the first {n} were written: {behind}"
    return body[:n].view(torch.float32).view(G, nwg, *kern.dw_shape(G)[1:])


def run_walk(kern, x, dy, k, **kw):
    """the op on a sentinel workspace of k partials per group (None: the default size); checks the restated rule against the
    partials written -> (dw on the CPU, partials on the CPU, (units, nwg, lo, hi))"""
    G, B, W = x.shape[0], x.shape[1], x.shape[3]
    kk = default_partials(kern, G, B, W) if k is None else k
    whole, ws = sentinel_ws(kern, G, kk)
    rule = nwg_rule(kern, G, B, W, ws.numel())
    dw = kern.op(dy, x, ws=ws, **kw)
    torch.cuda.synchronize()
    return dw.cpu(), written_partials(kern, whole, G, rule[1]), rule


def unit_refs(kern, x, dy, nwg):
    """float64 dW of one group restricted to each workgroup's units: dy zeroed outside the unit's 32 output columns, summed over
    the units wg, wg + nwg, ... -> [nwg][O][kh][kw][I]"""
    B, strips = x.shape[0], kern.strips(x.shape[2])
    out = []
    for wg in range(nwg):
        acc = torch.zeros(kern.dw_shape(1)[1:], dtype=torch.float64)
        for u in range(wg, B * strips, nwg):
            im, w0 = u // strips, (u % strips) * 32
            m = torch.zeros_like(dy[im:im + 1])
            m[:, :, w0:w0 + 32] = dy[im:im + 1, :, w0:w0 + 32]
            acc += kern.ref(x[im:im + 1], m)
        out.append(acc)
    return torch.stack(out)


# kernel, (G, B, H, W), max_partials (None = the default workspace), (units, nwg, fewest, most units per workgroup)
WALK3 = [
    ("wgrad3", (2, 5, 6, 70), 4, (15, 4, 3, 4)),           # shrink loop, uneven share, ragged last strip
    ("wgrad3", (2, 5, 6, 70), 7, (15, 7, 2, 3)),           # shrink after an even first choice (15 of 15)
    ("wgrad3", (1, 2, 5, 70), 1, (6, 1, 6, 6)),            # one workgroup walks everything
    ("wgrad3", (1, 7, 1, 33), 4, (14, 4, 3, 4)),           # H = 1: every prologue row but one is padding, at every boundary
    ("wgrad3", (8, 1, 2, 1056), None, (33, 32, 1, 2)),     # multi-unit with the default workspace
]
WALK7 = [
    ("wgrad7", (2, 3, 9, 130), 3, (9, 3, 3, 3)),           # even share, odd H, Wo = 65
    ("wgrad7", (2, 3, 9, 130), 2, (9, 2, 4, 5)),           # uneven share
    ("wgrad7", (1, 3, 9, 130), 1, (9, 1, 9, 9)),           # one workgroup walks everything
    ("wgrad7", (1, 5, 2, 2), 2, (5, 2, 2, 3)),             # 1x1 output map, every unit nearly all padding
    ("wgrad7", (16, 1, 4, 2112), None, (33, 32, 1, 2)),    # multi-unit with the default workspace
]
WALKS = WALK3 + WALK7
LIMITED = [c for c in WALKS if c[2] is not None]


def _id(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-k{c[2] if c[2] is not None else 'default'}"


# ---- 1. parity of every walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,k,want", WALKS, ids=[_id(c) for c in WALKS])
def test_multi_unit_walk_matches_float64(name, shape, k, want):
    kern = KERNS[name]
    x, dy, exp = _case(name, *shape)
    G = shape[0]
    assert kern.out_hw(shape[2], shape[3])[0] * kern.out_hw(shape[2], shape[3])[1] * shape[1] <= 2400          # the bound's range
    xd, dyd = x.to(dev()), dy.to(dev())
    got, parts, rule = run_walk(kern, xd, dyd, k)
    assert rule == want, f"the launcher's rule gives (units, nwg, share) = {rule}, the case was written for {want}"
    assert want[3] >= 2                                            # some workgroup crosses a unit boundary
    errs = [rel_err(got[c], exp[c]) for c in range(G)]
    print(f"1. {_id((name, shape, k))}: units {rule[0]}, nwg {rule[1]}, {rule[2]}..{rule[3]} units per workgroup; "
          f"worst group {max(errs):.2e} (bound {BOUND:.0e})")
    # dw is the fp32 sum of the partials in workgroup order (splitk_combine_kernel), bit for bit
    acc = torch.zeros_like(parts[:, 0])
    for s in range(rule[1]):
        acc = acc + parts[:, s]
    assert torch.equal(got, acc)
    if k is not None:
        # every partial is the float64 result of exactly its own units, on the scale of the whole gradient
        for c in range(G):
            ref = unit_refs(kern, x[c], dy[c], rule[1])
            e = float((parts[c].double() - ref).abs().max() / exp[c].abs().max())
            print(f"   group {c}: worst partial against its own units {e:.2e} (bound {BOUND:.0e})")
            assert e < BOUND, e
    for c in range(G):
        assert errs[c] < BOUND, (c, errs[c])
    again, _, _ = run_walk(kern, xd, dyd, k)
    assert torch.equal(got, again)
    sc = torch.tensor([2.0 ** 20], device=dev())                   # gradients of 1e-6: split after the device-side scale
    got_s, _, _ = run_walk(kern, xd, dyd * 2.0 ** -20, k, dy_scale=sc)
    assert torch.equal(got_s, got * 2.0 ** -20)


# ---- 2. the same operands, one unit per workgroup ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,k,want", LIMITED, ids=[_id(c) for c in LIMITED])
def test_limited_walk_agrees_with_the_default_launch(name, shape, k, want):
    kern = KERNS[name]
    x, dy, exp = _case(name, *shape)
    G, B, _, W = shape
    xd, dyd = x.to(dev()), dy.to(dev())
    limited = kern.op(dyd, xd, max_partials=k).cpu()               # the op's own workspace of k partials per group
    walked, _, rule = run_walk(kern, xd, dyd, k)
    assert rule == want
    assert torch.equal(limited, walked)                            # max_partials=k and a caller's ws of that size: one launch form
    units, nwg, lo, hi = nwg_rule(kern, G, B, W, G * default_partials(kern, G, B, W) * kern.slice)
    assert (nwg, lo, hi) == (units, 1, 1)                          # the default launch: the form the older tests cover
    default = kern.op(dyd, xd).cpu()
    errs = [rel_err(limited[c], default[c]) for c in range(G)]
    print(f"2. {_id((name, shape, k))}: {want[1]} workgroups against {units}: worst group {max(errs):.2e} (bound {BOUND:.0e}); "
          f"default against float64 {max(rel_err(default[c], exp[c]) for c in range(G)):.2e}")
    assert max(errs) < BOUND, errs


# ---- 3. nothing crosses a unit boundary -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", [("wgrad3", (2, 3, 5, 70)), ("wgrad7", (2, 3, 9, 130))], ids=["wgrad3", "wgrad7"])
def test_a_zero_image_changes_no_bit(name, shape):
    """k = 1: one workgroup per group walks all units in image order into one partial, so a unit that contributes exact zeros
    must leave every bit alone wherever it stands -- unless a ring slot or dY buffer of a neighbouring unit leaks into it.  The
    images alternate between 64x and 1/16x unit scale (both operands), the zero image's non-zero operand is loud."""
    kern = KERNS[name]
    G, B, H, W = shape
    x, dy, _ = _case(name, G, B, H, W, seed=3)
    amp = torch.tensor([64.0 if i % 2 == 0 else 1.0 / 16 for i in range(B)]).view(1, B, 1, 1, 1)
    x, dy = x * amp, dy * amp
    g = torch.Generator().manual_seed(77)
    loud_x, loud_dy = torch.randn(x[:, :1].shape, generator=g) * 64, torch.randn(dy[:, :1].shape, generator=g) * 64
    assert kern.strips(W) * 32 != kern.out_hw(H, W)[1] and kern.strips(W) > 1          # a ragged last strip
    base, _, rule = run_walk(kern, x.to(dev()), dy.to(dev()), 1)
    assert rule == (B * kern.strips(W), 1, B * kern.strips(W), B * kern.strips(W))
    exp = torch.stack([kern.ref(x[c], dy[c]) for c in range(G)])
    err = max(rel_err(base[c], exp[c]) for c in range(G))
    print(f"3. {name} {shape}: base batch against float64 {err:.2e} (bound {BOUND:.0e})")
    assert err < BOUND, err
    zero = {"dy == 0": (loud_x, torch.zeros_like(loud_dy)), "x == 0": (torch.zeros_like(loud_x), loud_dy)}
    for what, (zx, zdy) in zero.items():
        for where, cat in (("appended", lambda a, z: torch.cat([a, z], 1)), ("prepended", lambda a, z: torch.cat([z, a], 1))):
            got, _, r = run_walk(kern, cat(x, zx).to(dev()), cat(dy, zdy).to(dev()), 1)
            assert r[1] == 1 and r[0] == (B + 1) * kern.strips(W)
            same = torch.equal(got, base)
            print(f"   image with {what} {where}: bitwise equal {same}, max |difference| {float((got - base).abs().max()):.2e}")
            assert same, f"{name}: an image with {what} {where} changed the result"


# ---- 4. the engine's form: accumulate into dw -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,k", [("wgrad3", (2, 5, 6, 70), 4), ("wgrad7", (2, 3, 9, 130), 2)], ids=["wgrad3", "wgrad7"])
def test_accumulate_adds_the_result_last(name, shape, k):
    kern = KERNS[name]
    x, dy, _ = _case(name, *shape)
    G = shape[0]
    xd, dyd = x.to(dev()), dy.to(dev())
    plain, _, _ = run_walk(kern, xd, dyd, k)
    r = torch.randn(kern.dw_shape(G), generator=torch.Generator().manual_seed(5)) * float(plain.abs().max())
    want = r + plain                                               # one fp32 add per element on the CPU
    out = r.to(dev())
    got, _, _ = run_walk(kern, xd, dyd, k, out=out, accumulate=True)
    print(f"4. {name}: accumulate == r + dw bitwise: {torch.equal(got, want)}")
    assert torch.equal(got, want)
    # out = a view 4 bytes into its allocation: the combine's scalar path; accumulating and overwriting
    n = want.numel()
    for accumulate, expect in ((True, want), (False, plain)):
        buf = torch.full((n + 2,), SENTINEL, dtype=torch.int32, device=dev())
        view = buf[1:1 + n].view(torch.float32).view(kern.dw_shape(G))
        assert view.data_ptr() % 16 == 4
        view.copy_(r)
        run_walk(kern, xd, dyd, k, out=view, accumulate=accumulate)
        b = buf.cpu()
        same = torch.equal(b[1:1 + n].view(torch.float32).view(kern.dw_shape(G)), expect)
        print(f"   out 4 bytes into its allocation, accumulate={accumulate}: bitwise equal {same}")
        assert same
        assert int(b[0]) == SENTINEL and int(b[-1]) == SENTINEL, "the combine wrote outside the view"


# ---- 5. workload-shaped operands --------------------------------------------------------------------------------------------
def test_wgrad3_post_relu_input_and_tiny_gradients():
    """layer1 as the training step meets it: x after a ReLU (half zeros, non-negative, up to about 30), dy about 1e-6 under the
    device-side pow2_scale; 12 units over 4 workgroups per group (3 strips per image: a workgroup changes strip at every unit)"""
    G, B, H, W, k = 2, 4, 6, 70, 4
    g = torch.Generator().manual_seed(51)
    x = torch.relu(torch.randn(G, B, H, W, 64, generator=g) * 8)
    dy = torch.randn(G, B, H, W, 64, generator=g) * 1e-6
    assert 0.45 < float((x == 0).float().mean()) < 0.55 and 25 < float(x.max()) < 50
    dyd = dy.to(dev())
    sc = ops.pow2_scale(dyd.view(-1, 64))
    got, _, rule = run_walk(K3, x.to(dev()), dyd, k, dy_scale=sc)
    assert rule == (12, 4, 3, 3)
    assert 2.0 ** 13 <= float(sc[0].cpu()) * float(dy.abs().max()) < 2.0 ** 14
    errs = [rel_err(got[c], K3.ref(x[c], dy[c])) for c in range(G)]
    print(f"5. wgrad3 post-ReLU x, dy 1e-6 with pow2_scale {float(sc[0].cpu()):.0f}: {max(errs):.2e} (bound {BOUND:.0e})")
    assert max(errs) < BOUND, errs


def test_wgrad7_normalised_image_and_sparse_gradients():
    """the stem as the training step meets it: x the normalised image range [-2.2, 2.7] with the fourth (padding) channel exactly
    0, dy with three quarters zeros as behind the max-pool backward, under pow2_scale; 12 units over 4 workgroups per group (3
    strips per image: a workgroup changes strip at every unit).  The padding channel's gradient is exactly 0."""
    G, B, H, W, k = 2, 4, 10, 132, 4
    g = torch.Generator().manual_seed(52)
    Ho, Wo = K7.out_hw(H, W)
    x = torch.rand(G, B, H, W, 4, generator=g) * 4.9 - 2.2
    x[..., 3] = 0.0
    dy = torch.randn(G, B, Ho, Wo, 64, generator=g) * 1e-3 * (torch.rand(G, B, Ho, Wo, 64, generator=g) < 0.25)
    assert 0.72 < float((dy == 0).float().mean()) < 0.78
    dyd = dy.to(dev())
    sc = ops.pow2_scale(dyd.view(-1, 64))
    got, _, rule = run_walk(K7, x.to(dev()), dyd, k, dy_scale=sc)
    assert rule == (12, 4, 3, 3)
    errs = [rel_err(got[c], K7.ref(x[c], dy[c])) for c in range(G)]
    print(f"5. wgrad7 normalised image, sparse dy with pow2_scale {float(sc[0].cpu()):.0f}: {max(errs):.2e} (bound {BOUND:.0e}); "
          f"padding channel max |dw| {float(got[..., 3].abs().max()):.1e}")
    assert max(errs) < BOUND, errs
    assert torch.equal(got[..., 3], torch.zeros_like(got[..., 3]))


# ---- 6. rejections ----------------------------------------------------------------------------------------------------------
def _off4(t):
    """a dense copy of t on the device that starts 4 bytes into its allocation"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev())
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("name,shape", [("wgrad3", (2, 2, 3, 40)), ("wgrad7", (2, 2, 6, 70))], ids=["wgrad3", "wgrad7"])
def test_rejections_launch_nothing(name, shape):
    kern = KERNS[name]
    x, dy, _ = _case(name, *shape)
    G = shape[0]
    xd, dyd = x.to(dev()), dy.to(dev())

    def refused(what, x_, dy_, ws_whole, ws_):
        out = torch.full(kern.dw_shape(G), SENTINEL, dtype=torch.int32, device=dev())
        with pytest.raises(RuntimeError, match=E_INVALID):
            kern.op(dy_, x_, ws=ws_, out=out.view(torch.float32))
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), f"{what}: dw was written"
        assert bool((ws_whole == SENTINEL).all()), f"{what}: the workspace was written"
        print(f"6. {name} {what}: ACTMI_E_INVALID, dw and workspace untouched")

    # one float short of one partial per group, and no workspace at all
    whole, ws = sentinel_ws(kern, G, 1)
    refused("workspace one float below one partial per group", xd, dyd, whole, ws[:-1])
    refused("empty workspace", xd, dyd, whole, ws[:0])
    # misaligned operands
    refused("dy 4 bytes off", xd, _off4(dyd), whole, ws)
    refused("x 4 bytes off", _off4(xd), dyd, whole, ws)
    big = torch.full((8 + G * kern.slice,), SENTINEL, dtype=torch.int32, device=dev())
    refused("ws 4 bytes off", xd, dyd, big, big[1:1 + G * kern.slice].view(torch.float32))
    # B = 0
    refused("B = 0", xd[:, :0].contiguous(), dyd[:, :0].contiguous(), whole, ws)
    # and the same operands are accepted once nothing is wrong with them
    got = kern.op(dyd, xd, ws=ws)
    assert rel_err(got, _case(name, *shape)[2]) < BOUND


# ---- 7. the defaults are the entries without `accumulate` -------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", [("wgrad3", (2, 5, 6, 70)), ("wgrad7", (2, 3, 9, 130))], ids=["wgrad3", "wgrad7"])
def test_default_arguments_give_the_bits_of_the_plain_entry(name, shape):
    kern = KERNS[name]
    x, dy, _ = _case(name, *shape)
    G, B, H, W = shape
    xd, dyd = x.to(dev()), dy.to(dev())
    ws = torch.empty(G * default_partials(kern, G, B, W) * kern.slice, device=dev(), dtype=torch.float32)
    dw = torch.empty(kern.dw_shape(G), device=dev(), dtype=torch.float32)
    p = lambda t: C.c_void_p(t.data_ptr())                         # noqa: E731
    L.check(getattr(L.load(), kern.entry)(p(dyd), p(xd), p(dw), p(ws), ws.numel(), None, G, B, H, W, L.current_stream_ptr()),
            None, kern.entry)
    plain = dw.cpu()
    assert bool(torch.isfinite(plain).all()) and torch.equal(kern.op(dyd, xd).cpu(), plain)
    sc, small = torch.tensor([2.0 ** 20], device=dev()), dyd * 2.0 ** -20
    L.check(getattr(L.load(), kern.entry)(p(small), p(xd), p(dw), p(ws), ws.numel(), p(sc), G, B, H, W, L.current_stream_ptr()),
            None, kern.entry)
    scaled = dw.cpu()
    assert torch.equal(scaled, plain * 2.0 ** -20) and torch.equal(kern.op(small, xd, dy_scale=sc).cpu(), scaled)
