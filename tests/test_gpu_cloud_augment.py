"""The device-side point-cloud augmentation on the GPU: actmi_op_cloud_augment against its numpy definition
(actmi.ops.cloud_augment_ref), the CloudAugment class, graph capture, the error returns and forward_pass.

Every equality here is bitwise (torch.equal on xyz, rgb and the counts).  That bar is derived, not measured: the definition fixes
the order of every fp32 product and sum and forbids contraction; numpy on the CPU and the gfx950 VALU both round each of them
correctly; the per-point draws are integer hashes and an exact conversion; the mean is an integer sum divided in double; min and
max pick an operand.

Shapes: P in {1, 2, 63, 64, 65, 257, 1000} -- one row, either side of a wave, either side of a 256-row tile, a ragged tail."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402

DEV = "cuda:0"
SIZES = [1, 2, 63, 64, 65, 257, 1000]
DROPS = [0.0, 0.5, 0.9999999]
PIVOT = (0.25, -0.125, 0.4)
B = 5
GUARD = 64                                                             # sentinel elements in front of and behind every output
SENT_F, SENT_I = 12345.0, -77


def _counts(P):
    return np.array([P, 1, P // 2, max(1, P - 1), 0], np.int32)


@functools.lru_cache(maxsize=None)
def _case(P, drop):
    """inputs (NaN behind the counts), records (all six orders over the launches of a size) and the numpy result for both forms of
    the counts: computed once, shared, read only"""
    rng = np.random.default_rng(1000 * P + int(drop * 10))
    xyz = rng.uniform(-0.8, 0.8, (B, P, 3)).astype(np.float32)
    rgb = rng.uniform(0, 255, (B, P, 3)).astype(np.float32)
    n = _counts(P)
    shift = DROPS.index(drop)                                          # orders 0..4, 1..5, 2..5 + 0: the three drops cover all six
    rec = ops.cloud_augment_records(B, angle=rng.uniform(-5, 5, B), scale=rng.uniform(0.95, 1.05, B),
                                    shift=rng.uniform(-0.01, 0.01, (B, 3)), jitter=0.002, drop=np.float32(drop),
                                    order=(np.arange(B) + shift) % 6, fb=rng.uniform(0.7, 1.3, B), fc=rng.uniform(0.6, 1.4, B),
                                    fs=rng.uniform(0.5, 1.5, B), seed=rng.integers(0, 1 << 64, size=B, dtype=np.uint64))
    exp_full = ops.cloud_augment_ref(xyz, rgb, None, rec, PIVOT)
    exp_n = ops.cloud_augment_ref(xyz, rgb, n, rec, PIVOT)
    xyz_nan, rgb_nan = xyz.copy(), rgb.copy()
    for b in range(B):
        xyz_nan[b, max(int(n[b]), 1):], rgb_nan[b, max(int(n[b]), 1):] = np.nan, np.nan
    for a in (xyz, rgb, xyz_nan, rgb_nan, rec) + exp_full + exp_n:
        a.setflags(write=False)
    return xyz, rgb, xyz_nan, rgb_nan, n, rec, exp_full, exp_n


def _guarded(P):
    """sentinel-guarded outputs: (buffers, views)"""
    m = B * P * 3
    bx = torch.full((m + 2 * GUARD,), SENT_F, dtype=torch.float32, device=DEV)
    bc = torch.full((m + 2 * GUARD,), SENT_F, dtype=torch.float32, device=DEV)
    bn = torch.full((B + 2 * GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    return (bx, bc, bn), (bx[GUARD:GUARD + m].view(B, P, 3), bc[GUARD:GUARD + m].view(B, P, 3), bn[GUARD:GUARD + B])


def _guards_intact(bufs, P):
    m = B * P * 3
    bx, bc, bn = bufs
    return bool((bx[:GUARD] == SENT_F).all() and (bx[GUARD + m:] == SENT_F).all() and (bc[:GUARD] == SENT_F).all() and
                (bc[GUARD + m:] == SENT_F).all() and (bn[:GUARD] == SENT_I).all() and (bn[GUARD + B:] == SENT_I).all())


def _t(a):
    return torch.from_numpy(np.array(a))                               # (a copy: the shared arrays are read-only)


def _equal(got, exp):
    return all(torch.equal(g.cpu(), _t(e)) for g, e in zip(got, exp))


# ---- 1. bitwise equality with the numpy definition -----------------------------------------------------------------------------------
def test_the_cases_cover_all_six_orders():
    assert {int(o) for d in DROPS for o in _case(64, d)[5]["order"]} == set(range(6))


@pytest.mark.parametrize("drop", DROPS)
@pytest.mark.parametrize("P", SIZES)
def test_cloud_augment_is_bitwise_the_numpy_definition(P, drop):
    xyz, rgb, xyz_nan, rgb_nan, n, rec, exp_full, exp_n = _case(P, drop)
    # ragged: counts on the device, NaN behind them
    bufs, out = _guarded(P)
    got = ops.cloud_augment(_t(xyz_nan).to(DEV), _t(rgb_nan).to(DEV), _t(n).to(DEV), rec, PIVOT,
                            out=out)
    torch.cuda.synchronize()
    assert _guards_intact(bufs, P)
    kept = got[2].cpu().numpy()
    print(f"P = {P}, drop = {drop}: kept {kept.tolist()} of {np.clip(n, 1, P).tolist()}")
    assert np.array_equal(kept, exp_n[2])
    assert _equal(got, exp_n)
    assert bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all())
    # counts = NULL: every row is a point
    bufs, out = _guarded(P)
    got = ops.cloud_augment(_t(xyz).to(DEV), _t(rgb).to(DEV), None, rec, PIVOT, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(bufs, P) and _equal(got, exp_full)
    if drop == 0.0:
        assert np.array_equal(got[2].cpu().numpy(), np.full(B, P))
    elif drop > 0.9:
        assert np.array_equal(got[2].cpu().numpy(), np.ones(B))          # row 0 survives a draw that drops everything


def test_identity_and_two_launches_give_the_same_bits():
    P = 257
    xyz, rgb, _, _, n, rec, _, exp_n = _case(P, 0.5)
    t_xyz, t_rgb, t_n = _t(xyz).to(DEV), _t(rgb).to(DEV), _t(n).to(DEV)
    a = ops.cloud_augment(t_xyz, t_rgb, t_n, rec, PIVOT)
    b = ops.cloud_augment(t_xyz, t_rgb, t_n, rec, PIVOT)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and _equal(a, exp_n)
    ident = ops.cloud_augment(t_xyz, t_rgb, None, ops.cloud_augment_records(B), (0, 0, 0))
    assert torch.equal(ident[0], t_xyz) and torch.equal(ident[1], t_rgb) and ident[2].tolist() == [P] * B
    # the class: apply = draw + run, run repeats, set_seed restarts
    aug = ops.CloudAugment(DEV, max_points=300, max_batch=B, pivot=PIVOT, seed=3)
    got = tuple(t.clone() for t in aug.apply(t_xyz, t_rgb, t_n))
    r = aug.records()
    assert len(r) == B and tuple(got[0].shape) == (B, P, 3) and got[0].is_contiguous()
    assert _equal(got, ops.cloud_augment_ref(xyz, rgb, n, r, PIVOT))
    assert all(torch.equal(x, y) for x, y in zip(aug.run(t_xyz, t_rgb, t_n), got))
    again = tuple(t.clone() for t in aug.apply(t_xyz, t_rgb, t_n))
    assert not torch.equal(again[0], got[0]) and not np.array_equal(aug.records(), r)
    aug.set_seed(3)
    assert all(torch.equal(x, y) for x, y in zip(aug.apply(t_xyz, t_rgb, t_n), got))
    with pytest.raises(TypeError):
        aug.run(t_xyz.double(), t_rgb, t_n)
    with pytest.raises(ValueError):
        aug.run(t_xyz, t_rgb[:, :5].contiguous(), t_n)
    with pytest.raises(TypeError):
        aug.run(t_xyz, t_rgb, t_n.long())


# ---- 2. a captured launch reads the records and counts of every replay -----------------------------------------------------------------
def test_captured_graph_replays_with_new_records():
    P = 65
    xyz, rgb, _, _, n, r1, _, _ = _case(P, 0.5)
    r2 = _case(P, 0.0)[5]
    t_xyz, t_rgb, t_n = _t(xyz).to(DEV), _t(rgb).to(DEV), _t(n).to(DEV)
    aug = ops.CloudAugment(DEV, max_points=P, max_batch=B, pivot=PIVOT)
    aug.set_records(r1)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.run(t_xyz, t_rgb, t_n)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):   # one stream, no parallel branches
        out = aug.run(t_xyz, t_rgb, t_n)
    for rec in (r1, r2, r1):
        aug.set_records(rec)                                           # a stream-ordered upload between replays
        for t in out:
            t.zero_()
        graph.replay()
        assert _equal(out, ops.cloud_augment_ref(xyz, rgb, n, rec, PIVOT))


# ---- 3. the error returns ------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_with_a_message_and_launch_nothing():
    lib = L.load()
    P = 16
    xyz, rgb, _, _, n, rec, _, exp_n = _case(64, 0.5)
    xyz, rgb = np.ascontiguousarray(xyz[:, :P]), np.ascontiguousarray(rgb[:, :P])
    t_xyz, t_rgb = torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV)
    t_n = torch.from_numpy(np.minimum(n, P)).to(DEV)
    t_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    bufs, (ox, oc, on) = _guarded(P)
    ptr = {"xyz": t_xyz.data_ptr(), "rgb": t_rgb.data_ptr(), "counts": t_n.data_ptr(), "records": t_rec.data_ptr(),
           "out_xyz": ox.data_ptr(), "out_rgb": oc.data_ptr(), "out_counts": on.data_ptr()}

    def desc(B_=B, P_=P, **over):
        d = L.CloudAugmentDesc()
        for k, v in dict(ptr, **over).items():
            setattr(d, k, v)
        d.B, d.P = B_, P_
        return d
    bad = {f"null {k}": desc(**{k: None}) for k in ptr if k != "counts"}
    bad.update({
        "out_xyz is xyz": desc(out_xyz=ptr["xyz"]), "out_rgb overlaps the end of rgb": desc(out_rgb=ptr["rgb"] + B * P * 12 - 4),
        "out_xyz is rgb": desc(out_xyz=ptr["rgb"]), "out_counts is counts": desc(out_counts=ptr["counts"]),
        "out_rgb is out_xyz": desc(out_rgb=ptr["out_xyz"]), "out_counts inside records": desc(out_counts=ptr["records"] + 8),
        "misaligned xyz": desc(xyz=ptr["xyz"] + 2),
        "B 0": desc(B_=0), "B -1": desc(B_=-1), "B 65536": desc(B_=65536), "P 0": desc(P_=0), "P -3": desc(P_=-3),
        "3 * P beyond int32": desc(B_=1, P_=715827883),
    })
    for name, d in bad.items():
        rc = lib.actmi_op_cloud_augment(C.byref(d), L.current_stream_ptr())
        msg = lib.actmi_op_last_error()
        assert rc == -1 and msg and b"cloud_augment" in msg, (name, rc, msg)          # ACTMI_E_INVALID
    assert lib.actmi_op_cloud_augment(None, L.current_stream_ptr()) == -1 and b"null descriptor" in lib.actmi_op_last_error()
    torch.cuda.synchronize()
    assert all(bool((b == s).all()) for b, s in zip(bufs, (SENT_F, SENT_F, SENT_I)))       # nothing ran
    assert torch.equal(t_xyz.cpu(), torch.from_numpy(xyz)) and torch.equal(t_rgb.cpu(), torch.from_numpy(rgb))
    # the same buffers are fine when asked properly, with and without counts
    for d, cnt in ((desc(), np.minimum(n, P)), (desc(counts=None), None)):
        L.check(lib.actmi_op_cloud_augment(C.byref(d), L.current_stream_ptr()), None, "op_cloud_augment")
        assert not lib.actmi_op_last_error()
        torch.cuda.synchronize()
        assert _guards_intact(bufs, P) and _equal((ox, oc, on), ops.cloud_augment_ref(xyz, rgb, cnt, rec, (0, 0, 0)))


# ---- 4. forward_pass and two optimizer steps at the tiny pcd config ------------------------------------------------------------------------
def _policy():
    from policy import ACTPolicy
    pol = ACTPolicy({"use_pcd": True, "pcd_hidden_dim": 64, "pcd_output_dim": 64, "max_points": 48, "kl_weight": 10, "lr": 1e-4,
                     "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2, "nheads": 4,
                     "camera_names": ["a", "b"], "image_h": 64, "image_w": 96, "base_width": 8}, max_batch=3)
    pol.train()
    pol.train_dropout = 0.0                                            # (the compared calls must draw the same masks: none)
    return pol


def test_two_training_steps_match_steps_fed_the_numpy_definition_by_hand():
    import imitate_episodes as ie
    Bt, P, K, H, W = 3, 37, 2, 64, 96
    rng = np.random.default_rng(21)
    g = torch.Generator().manual_seed(22)
    img = torch.from_numpy(rng.integers(0, 256, (Bt, K, H, W, 3), dtype=np.uint8))
    qpos, act = torch.randn(Bt, 14, generator=g), torch.randn(Bt, 8, 16, generator=g)
    pad = torch.zeros(Bt, 8, dtype=torch.bool)
    pad[:, 6:] = True
    n = torch.tensor([37, 5, 20], dtype=torch.int32)
    xyz = torch.from_numpy(rng.uniform(-0.5, 0.5, (Bt, P, 3)).astype(np.float32))
    rgb = torch.from_numpy(rng.uniform(0, 255, (Bt, P, 3)).astype(np.float32))
    for b in range(Bt):                                                # the loader's zero rows behind the counts
        xyz[b, int(n[b]):], rgb[b, int(n[b]):] = 0, 0
    batch = (img, qpos, act, pad, xyz, rgb, n)
    p1, p2 = _policy(), _policy()
    eps = torch.randn(Bt, p1.model.cfg.latent_in_dim, generator=g).cuda()
    # cloud_augment=None: the code as it stands -- the policy called with the batch's own clouds
    p1.next_eps = eps
    plain = ie.forward_pass(batch, p1, cloud_augment=None)
    p2.next_eps = eps
    direct = p2(qpos.cuda(), img.cuda(), act.cuda(), pad.cuda(), pointcloud={"xyz": xyz.cuda(), "rgb": rgb.cuda(), "n": n.cuda()})
    p2.next_eps = eps
    positional = ie.forward_pass(batch, p2)
    for k in ("l1", "kl", "loss"):
        assert float(plain[k]) == float(direct[k]) == float(positional[k]), k
    aug = ie.make_cloud_augment({"augment_clouds": True, "cloud_pivot": list(PIVOT)}, p1, seed=4)
    assert (aug.max_points, aug.max_batch, aug.pivot) == (48, 3, PIVOT)
    o1, o2 = p1.configure_optimizers(), p2.configure_optimizers()
    losses = []
    for step in range(2):
        o1.zero_grad()
        p1.next_eps = eps
        got = ie.forward_pass(batch, p1, cloud_augment=aug)
        rec = aug.records()
        got["loss"].backward()
        o1.step()
        rx, rc, rn = ops.cloud_augment_ref(xyz.numpy(), rgb.numpy(), n.numpy(), rec, PIVOT)
        assert rn.min() >= 1 and (rn <= n.numpy()).all() and (rn < n.numpy()).any()    # (a tenth dropped: some sample lost a point)
        o2.zero_grad()
        p2.next_eps = eps
        exp = ie.forward_pass((img, qpos, act, pad, torch.from_numpy(rx), torch.from_numpy(rc), torch.from_numpy(rn)), p2)
        exp["loss"].backward()
        o2.step()
        for k in ("l1", "kl", "loss"):
            print(f"step {step} {k}: augmented {float(got[k]):.6f}, plain batch at step 0 {float(plain[k]):.6f}")
            assert np.isfinite(float(got[k])) and float(got[k]) == float(exp[k]), (step, k)
        losses.append(float(got["loss"]))
    assert losses[0] != float(plain["loss"]) and losses[1] != losses[0]
