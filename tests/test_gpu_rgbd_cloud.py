"""RGB-D frames fused into the policy's point cloud on the device: actmi_op_rgbd_cloud / ops.RGBDFusion, the policy and engine
surface (pointcloud={"depth": frames}), graph capture, the host-fed pipeline and the error returns.

The oracle (`fuse_oracle`) is a float64 numpy TRANSCRIPTION of the reference's fusion node,
aloha_scripts/jie_aloha_scripts/pcd_fusion.py:201-243 (4x4 camera -> base_link transform, crop to spatial_cutoff with both ends
inclusive, random subset of downsample_N points per camera) and :278-279 (concatenation of the cameras), in front of it the
pinhole deprojection of the sensor driver that produces the node's input (z = d * depth_scale, x = (u - cx) / fx * z,
y = (v - cy) / fy * z; `remove_nans` drops the pixels without a depth).  The node imports rospy and cannot be called here, so
this is a restatement, as for the temporal ensemble.  Where the reference draws `np.random.choice`, the library's draw is the
quota smallest values of the documented key (ops.rgbd_select_key): the oracle applies that key to ITS OWN survivors.

Tolerances.  Coordinates 1e-5 m absolute: about 8 fp32 roundings on sums of magnitude |x| + |y| + |z| + |t|; the scenes keep
depth <= 4000 units of 1 mm and |t| <= 2 m, so that sum stays under 10 m: 8 * 2^-24 * 10 = 5e-6.  Colours, counts, indices and
the row order: exact.  Crop membership near a face could flip between fp32 and float64, so the scenes are built (on the CPU) with
no oracle point within 1e-4 m of a face -- offending depth values are nudged by one unit until that holds, and it is asserted --
which makes the share of points left out of a comparison zero."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_fixture, regenerate  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402
from actmi import weights as W  # noqa: E402
from actmi.config import tiny_config  # noqa: E402
from actmi.engine import ACTEngine, InferPipeline  # noqa: E402

XYZ_ATOL = 1e-5
FACE_MARGIN = 1e-4
DEPTH_SCALE = 1e-3
DEV = "cuda:0"


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def _points(depth_k, intr, ds, T):
    """float64 points [H*W, 3] in the base frame and the valid mask of one depth frame (pinhole; pcd_fusion.py:201-208)"""
    H, W = depth_k.shape
    v, u = np.divmod(np.arange(H * W), W)
    d = depth_k.reshape(-1).astype(np.float64)
    fx, fy, cx, cy = (float(a) for a in intr)
    z = d * float(ds)
    x = (u - cx) / fx * z
    y = (v - cy) / fy * z
    T = np.asarray(T, dtype=np.float64)[:3]
    p = np.stack([x, y, z], 1) @ T[:, :3].T + T[:, 3]
    return p, d != 0


def _inside(p, box):
    b = np.asarray(box, dtype=np.float64)
    return ((p >= b[0::2]) & (p <= b[1::2])).all(1)                    # pcd_fusion.py:211-226, both ends inclusive


def fuse_oracle(depth, image, cam_index, intr, ds, T, box, quota, seed):
    B, K, H, W = depth.shape
    P = int(sum(quota))
    out = dict(xyz=np.zeros((B, P, 3)), rgb=np.zeros((B, P, 3), np.float32), n=np.zeros(B, np.int32),
               src_idx=np.full((B, P), -1, np.int32), survivors=np.zeros((B, K), np.int32), surv=[[None] * K for _ in range(B)])
    for b in range(B):
        r = 0
        for k in range(K):
            p, valid = _points(depth[b, k], intr[k], ds, T[k])
            surv = np.nonzero(valid & _inside(p, box))[0]
            out["survivors"][b, k] = len(surv)
            out["surv"][b][k] = surv
            keep = surv
            if len(surv) > quota[k]:                                   # pcd_fusion.py:229-241, with the library's documented draw
                key = ops.rgbd_select_key(seed, b, k, surv, H, W)
                keep = np.sort(surv[np.argsort(key, kind="stable")[:quota[k]]])
            m = len(keep)
            out["xyz"][b, r:r + m] = p[keep]
            out["rgb"][b, r:r + m] = image[b, cam_index[k]].reshape(-1, 3)[keep].astype(np.float32)
            out["src_idx"][b, r:r + m] = k * H * W + keep
            r += m                                                     # pcd_fusion.py:278-279: the cameras, concatenated
        out["n"][b] = r
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _extrinsics(K, flavour=0):
    T = np.zeros((K, 3, 4))
    for k in range(K):
        T[k, :, :3] = _rot([1.0 + k, -0.5 + flavour, 0.7], 0.4 + 0.35 * k + 0.2 * flavour)
        t = np.array([0.3 - 0.5 * k, -0.2 + 0.1 * flavour, 0.6 + 0.2 * k])
        T[k, :, 3] = t
        assert np.linalg.norm(t) <= 2.0 and np.abs(T[k, :, :3] - np.eye(3)).max() > 0.1
    return T


def _margin(depth, intr, T, box):
    """smallest distance of a valid pixel's point to a face of the box, and the pixels closer than FACE_MARGIN"""
    B, K, H, W = depth.shape
    near = np.zeros(depth.shape, bool)
    lo = np.inf
    faces = np.asarray(box, dtype=np.float64)
    for b in range(B):
        for k in range(K):
            p, valid = _points(depth[b, k], intr[k], DEPTH_SCALE, T[k])
            dist = np.abs(np.repeat(p, 2, axis=1) - faces).min(1)
            dist[~valid] = np.inf
            lo = min(lo, float(dist.min()))
            near[b, k] = (dist < FACE_MARGIN).reshape(H, W)
    return lo, near


@functools.lru_cache(maxsize=None)
def scene(H, W, B=3, K=2, Cn=2, seed=0, flavour=0):
    """frames, calibration and a box that about a quarter of the pixels survive; no oracle point within FACE_MARGIN of a face"""
    g = np.random.default_rng(1000 * H + W + 7 * seed)
    depth = g.integers(300, 4001, size=(B, K, H, W)).astype(np.uint16)
    depth[g.random((B, K, H, W)) < 0.4] = 0                           # pixels without a depth
    image = g.integers(0, 256, size=(B, Cn, H, W, 3), dtype=np.uint8)
    intr = np.array([[0.8 * W + 3 * k, 0.8 * W - 2 * k, W / 2 - 0.5 + 0.3 * k, H / 2 - 0.5 - 0.2 * k] for k in range(K)])
    T = _extrinsics(K, flavour)
    cam_index = [(K - 1 - k) % Cn for k in range(K)]                   # [1, 0]: a swapped colour source shows
    pts = np.concatenate([_points(depth[0, k], intr[k], DEPTH_SCALE, T[k])[0][depth[0, k].reshape(-1) != 0] for k in range(K)])
    q = np.quantile(pts, [0.2, 0.8, 0.1, 0.9, 0.1, 0.9], axis=0)
    box = tuple(float(np.round(v, 3)) for v in (q[0, 0], q[1, 0], q[2, 1], q[3, 1], q[4, 2], q[5, 2]))
    for i in range(12):
        lo, near = _margin(depth, intr, T, box)
        if not near.any():
            break
        # one unit further along the ray; a ray that runs almost parallel to the face it is near loses its depth instead
        depth[near] = np.where(depth[near] < 4000, depth[near] + 1, depth[near] - 7) if i < 8 else 0
    lo, near = _margin(depth, intr, T, box)
    assert lo >= FACE_MARGIN and not near.any() and int(depth.max()) <= 4000
    return dict(depth=depth, image=image, intr=intr, T=T, box=box, cam_index=cam_index, H=H, W=W, B=B, K=K, C=Cn)


def make_fusion(sc, quota, target=DEV, seed=0, max_batch=None):
    return ops.RGBDFusion(target, sc["K"], sc["H"], sc["W"], sc["cam_index"], sc["intr"], DEPTH_SCALE, sc["T"], sc["box"], quota,
                          max_batch=max_batch or sc["B"], num_cams=sc["C"], seed=seed)


def run_op(sc, quota, seed=0, fusion=None, depth=None):
    f = fusion or make_fusion(sc, quota, seed=seed)
    depth = sc["depth"] if depth is None else depth
    out = f.fuse(torch.from_numpy(sc["image"]).to(DEV), torch.from_numpy(depth).to(DEV), depth.shape[0])
    torch.cuda.synchronize()
    B = depth.shape[0]
    res = {k: v.cpu().numpy().copy() for k, v in out.items()}
    res["src_idx"], res["survivors"] = f.src_idx[:B].cpu().numpy().copy(), f.survivors[:B].cpu().numpy().copy()
    return res


def oracle_of(sc, quota, seed=0, depth=None, T=None):
    return fuse_oracle(sc["depth"] if depth is None else depth, sc["image"], sc["cam_index"], sc["intr"], DEPTH_SCALE,
                       sc["T"] if T is None else T, sc["box"], list(quota), seed)


def check_rows(got, ref, what):
    """row for row: exact counts, indices, order and colours; coordinates to XYZ_ATOL; padding exactly zero"""
    assert np.array_equal(got["survivors"], ref["survivors"]), what
    assert np.array_equal(got["n"], ref["n"]), what
    assert np.array_equal(got["src_idx"], ref["src_idx"]), what
    assert np.array_equal(got["rgb"], ref["rgb"]), what
    err = float(np.abs(got["xyz"].astype(np.float64) - ref["xyz"]).max())
    print(f"{what}: n = {ref['n'].tolist()}, survivors = {ref['survivors'].tolist()}, max |xyz - oracle| = {err:.3e} m")
    assert err <= XYZ_ATOL, what
    for b, n in enumerate(ref["n"]):
        assert not got["xyz"][b, n:].any() and not got["rgb"][b, n:].any() and (got["src_idx"][b, n:] == -1).all(), what


SIZES = [(64, 96), (37, 53)]                                           # six tiles of 1024 pixels; a ragged last tile, odd width, m = 11
BELOW = {(64, 96): [2048, 1800], (37, 53): [700, 600]}
ABOVE = {(64, 96): [300, 257], (37, 53): [100, 33], (120, 160): [1000, 999]}


# ---- 1. every survivor kept -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_all_survivors_kept_match_oracle_row_for_row(H, W):
    sc, quota = scene(H, W), BELOW[(H, W)]
    ref = oracle_of(sc, quota)
    assert (ref["survivors"] < np.asarray(quota)).all() and (ref["survivors"] > 50).all()
    got = run_op(sc, quota)
    check_rows(got, ref, f"{H}x{W} below quota")
    assert np.array_equal(got["n"], ref["survivors"].sum(1))


# ---- 2. downsampling ------------------------------------------------------------------------------------------------------------
def _check_downsampled(sc, quota, seed, what):
    H, W, B, K = sc["H"], sc["W"], sc["depth"].shape[0], sc["K"]
    ref = oracle_of(sc, quota, seed)
    assert (ref["survivors"] > np.asarray(quota)).all(), (what, ref["survivors"])
    got = run_op(sc, quota, seed)
    for b in range(B):
        idx = got["src_idx"][b]
        assert got["n"][b] == sum(quota) and (np.diff(idx) > 0).all(), what             # strictly increasing within the sample
        for k in range(K):
            mine = idx[(idx >= k * H * W) & (idx < (k + 1) * H * W)] - k * H * W
            surv = ref["surv"][b][k]
            assert len(mine) == quota[k] and np.isin(mine, surv).all(), what             # exactly the quota, survivors only
            key = ops.rgbd_select_key(seed, b, k, surv, H, W)
            assert np.array_equal(mine, np.sort(surv[np.argsort(key, kind="stable")[:quota[k]]])), what
    check_rows(got, ref, what)
    return got


@pytest.mark.parametrize("H,W", SIZES + [(120, 160)])                 # 120 x 160: both histogram levels carry several keys
def test_downsampled_set_is_the_quota_smallest_keys(H, W):
    _check_downsampled(scene(H, W), ABOVE[(H, W)], seed=12345, what=f"{H}x{W} above quota")


def test_downsampled_vga_frame_more_tiles_than_one_scan_chunk():
    """480 x 640, the deployment size: 300 tiles (the scan walks them in two chunks of 256), m = 19, plane offsets that are
    multiples of four pixels (the 8-byte depth loads)"""
    sc = scene(480, 640, B=1, K=1, Cn=1)
    _check_downsampled(sc, [2048], seed=99, what="480x640 above quota")


# ---- 3. seeds -------------------------------------------------------------------------------------------------------------------
def test_same_seed_is_bitwise_repeatable_and_another_seed_another_set():
    sc, quota = scene(64, 96), ABOVE[(64, 96)]
    f = make_fusion(sc, quota, seed=7)
    a, b = run_op(sc, quota, fusion=f), run_op(sc, quota, fusion=f)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    f.set_seed(8)
    c = run_op(sc, quota, fusion=f)
    assert np.array_equal(c["n"], a["n"]) and np.array_equal(c["survivors"], a["survivors"])
    assert (c["src_idx"] != a["src_idx"]).mean() > 0.5
    check_rows(c, oracle_of(sc, quota, 8), "seed 8")
    f.set_seed((1 << 64) - 3)                                          # the whole 64-bit word reaches the device
    check_rows(run_op(sc, quota, fusion=f), oracle_of(sc, quota, (1 << 64) - 3), "seed 2^64 - 3")


# ---- 4. edge cases ----------------------------------------------------------------------------------------------------------------
def test_empty_camera_empty_sample_and_quota_one():
    sc = scene(37, 53)
    depth = sc["depth"].copy()
    depth[1, 0] = 0                                                    # sample 1: camera 0 sees nothing
    depth[2] = 0                                                       # sample 2: no depth at all
    quota = [100, 33]
    ref = oracle_of(sc, quota, 3, depth=depth)
    got = run_op(sc, quota, 3, depth=depth)
    check_rows(got, ref, "empty camera / empty sample")
    assert ref["survivors"][1, 0] == 0 and got["src_idx"][1, 0] >= 37 * 53              # camera 1's rows start at row 0
    assert got["n"][1] == quota[1] and got["n"][2] == 0
    assert not got["xyz"][2].any() and not got["rgb"][2].any() and (got["survivors"][2] == 0).all()
    one = run_op(sc, [1, 1], 3, depth=depth)
    check_rows(one, oracle_of(sc, [1, 1], 3, depth=depth), "quota 1")
    assert one["n"].tolist() == [2, 1, 0]


def test_point_exactly_on_a_box_face_is_kept():
    """identity rotation, power-of-two calibration: x = 32 / 64 * 2 = 1, y = -16 / 64 * 2 = -0.5, z = 2048 * 2^-10 = 2 without any
    rounding, each ON a face of the box; the neighbour one pixel further out (x = 33 / 32) is dropped"""
    H, W = 37, 53
    depth = np.zeros((1, 1, H, W), np.uint16)
    depth[0, 0, 4, 40] = 2048
    depth[0, 0, 4, 41] = 2048
    depth[0, 0, 20, 8] = 1024                                          # the optical axis: (0, 0, 1), on the near face
    image = np.random.default_rng(5).integers(0, 256, size=(1, 1, H, W, 3), dtype=np.uint8)
    T = np.eye(4)[None, :3]
    f = ops.RGBDFusion(DEV, 1, H, W, [0], [[64.0, 64.0, 8.0, 20.0]], 2.0 ** -10, T, (-1.0, 1.0, -0.5, 0.5, 1.0, 2.0), [8], max_batch=1)
    out = f.fuse(torch.from_numpy(image).to(DEV), torch.from_numpy(depth).to(DEV), 1)
    assert out["n"].tolist() == [2] and f.survivors.tolist() == [[2]]
    assert f.src_idx[0, :3].tolist() == [4 * W + 40, 20 * W + 8, -1]
    assert out["xyz"][0, :2].tolist() == [[1.0, -0.5, 2.0], [0.0, 0.0, 1.0]]
    assert np.array_equal(out["rgb"][0, 0].cpu().numpy(), image[0, 0, 4, 40].astype(np.float32))


# ---- 5. policy, graph, pipeline ---------------------------------------------------------------------------------------------------
POL_QUOTA = [40, 24]                                                   # above-quota cameras: the draw is part of what is compared


@pytest.fixture(scope="module")
def pcd_engine():
    z, cfg = load_fixture("tiny_pcd")
    sd_np, inp = regenerate(z, cfg)
    B = int(z["batch"])
    assert (cfg.image_h, cfg.image_w, cfg.num_cams) == (64, 96, 2)
    sc = scene(64, 96, B=B, seed=3)
    eng = ACTEngine(cfg, max_batch=B, training=True, max_points=sum(POL_QUOTA))
    eng.load_state_dict(sd_np)
    eng.finalize()
    fusion = ops.RGBDFusion(eng, sc["K"], 64, 96, sc["cam_index"], sc["intr"], DEPTH_SCALE, sc["T"], sc["box"], POL_QUOTA, seed=11)
    d = eng.device
    t = {k: torch.from_numpy(inp[k]).to(d) for k in ("qpos", "image_u8", "actions", "is_pad")}
    t["eps"] = torch.from_numpy(z["train.eps"]).to(d)
    sc = dict(sc, image=inp["image_u8"])                               # the cloud's colours come from the forward's own frames
    return eng, fusion, sc, t


def _oracle_cloud(sc, dev, seed=11, depth=None, T=None):
    ref = oracle_of(sc, POL_QUOTA, seed, depth=depth, T=T)
    return {"xyz": torch.from_numpy(ref["xyz"].astype(np.float32)).to(dev), "rgb": torch.from_numpy(ref["rgb"]).to(dev),
            "n": torch.from_numpy(ref["n"]).to(dev)}


def test_policy_accepts_depth_frames_infer_and_train(pcd_engine):
    eng, fusion, sc, t = pcd_engine
    d = eng.device
    depth = torch.from_numpy(sc["depth"]).to(d)
    with pytest.raises(ValueError, match="set_rgbd_fusion"):           # fuse before set_rgbd_fusion
        eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": depth})
    with pytest.raises(ValueError, match="set_rgbd_fusion"):
        eng.capture_infer(sc["B"], fuse_depth=True)
    eng.set_rgbd_fusion(fusion)
    try:
        a_depth = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": depth}).clone()
        a_5d = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": depth.unsqueeze(2)}).clone()
        cloud = fusion.fuse(t["image_u8"], depth, sc["B"])
        a_fused = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud=cloud).clone()
        assert torch.equal(a_depth, a_fused) and torch.equal(a_5d, a_fused)
        a_ref = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud=_oracle_cloud(sc, d))
        err = float((a_depth - a_ref).abs().max())
        print(f"a_hat: fused on the device vs fed the oracle's cloud: {err:.3e}")
        assert err <= 1e-4 and float(a_ref.abs().max()) > 0
        # a ready-made cloud still goes through as before, and the float frames cannot colour a cloud
        with pytest.raises(ValueError, match="RGBDFusion"):
            eng.forward_infer(t["qpos"], torch.from_numpy(W.u8_nhwc_to_f32_nchw(sc["image"])).to(d), pointcloud={"depth": depth})
        # training: the three losses
        def losses(pc):
            out = eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], eps=t["eps"], pointcloud=pc)
            return torch.stack([out["l1"], out["kl"], out["loss"]]).clone()
        l_depth = losses({"depth": depth})
        l_fused = losses(fusion.fuse(t["image_u8"], depth, sc["B"]))
        l_ref = losses(_oracle_cloud(sc, d))
        assert torch.equal(l_depth, l_fused)
        print(f"losses: fused {l_depth.tolist()} oracle cloud {l_ref.tolist()}")
        for got, exp in zip(l_depth.tolist(), l_ref.tolist()):
            assert abs(got - exp) <= 1e-4 * max(1.0, abs(exp))
        eng.zero_grad()
        eng.backward(1.0)                                              # the backward reads the fusion's buffers again
        assert torch.isfinite(eng.grad_arena()).all()
        # the policy surface
        from policy import ACTPolicy
        pol = ACTPolicy({"use_pcd": True, "pcd_hidden_dim": 64, "pcd_output_dim": 64, "max_points": sum(POL_QUOTA), "kl_weight": 10,
                         "lr": 1e-5, "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2,
                         "nheads": 4, "camera_names": ["a", "b"], "image_h": 64, "image_w": 96, "base_width": 8, "training": False},
                        max_batch=sc["B"])
        with pytest.raises(ValueError, match="set_rgbd_fusion"):       # {"depth": ...} given to an engine without a fusion
            pol(t["qpos"], t["image_u8"], pointcloud={"depth": depth})
        pf = ops.RGBDFusion(pol.model, sc["K"], 64, 96, sc["cam_index"], sc["intr"], DEPTH_SCALE, sc["T"], sc["box"], POL_QUOTA, seed=11)
        pol.set_rgbd_fusion(pf)
        p_depth = pol(t["qpos"], t["image_u8"], pointcloud={"depth": depth}).clone()
        p_fused = pol(t["qpos"], t["image_u8"], pointcloud=pf.fuse(t["image_u8"], depth, sc["B"]))
        assert torch.equal(p_depth, p_fused)
    finally:
        eng.set_rgbd_fusion(None)


def test_captured_graph_sees_new_frames_extrinsics_and_seed(pcd_engine):
    eng, fusion, sc, t = pcd_engine
    d, B = eng.device, sc["B"]
    eng.set_rgbd_fusion(fusion)
    try:
        replay = eng.capture_infer(B, fuse_depth=True)
        s_depth = replay.static_cloud["depth"]
        assert s_depth.dtype == torch.uint16 and tuple(s_depth.shape) == (B, 2, 64, 96)
        d1 = torch.from_numpy(sc["depth"]).to(d)
        d2 = torch.from_numpy(scene(64, 96, B=B, seed=4)["depth"]).to(d)

        def both(depth):
            s_depth.copy_(depth)                                       # the static buffer, overwritten in place
            a_g = replay(t["qpos"], t["image_u8"], pointcloud=replay.static_cloud).clone()
            a_e = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": depth}).clone()
            assert torch.equal(a_g, a_e)
            return a_g
        a1, a2 = both(d1), both(d2)
        assert not torch.equal(a1, a2)
        fusion.set_extrinsics(_extrinsics(2, flavour=1))
        a3 = both(d2)
        fusion.set_seed(12)
        a4 = both(d2)
        assert not torch.equal(a3, a2) and not torch.equal(a4, a3)
        a_other = replay(t["qpos"], t["image_u8"], pointcloud={"depth": d1.unsqueeze(2)}).clone()      # copied into the static buffer
        assert torch.equal(a_other, eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": d1}))
        with pytest.raises(ValueError):
            replay(t["qpos"], t["image_u8"])
    finally:
        fusion.set_extrinsics(sc["T"])
        fusion.set_seed(11)
        eng.set_rgbd_fusion(None)


def test_infer_pipeline_feeds_depth_frames(pcd_engine):
    eng, fusion, sc, t = pcd_engine
    d, B = eng.device, sc["B"]
    with pytest.raises(ValueError, match="set_rgbd_fusion"):
        InferPipeline(eng, B, fuse_depth=True)
    eng.set_rgbd_fusion(fusion)
    try:
        pipe = InferPipeline(eng, B, fuse_depth=True, copy_stream_candidates=1)
        frames = [sc["depth"], scene(64, 96, B=B, seed=4)["depth"]]
        hq, him = t["qpos"].cpu().pin_memory(), t["image_u8"].cpu().pin_memory()
        hd = [torch.from_numpy(f).pin_memory() for f in frames]
        pipe.feed(hq, him, depth_host=hd[0])
        outs = [pipe.step(next_inputs=(hq, him, hd[1])).clone(), pipe.step().clone()]
        for a, f in zip(outs, frames):
            assert torch.equal(a, eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": torch.from_numpy(f).to(d)}))
        assert not torch.equal(outs[0], outs[1])
        with pytest.raises(ValueError):
            pipe.feed(hq, him)
    finally:
        eng.set_rgbd_fusion(None)


# ---- 6. error returns -------------------------------------------------------------------------------------------------------------
def test_error_returns_are_codes_not_faults():
    lib = L.load()
    assert lib.actmi_op_rgbd_cloud(None, None) == -1 and b"null descriptor" in lib.actmi_op_last_error()
    sc, quota = scene(37, 53), [100, 33]
    f = make_fusion(sc, quota)
    img, dep = torch.from_numpy(sc["image"]).to(DEV), torch.from_numpy(sc["depth"]).to(DEV)
    sentinel = f.fuse(img, dep, 3)["xyz"].clone()

    def desc(**over):
        d = L.RgbdDesc()
        d.depth, d.image, d.calib, d.seed = dep.data_ptr(), img.data_ptr(), f._calib.data_ptr(), f._seed.data_ptr()
        d.xyz, d.rgb, d.n, d.ws, d.ws_bytes = f.xyz.data_ptr(), f.rgb.data_ptr(), f.n.data_ptr(), f._ws.data_ptr(), f._ws.numel() * 8
        d.B, d.K, d.C, d.H, d.W, d.P = 3, 2, 2, 37, 53, sum(quota)
        for k in range(2):
            d.quota[k], d.cam_index[k] = quota[k], sc["cam_index"][k]
        for k, v in over.items():
            if k in ("quota", "cam_index"):
                for i, x in enumerate(v):
                    getattr(d, k)[i] = x
            else:
                setattr(d, k, v)
        return d

    def call(**over):
        d = desc(**over)
        return lib.actmi_op_rgbd_cloud(C.byref(d), L.current_stream_ptr()), lib.actmi_op_last_error()
    assert call()[0] == 0
    for over, word in ((dict(K=0), b"K outside"), (dict(K=9), b"K outside"), (dict(P=sum(quota) + 1), b"sum to P"),
                       (dict(quota=[100, 34]), b"sum to P"), (dict(quota=[133, 0]), b"quota"), (dict(cam_index=[2, 0]), b"cam_index"),
                       (dict(cam_index=[0, -1]), b"cam_index"), (dict(ws_bytes=64), b"workspace"), (dict(depth=0), b"null"),
                       (dict(n=0), b"null"), (dict(H=2048, W=2048), b"H * W"), (dict(B=0), b"B outside")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg, (over, rc, msg)
    assert lib.actmi_op_rgbd_cloud_workspace_bytes(3, 2, 37, 53) > 0 and lib.actmi_op_rgbd_cloud_workspace_bytes(3, 9, 37, 53) < 0
    torch.cuda.synchronize()
    assert torch.equal(f.xyz[:3], sentinel)                            # a refused call launched nothing
    # engines
    plain_cfg = tiny_config()
    plain = ACTEngine(plain_cfg, max_batch=1)
    with pytest.raises(ValueError, match="use_pcd"):
        plain.set_rgbd_fusion(f)
    cfg = tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64)
    small = ACTEngine(cfg, max_batch=1, max_points=64)
    with pytest.raises(ValueError, match="max_points"):
        ops.RGBDFusion(small, 2, 64, 96, [1, 0], scene(64, 96)["intr"], DEPTH_SCALE, scene(64, 96)["T"], scene(64, 96)["box"], [40, 25])
    with pytest.raises(ValueError, match="max_points"):
        small.set_rgbd_fusion(make_fusion(scene(64, 96), [40, 25]))
    with pytest.raises(ValueError):
        small.set_rgbd_fusion(f)                                       # frames of another size
