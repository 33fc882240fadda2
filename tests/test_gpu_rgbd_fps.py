"""Farthest-point sampling in the RGB-D fusion on the device: actmi_op_rgbd_cloud_fps / ops.RGBDFusion(sampling="fps"), every
surface that takes a fusion, and the error returns of the raw entry.

How the comparison is pinned.  Near-ties in distance would flip between float64 and fp32, so the selection is not compared with a
float64 oracle.  Instead every camera's full survivor set, with the coordinates the device computes, comes from a
sampling="key" run with quota = [H * W] * K -- that run keeps everything, and tests/test_gpu_rgbd_cloud.py pins it to the float64
transcription of the reference's node at 1e-5 m.  ops.rgbd_fps_select (the definition of actmi.h in numpy) is applied to those fp32
coordinates and to ops.rgbd_select_key, and src_idx, order, n, survivors and rgb must be EQUAL, xyz bitwise equal to the all-kept
run's rows, the padding exactly zero.  Both sides run the same fp32 operations in the same order, so every assertion is exact and
the share of inputs left out of a comparison is zero."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_fixture, regenerate  # noqa: E402
from test_gpu_rgbd_cloud import ABOVE, DEPTH_SCALE, DEV, _extrinsics, scene  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402
from actmi.engine import ACTEngine, InferPipeline  # noqa: E402


# ---- running the op, and what it must give ------------------------------------------------------------------------------------
def make(sc, quota, sampling="fps", pool=None, seed=0, T=None, target=DEV, max_batch=None, depth_scale=DEPTH_SCALE):
    kw = dict(sampling="fps", fps_pool=pool) if sampling == "fps" else {}
    return ops.RGBDFusion(target, sc["K"], sc["H"], sc["W"], sc["cam_index"], sc["intr"], depth_scale, sc["T"] if T is None else T,
                          sc["box"], quota, max_batch=max_batch or sc["depth"].shape[0], num_cams=sc["C"], seed=seed, **kw)


def run(f, sc, depth=None):
    depth = sc["depth"] if depth is None else depth
    B = depth.shape[0]
    out = f.fuse(torch.from_numpy(sc["image"]).to(DEV), torch.from_numpy(depth).to(DEV), B)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy().copy() for k, v in out.items()}
    res["src_idx"], res["survivors"] = f.src_idx[:B].cpu().numpy().copy(), f.survivors[:B].cpu().numpy().copy()
    if f.order is not None:
        res["order"] = f.order[:B].cpu().numpy().copy()
    return res


_FULL = {}


def all_kept(name, sc, depth=None, T=None, depth_scale=DEPTH_SCALE):
    """per (b, k): the survivors' pixels, device coordinates and colours, from the key-draw op with quota H * W (computed once
    per `name` and shared)"""
    if name not in _FULL:
        HW, K = sc["H"] * sc["W"], sc["K"]
        got = run(make(sc, [HW] * K, sampling="key", T=T, depth_scale=depth_scale), sc, depth)
        cams = []
        for b in range(len(got["n"])):
            idx = got["src_idx"][b, :got["n"][b]]
            assert (np.diff(idx) > 0).all() and (got["src_idx"][b, got["n"][b]:] == -1).all()
            row = []
            for k in range(K):
                m = (idx >= k * HW) & (idx < (k + 1) * HW)
                row.append(dict(pix=idx[m] - k * HW, xyz=got["xyz"][b, :got["n"][b]][m], rgb=got["rgb"][b, :got["n"][b]][m]))
                assert len(row[-1]["pix"]) == got["survivors"][b, k]
            cams.append(row)
        _FULL[name] = cams
    return _FULL[name]


def expected(full, sc, quota, pool, seed):
    """the rows the FPS op must write, from the all-kept survivors and the numpy definition"""
    H, W, K, B, P = sc["H"], sc["W"], sc["K"], len(full), int(sum(quota))
    ref = dict(xyz=np.zeros((B, P, 3), np.float32), rgb=np.zeros((B, P, 3), np.float32), n=np.zeros(B, np.int32),
               src_idx=np.full((B, P), -1, np.int32), order=np.full((B, P), -1, np.int32), survivors=np.zeros((B, K), np.int32),
               seq=[[None] * K for _ in range(B)], key=[[None] * K for _ in range(B)])
    for b in range(B):
        r = 0
        for k in range(K):
            cam = full[b][k]
            key = ops.rgbd_select_key(seed, b, k, cam["pix"], H, W)
            kept, seq = ops.rgbd_fps_select(cam["xyz"], key, quota[k], pool)
            turn = np.full(len(cam["pix"]), -1, np.int32)
            turn[seq] = np.arange(len(seq), dtype=np.int32)
            m = len(kept)
            ref["xyz"][b, r:r + m], ref["rgb"][b, r:r + m] = cam["xyz"][kept], cam["rgb"][kept]
            ref["src_idx"][b, r:r + m], ref["order"][b, r:r + m] = k * H * W + cam["pix"][kept], turn[kept]
            ref["survivors"][b, k], ref["seq"][b][k], ref["key"][b][k] = len(cam["pix"]), seq, key
            r += m
        ref["n"][b] = r
    return ref


def check(got, ref, what):
    for name in ("survivors", "n", "src_idx", "order", "rgb"):
        assert np.array_equal(got[name], ref[name]), (what, name)
    assert got["xyz"].tobytes() == ref["xyz"].tobytes(), (what, "xyz bits")
    for b, n in enumerate(ref["n"]):
        assert not got["xyz"][b, n:].any() and not got["rgb"][b, n:].any(), what
        assert (got["src_idx"][b, n:] == -1).all() and (got["order"][b, n:] == -1).all(), what
        assert (np.diff(got["src_idx"][b, :n]) > 0).all(), what


def fps_case(name, sc, quota, pool, seed, depth=None, T=None, depth_scale=DEPTH_SCALE):
    full = all_kept(name, sc, depth, T, depth_scale)
    f = make(sc, quota, pool=pool, seed=seed, T=T, depth_scale=depth_scale)
    ref = expected(full, sc, quota, f.fps_pool, seed)
    got = run(f, sc, depth)
    print(f"{name}: quota {quota}, pool {f.fps_pool}, survivors {ref['survivors'].tolist()}, n {ref['n'].tolist()}")
    check(got, ref, name)
    return got, ref, f


# ---- 1. the pool is every survivor --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,pool", [(37, 53, 2048), (64, 96, 6144)])      # ragged last tile, odd width; six tiles
def test_fps_over_all_survivors_matches_the_definition(H, W, pool):
    sc, quota = scene(H, W), ABOVE[(H, W)]
    got, ref, _ = fps_case(f"{H}x{W}", sc, quota, pool, seed=12345)
    assert (ref["survivors"] > np.asarray(quota)).all() and (ref["survivors"] <= pool).all()
    assert (got["n"] == sum(quota)).all()
    for b in range(sc["B"]):
        assert sorted(got["order"][b, :quota[0]].tolist()) == list(range(quota[0]))       # every turn once per camera
        assert sorted(got["order"][b, quota[0]:].tolist()) == list(range(quota[1]))


# ---- 2. the pool is preselected by key ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,pool,quota", [(64, 96, 256, [100, 33]), (120, 160, 512, [200, 129])])
def test_pool_preselection_by_key_then_fps(H, W, pool, quota):
    sc = scene(H, W)
    got, ref, _ = fps_case(f"{H}x{W}", sc, quota, pool, seed=777)
    assert (ref["survivors"] > pool).all() and ref["survivors"].min() > (300 if H == 64 else 1000)
    full = all_kept(f"{H}x{W}", sc)
    for b in range(sc["B"]):
        idx = got["src_idx"][b]
        for k in range(sc["K"]):
            mine = idx[(idx >= k * H * W) & (idx < (k + 1) * H * W)] - k * H * W
            members = full[b][k]["pix"][np.argsort(ref["key"][b][k], kind="stable")[:pool]]
            assert len(mine) == quota[k] and np.isin(mine, members).all()                 # kept rows come from the pool only
            start = idx[(got["order"][b] == 0) & (idx >= k * H * W) & (idx < (k + 1) * H * W)] - k * H * W
            assert start.tolist() == [members[0]]                                         # and the start is its smallest key


# ---- 3. one camera below its quota, the other above ---------------------------------------------------------------------------------
def test_camera_below_quota_next_to_camera_above():
    H, W = 64, 96
    sc, quota = scene(H, W), [2048, 257]
    got, ref, f = fps_case("64x96", sc, quota, None, seed=5)
    assert f.fps_pool == 8192
    assert (ref["survivors"][:, 0] < quota[0]).all() and (ref["survivors"][:, 1] > quota[1]).all()
    for b in range(sc["B"]):
        m0 = int(ref["survivors"][b, 0])
        assert got["n"][b] == m0 + quota[1]
        assert got["order"][b, :m0].tolist() == list(range(m0))                           # all kept: the rank in pixel order
        assert got["src_idx"][b, m0 - 1] < H * W <= got["src_idx"][b, m0]                 # camera 1 starts right behind
        assert sorted(got["order"][b, m0:m0 + quota[1]].tolist()) == list(range(quota[1]))


# ---- 4. edge counts ----------------------------------------------------------------------------------------------------------------
def test_quota_equal_to_pool_quota_one_and_empty_inputs():
    sc = scene(64, 96)
    got, ref, _ = fps_case("64x96", sc, [128, 33], 128, seed=3)                           # camera 0: FPS degenerates to its pool
    assert (ref["survivors"] > 128).all()
    full = all_kept("64x96", sc)
    for b in range(sc["B"]):
        members = np.sort(full[b][0]["pix"][np.argsort(ref["key"][b][0], kind="stable")[:128]])
        assert np.array_equal(got["src_idx"][b, :128], members)
        assert sorted(got["order"][b, :128].tolist()) == list(range(128)) and got["order"][b, :128].tolist() != list(range(128))
    one, ref1, f1 = fps_case("64x96", sc, [1, 1], None, seed=3)                           # only the start
    assert f1.fps_pool == 4 and one["n"].tolist() == [2] * sc["B"] and (one["order"][:, :2] == 0).all()
    sc = scene(37, 53)
    depth = sc["depth"].copy()
    depth[1, 0] = 0                                                                       # sample 1: camera 0 sees nothing
    depth[2] = 0                                                                          # sample 2: no depth at all
    got, ref, _ = fps_case("37x53 holes", sc, [100, 33], None, seed=3, depth=depth)
    assert ref["survivors"][1, 0] == 0 and got["src_idx"][1, 0] >= 37 * 53 and got["n"].tolist() == [133, 33, 0]
    assert not got["xyz"][2].any() and not got["rgb"][2].any() and (got["order"][2] == -1).all()


# ---- 5. coincident points ------------------------------------------------------------------------------------------------------------
def test_coincident_points_never_give_a_duplicate():
    sc = scene(37, 53)
    box = sc["box"]
    T = np.zeros((2, 3, 4))
    T[:, :, 3] = [(box[0] + box[1]) / 2, (box[2] + box[3]) / 2, (box[4] + box[5]) / 2]    # every pixel with a depth lands here
    quota = [100, 33]
    got, ref, f = fps_case("37x53 one point", sc, quota, None, seed=21, T=T)
    assert f.fps_pool == 400 and (ref["survivors"] > 400).all()
    assert (ref["survivors"] == (sc["depth"] != 0).sum((2, 3))).all()
    for b in range(sc["B"]):
        assert len(np.unique(got["xyz"][b, :133], axis=0)) == 1
        assert len(set(got["src_idx"][b, :133].tolist())) == 133                          # no duplicate
        r = 0
        for k in range(2):
            o = got["order"][b, r:r + quota[k]]
            start = int(np.nonzero(o == 0)[0][0])
            # pool members below the quota-th in pixel order, the start among or behind them: picked in index order around it
            rest = [i for i in range(quota[k]) if i != start]
            assert o[rest].tolist() == list(range(1, quota[k])), (b, k)
            r += quota[k]


# ---- 6. ties -------------------------------------------------------------------------------------------------------------------------
def lattice_scene():
    """constant depth, identity rotation, power-of-two calibration: x = (u - 8) / 64, y = (v - 20) / 64, z = 1 without rounding"""
    H, W, B, K = 37, 53, 2, 2
    g = np.random.default_rng(9)
    T = np.tile(np.eye(4)[:3], (K, 1, 1))
    T[1, :, 3] = [0.5, -0.25, 0.125]
    return dict(depth=np.full((B, K, H, W), 1024, np.uint16), image=g.integers(0, 256, size=(B, 2, H, W, 3), dtype=np.uint8),
                intr=np.array([[64.0, 64.0, 8.0, 20.0]] * K), T=T, box=(-4.0, 4.0, -4.0, 4.0, 0.5, 2.0), cam_index=[1, 0], H=H, W=W,
                B=B, K=K, C=2)


def test_ties_on_a_lattice_go_to_the_lowest_index():
    sc, quota = lattice_scene(), [100, 33]
    got, ref, _ = fps_case("lattice", sc, quota, 2048, seed=4, depth_scale=2.0 ** -10)
    assert (ref["survivors"] == 37 * 53).all()
    full = all_kept("lattice", sc)
    ties = 0
    for b in range(sc["B"]):                                               # the picks at which several points were equally far
        p, seq = full[b][0]["xyz"].astype(np.float64), ref["seq"][b][0]
        d = np.full(len(p), np.inf)
        for s, nxt in zip(seq[:-1], seq[1:]):
            d = np.minimum(d, ((p - p[s]) ** 2).sum(1))
            d[s] = -1
            ties += int((d == d.max()).sum() > 1)
            assert nxt == int(np.argmax(d))                                # exact arithmetic on this lattice: the lowest index
    print(f"lattice: {ties} of {sc['B'] * (quota[0] - 1)} picks of camera 0 were ties")
    assert ties >= 10


# ---- 7. repeatability and seeding ----------------------------------------------------------------------------------------------------
def test_same_seed_is_bitwise_repeatable_and_another_seed_another_start():
    sc, quota = scene(64, 96), ABOVE[(64, 96)]
    f = make(sc, quota, pool=1024, seed=7)
    a, b = run(f, sc), run(f, sc)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    f.set_seed(8)
    c = run(f, sc)
    check(c, expected(all_kept("64x96", sc), sc, quota, 1024, 8), "seed 8")
    starts = lambda r: [r["src_idx"][i][r["order"][i] == 0].tolist() for i in range(sc["B"])]
    assert all(len(s) == 2 for s in starts(a)) and starts(a) != starts(c)


# ---- 8. coverage: a guaranteed bound ---------------------------------------------------------------------------------------------------
def test_fps_covers_within_twice_the_key_draws_radius():
    """The coverage radius of a subset: the largest distance from a pool point to its nearest kept point.  Greedy farthest-point
    sampling is a 2-approximation of the k-centre optimum, and no subset of the same size beats the optimum, so FPS's radius is
    at most twice the radius of the key draw's subset -- a guarantee, not a measurement (the measured ratio is printed)."""
    H, W = 64, 96
    sc, quota = scene(H, W), ABOVE[(H, W)]
    full = all_kept("64x96", sc)
    fps = run(make(sc, quota, pool=6144, seed=31), sc)
    keyd = run(make(sc, quota, sampling="key", seed=31), sc)

    def radius(pts, idx, pix):
        kept = pts[np.isin(pix, idx)].astype(np.float64)
        assert len(kept) == len(idx)
        d = ((pts.astype(np.float64)[:, None, :] - kept[None]) ** 2).sum(2).min(1)
        return float(np.sqrt(d.max()))
    worst = 0.0
    for b in range(sc["B"]):
        for k in range(sc["K"]):
            cam = full[b][k]
            sel = lambda r: r["src_idx"][b][(r["src_idx"][b] >= k * H * W) & (r["src_idx"][b] < (k + 1) * H * W)] - k * H * W
            rf, rk = radius(cam["xyz"], sel(fps), cam["pix"]), radius(cam["xyz"], sel(keyd), cam["pix"])
            print(f"sample {b} camera {k}: coverage radius fps {rf:.4f} m, key draw {rk:.4f} m, ratio {rf / rk:.3f}")
            worst = max(worst, rf / rk)
            assert rf <= 2.0 * rk
    print(f"largest fps / key-draw radius ratio: {worst:.3f}")


# ---- 9. policy, training, graph, pipeline ----------------------------------------------------------------------------------------------
POL_QUOTA, POL_POOL = [40, 24], 160


@pytest.fixture(scope="module")
def fps_engine():
    z, cfg = load_fixture("tiny_pcd")
    sd_np, inp = regenerate(z, cfg)
    B = int(z["batch"])
    assert (cfg.image_h, cfg.image_w, cfg.num_cams) == (64, 96, 2)
    sc = dict(scene(64, 96, B=B, seed=3), image=inp["image_u8"])       # the cloud's colours come from the forward's own frames
    eng = ACTEngine(cfg, max_batch=B, training=True, max_points=sum(POL_QUOTA))
    eng.load_state_dict(sd_np)
    eng.finalize()
    fusion = ops.RGBDFusion(eng, sc["K"], 64, 96, sc["cam_index"], sc["intr"], DEPTH_SCALE, sc["T"], sc["box"], POL_QUOTA, seed=11,
                            sampling="fps")
    assert fusion.fps_pool == POL_POOL
    d = eng.device
    t = {k: torch.from_numpy(inp[k]).to(d) for k in ("qpos", "image_u8", "actions", "is_pad")}
    t["eps"] = torch.from_numpy(z["train.eps"]).to(d)
    return eng, fusion, sc, t


def _oracle_cloud(name, sc, dev, seed, depth=None, T=None):
    ref = expected(all_kept(name, sc, depth, T), sc, POL_QUOTA, POL_POOL, seed)
    return {k: torch.from_numpy(ref[k]).to(dev) for k in ("xyz", "rgb", "n")}


def test_policy_and_training_take_an_fps_fusion(fps_engine):
    eng, fusion, sc, t = fps_engine
    d = eng.device
    depth = torch.from_numpy(sc["depth"]).to(d)
    cloud = _oracle_cloud("engine frames", sc, d, 11)
    assert (cloud["n"] == sum(POL_QUOTA)).all()
    eng.set_rgbd_fusion(fusion)
    try:
        a_depth = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": depth}).clone()
        a_ref = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud=cloud).clone()
        assert torch.equal(a_depth, a_ref) and float(a_ref.abs().max()) > 0                  # the cloud bits are equal
        fusion_key = ops.RGBDFusion(eng, sc["K"], 64, 96, sc["cam_index"], sc["intr"], DEPTH_SCALE, sc["T"], sc["box"], POL_QUOTA,
                                    seed=11)
        eng.set_rgbd_fusion(fusion_key)
        a_key = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": depth}).clone()
        assert not torch.equal(a_key, a_depth)                                               # another subset, another action
        eng.set_rgbd_fusion(fusion)
        # one training step
        out = eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], eps=t["eps"], pointcloud={"depth": depth})
        l_depth = torch.stack([out["l1"], out["kl"], out["loss"]]).clone()
        eng.zero_grad()
        eng.backward(1.0)
        assert torch.isfinite(eng.grad_arena()).all() and torch.isfinite(l_depth).all()
        out = eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], eps=t["eps"], pointcloud=cloud)
        assert torch.equal(l_depth, torch.stack([out["l1"], out["kl"], out["loss"]]))
        # the policy surface
        from policy import ACTPolicy
        pol = ACTPolicy({"use_pcd": True, "pcd_hidden_dim": 64, "pcd_output_dim": 64, "max_points": sum(POL_QUOTA), "kl_weight": 10,
                         "lr": 1e-5, "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2,
                         "nheads": 4, "camera_names": ["a", "b"], "image_h": 64, "image_w": 96, "base_width": 8, "training": False},
                        max_batch=sc["B"])
        pol.set_rgbd_fusion(ops.RGBDFusion(pol.model, sc["K"], 64, 96, sc["cam_index"], sc["intr"], DEPTH_SCALE, sc["T"], sc["box"],
                                           POL_QUOTA, seed=11, sampling="fps"))
        p_depth = pol(t["qpos"], t["image_u8"], pointcloud={"depth": depth}).clone()
        p_ref = pol(t["qpos"], t["image_u8"], pointcloud=cloud)
        assert torch.equal(p_depth, p_ref)
    finally:
        eng.set_rgbd_fusion(None)


def test_captured_graph_replays_an_fps_fusion_with_new_frames_and_seed(fps_engine):
    eng, fusion, sc, t = fps_engine
    d, B = eng.device, sc["B"]
    eng.set_rgbd_fusion(fusion)
    try:
        replay = eng.capture_infer(B, fuse_depth=True)
        s_depth = replay.static_cloud["depth"]
        d1 = torch.from_numpy(sc["depth"]).to(d)
        d2 = torch.from_numpy(scene(64, 96, B=B, seed=4)["depth"]).to(d)

        def both(depth):
            s_depth.copy_(depth)
            a_g = replay(t["qpos"], t["image_u8"], pointcloud=replay.static_cloud).clone()
            a_e = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud={"depth": depth}).clone()
            assert torch.equal(a_g, a_e)
            return a_g
        a1, a2 = both(d1), both(d2)
        fusion.set_seed(12)
        a3 = both(d2)
        fusion.set_extrinsics(_extrinsics(2, flavour=1))
        a4 = both(d2)
        assert not torch.equal(a1, a2) and not torch.equal(a3, a2) and not torch.equal(a4, a3)
        fusion.set_extrinsics(sc["T"])
        sc2 = dict(sc, depth=d2.cpu().numpy())
        a_ref = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud=_oracle_cloud("engine frames 2", sc2, d, 12))
        assert torch.equal(both(d2), a_ref)                                                  # the replay follows the definition too
    finally:
        fusion.set_extrinsics(sc["T"])
        fusion.set_seed(11)
        eng.set_rgbd_fusion(None)


def test_infer_pipeline_feeds_depth_frames_to_an_fps_fusion(fps_engine):
    eng, fusion, sc, t = fps_engine
    d, B = eng.device, sc["B"]
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
    finally:
        eng.set_rgbd_fusion(None)


# ---- 10. error returns ---------------------------------------------------------------------------------------------------------------
def test_error_returns_are_codes_not_faults():
    lib = L.load()
    assert lib.actmi_op_rgbd_cloud_fps(None, None) == -1 and b"null descriptor" in lib.actmi_op_last_error()
    sc, quota, pool = scene(37, 53), [100, 33], 400
    f = make(sc, quota, pool=pool)
    img, dep = torch.from_numpy(sc["image"]).to(DEV), torch.from_numpy(sc["depth"]).to(DEV)
    sentinel = {k: v.clone() for k, v in f.fuse(img, dep, 3).items()}
    order = f.order.clone()

    def call(**over):
        d = L.RgbdFpsDesc()
        a = d.base
        a.depth, a.image, a.calib, a.seed = dep.data_ptr(), img.data_ptr(), f._calib.data_ptr(), f._seed.data_ptr()
        a.xyz, a.rgb, a.n, a.ws, a.ws_bytes = f.xyz.data_ptr(), f.rgb.data_ptr(), f.n.data_ptr(), f._ws.data_ptr(), f._ws.numel() * 8
        a.src_idx, a.survivors = f.src_idx.data_ptr(), f.survivors.data_ptr()
        a.B, a.K, a.C, a.H, a.W, a.P = 3, 2, 2, 37, 53, sum(quota)
        for k in range(2):
            a.quota[k], a.cam_index[k] = quota[k], sc["cam_index"][k]
        d.pool, d.order = pool, f.order.data_ptr()
        for k, v in over.items():
            if k in ("quota", "cam_index"):
                for i, x in enumerate(v):
                    getattr(a, k)[i] = x
            elif k in ("pool", "order"):
                setattr(d, k, v)
            else:
                setattr(a, k, v)
        return lib.actmi_op_rgbd_cloud_fps(C.byref(d), L.current_stream_ptr()), lib.actmi_op_last_error()
    assert call()[0] == 0
    assert call(order=0)[0] == 0                                                             # the order output is optional
    need = lib.actmi_op_rgbd_cloud_fps_workspace_bytes(3, 2, 37, 53, pool)
    assert 0 < need <= f._ws.numel() * 8
    for over, word in ((dict(pool=0), b"pool outside"), (dict(pool=L.RGBD_FPS_MAX_POOL + 1), b"pool outside"),
                       (dict(pool=99), b"quota[k] > pool"), (dict(quota=[32, 101], pool=100), b"quota[k] > pool"),
                       (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=64), b"workspace"), (dict(depth=0), b"null"),
                       (dict(n=0), b"null"), (dict(ws=f._ws.data_ptr() + 4), b"misaligned"), (dict(order=f.order.data_ptr() + 2), b"misaligned"),
                       (dict(K=9), b"K outside"), (dict(quota=[100, 34]), b"sum to P"), (dict(cam_index=[2, 0]), b"cam_index")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg, (over, rc, msg)
    torch.cuda.synchronize()
    for k, v in sentinel.items():                                                            # a refused call launched nothing
        assert torch.equal(f.outputs(3)[k], v), k
    assert torch.equal(f.order, order)
    with pytest.raises(ValueError, match="fps_pool"):
        make(sc, quota, pool=99)
