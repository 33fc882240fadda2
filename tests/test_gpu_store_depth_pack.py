"""DeviceEpisodeStore(..., store_compressed=True, store_encode=True, depth_pack=True) on the GPU: the raw uint16 depth of raw episodes
is packed on the device as the store reads it and every batch's depth is unpacked by one launch.  The depth tensors are torch.equal
to those of the decoded store and of the host loader on the same files; the camera tensors to those of the route that exists for
cameras -- ``compress_dataset_dir`` on the files without their depth entries and a compressed store of its output.  Train and
validation loaders, mirrored twins, ``replay_batch``, launches that loop, training steps, a corrupted arena, the arena's size."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from actmi import episode_store as E  # noqa: E402
from actmi import ops  # noqa: E402
from actmi.episode_compress import compress_dataset_dir  # noqa: E402
from test_gpu_store_encode import smooth_frames  # noqa: E402

DEV = "cuda:0"
CAMS = ("left_wrist", "right_wrist")
LENGTHS = (6, 4, 3)
SIZES = [(8, 12), (17, 23), (33, 40), (12, 67)]                     # the store tests' sizes, and a width of more than 64 that is no multiple of 8
PACK = dict(store_encode=True, depth_pack=True)
DEPTH = dict(depth_camera_names=list(CAMS), use_depth=True)


def depth_frames(rng, T, H, W, noisy):
    """planes with steps, sensor noise, a blob of holes and salt holes (noisy: full-range values with holes)"""
    if noisy:
        d = rng.integers(0, 65536, (T, H, W)).astype(np.uint16)
        d[rng.random((T, H, W)) < 0.2] = 0
        return d
    yy, xx = np.mgrid[:H, :W]
    out = np.empty((T, H, W), dtype=np.uint16)
    for t in range(T):
        z = 900.0 + 40 * t + 3.0 * xx + 2.0 * yy + 300.0 * (xx // 9) + rng.normal(0.0, 2.0, (H, W))
        z = np.clip(np.rint(z), 1, 65535).astype(np.uint16)
        z[H // 3:H // 3 + 2, W // 4:W // 4 + 5] = 0
        z[rng.random((H, W)) < 0.04] = 0
        out[t] = z
    return out


def write_dataset(dirpath, hw, seed=0, cams=CAMS, lengths=LENGTHS, action_dim=14):
    """raw episodes with a depth camera per camera, and beside them the same episodes without their depth entries"""
    rng = np.random.default_rng(seed)
    raw, bare = os.path.join(str(dirpath), "raw"), os.path.join(str(dirpath), "bare")
    os.makedirs(raw), os.makedirs(bare)
    H, W = hw
    for i, T in enumerate(lengths):
        ep = {"/observations/qpos": (rng.standard_normal((T, 14)) * 2 + 1).astype(np.float32),
              "/observations/qvel": rng.standard_normal((T, 14)).astype(np.float32),
              "/action": (rng.standard_normal((T, action_dim)) * 3 - 0.5).astype(np.float32), "attrs_sim": np.array(i != 1)}
        for c in cams:
            ep[f"/observations/images/{c}"] = smooth_frames(rng, T, H, W)
        np.savez(os.path.join(bare, f"episode_{i}.npz"), **ep)
        for k, c in enumerate(cams):
            ep[f"/observations/depth_images/{c}"] = depth_frames(rng, T, H, W, noisy=(i + k) % 2 == 1)
        np.savez(os.path.join(raw, f"episode_{i}.npz"), **ep)
    return raw, bare


def dirs(tmp_path, hw, **kw):
    raw, bare = write_dataset(tmp_path, hw, **kw)
    written = compress_dataset_dir(bare, device=DEV)
    assert len(written) == len(kw.get("lengths", LENGTHS))
    return raw, bare + "_compressed"


def files(d):
    return sorted(os.path.join(d, f) for f in os.listdir(d))


def loaders(dirpath, route, cams=CAMS, **kw):
    """route: 'pack' the new store, 'decoded' the parent's store for such a dataset, 'host' the host loader (all three with depth),
    'cams' the compressed store of the compressed camera files"""
    args = (dirpath, lambda n: True, list(cams), 4, 3, 5)
    common = dict(policy_class="ACT", num_workers=0, train_ratio=0.67, rng=np.random.default_rng(3), **kw)
    depth = dict(depth_camera_names=list(cams), use_depth=True)
    if route == "host":
        return D.load_data(*args, **common, **depth)
    if route == "decoded":
        return D.load_data(*args, **common, **depth, device_dataset=True, device=DEV)
    packed = dict(device_dataset=True, device=DEV, device_decode=True, store_compressed=True)
    if route == "cams":
        return D.load_data(*args, **common, **packed)
    return D.load_data(*args, **common, **depth, **packed, **PACK)


def same(d, h):
    assert d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape)
    return torch.equal(d.cpu().view(torch.uint8), torch.as_tensor(h).cpu().view(torch.uint8))


def assert_same_batches(pack, depth_routes, cam_routes, draws=(0, 0, 1, 0, 0, 1, 0, 0)):
    its = [[iter(r[0]), iter(r[1])] for r in [pack] + list(depth_routes) + list(cam_routes)]
    for which in draws:                                               # train and validation loaders
        got, *others = [next(it[which]) for it in its]
        assert len(got) == 5 and got[4].is_cuda and got[4].dtype == torch.uint16
        for other in others[:len(depth_routes)]:
            assert len(other) == 5
            for i in (1, 2, 3, 4):                                    # qpos, action, is_pad and the depth frames
                assert same(got[i], other[i]), (which, i)
        for other in others[len(depth_routes):]:
            assert len(other) == 4
            for i in (0, 1, 2, 3):                                    # the camera frames
                assert same(got[i], other[i]), (which, i)


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_batches_equal_the_decoded_store_the_host_loader_and_the_camera_route(tmp_path, hw):
    raw, cams_dir = dirs(tmp_path, hw)
    pack, decoded = loaders(raw, "pack"), loaders(raw, "decoded")
    store, ref = pack[0].store, decoded[0].store
    n = sum(LENGTHS) * len(CAMS)
    assert store.depth_pack and store.encode_stats == {"device": n} and store._held_depth == {} and store._held_bytes == 0
    st = store.depth_pack_stats
    assert st["frames"] == n and st["raw_bytes"] == n * 2 * hw[0] * hw[1]
    dep = store.layout.all_kinds[1]
    assert dep.marks_per_frame == 0 and int(dep.stream_cap.sum()) == st["stream_bytes"]
    assert store.stream_bytes_used == sum(int(k.stream_cap.sum()) for k in store.layout.kinds)
    want = 0                                                          # the streams are depth_pack_ref's of the files' frames
    for path in files(raw):
        with np.load(path) as z:
            want += sum(len(ops.depth_pack_ref(f)) for c in CAMS for f in z[f"/observations/depth_images/{c}"])
    assert st["stream_bytes"] == want
    assert_same_batches(pack, [decoded, loaders(raw, "host")], [loaders(cams_dir, "cams")])
    store.check_decoded()
    assert store.device_bytes() >= store.nbytes + 8 and ref.depth_pack is False


def test_the_arena_is_smaller_than_the_decoded_stores(tmp_path):
    raw, _cams = dirs(tmp_path, (64, 96), lengths=(6, 4, 5))
    stats, _ = D.get_norm_stats(files(raw))
    args = (files(raw), range(3), list(CAMS), stats, DEV)
    common = dict(device_decode=True, store_compressed=True, decode_frames=2, **DEPTH, **PACK)   # two frames a launch: small workspaces
    plain = D.DeviceEpisodeStore(*args, **DEPTH)
    packed = D.DeviceEpisodeStore(*args, **common)
    assert packed.nbytes < plain.nbytes and packed.device_bytes() < plain.device_bytes()
    dep = packed.layout.all_kinds[1]
    assert int(dep.stream_cap.sum()) < 15 * len(CAMS) * dep.frame_bytes                # the depth blocks themselves shrink
    with pytest.raises(MemoryError, match="bytes on the device"):      # the held streams and the stage count against the budget
        D.DeviceEpisodeStore(*args, budget_bytes=packed.nbytes, **common)


def test_mirror_twins_and_replay_batches(tmp_path):
    raw, cams_dir = dirs(tmp_path, (17, 23))
    spec = D.MirrorSpec(swap=(CAMS,), flip=CAMS)
    kw = dict(mirror_twins=True, mirror_spec=spec)
    pack = loaders(raw, "pack", **kw)
    store = pack[0].store
    assert store.has_twins and store.depth_pack_stats["frames"] == sum(LENGTHS) * len(CAMS)      # a twin adds no frame and no pack
    assert store.layout.all_kinds[1].flip.any() and 1 not in store._scratch                       # flips ride in the records
    assert_same_batches(pack, [loaders(raw, "decoded", **kw), loaders(raw, "host", **kw)], [loaders(cams_dir, "cams", **kw)])
    # replay: what EpisodeReplay yields for the raw file (and its twin), bit for bit, for qpos and depth
    paths = D.mirror_twin_paths(files(raw), spec, dict(zip(CAMS, CAMS)))
    assert len(paths) == len(store.paths)
    for eid in store.episode_ids:
        host = D.EpisodeReplay(paths[eid], list(CAMS), store.norm_stats, 4, **DEPTH)
        dev = D.DeviceEpisodeReplay(store, eid, 4)
        assert len(host) == len(dev)
        for hb, db in zip(host, dev):
            assert len(hb) == len(db) == 3
            assert same(db[1], hb[1]) and same(db[2], hb[2])
    store.check_decoded()


def test_launches_that_loop_give_the_same_batches(tmp_path):
    raw, _cams = dirs(tmp_path, (17, 23))
    stats, _ = D.get_norm_stats(files(raw))
    args = (files(raw), range(3), list(CAMS), stats, DEV)
    common = dict(device_decode=True, store_compressed=True, **DEPTH, **PACK)
    small = D.DeviceEpisodeStore(*args, decode_frames=2, stage_bytes=1500, **common)     # pieces of two frames, one frame a staging copy
    ref = D.DeviceEpisodeStore(*args, **common)
    plain = D.DeviceEpisodeStore(*args, **DEPTH)
    assert small.depth_pack_stats == ref.depth_pack_stats and torch.equal(small.arena, ref.arena)
    e, t = np.asarray([0, 1, 2, 0, 1]), np.asarray([5, 0, 2, 1, 3])
    a, b, c = ref.gather(e, t, 4), small.gather(e, t, 4), plain.gather(e, t, 4)
    assert all(same(y, x) for x, y in zip(a, b)) and same(a[4], c[4])
    small.check_decoded()


def test_a_corrupted_header_byte_is_flagged_and_survived(tmp_path):
    """a data error in the arena: the unpack flags the row, writes it as zeros, stays inside its bounds, and check_decoded raises"""
    raw, _cams = dirs(tmp_path, (17, 23))
    stats, _ = D.get_norm_stats(files(raw))
    common = dict(device_decode=True, store_compressed=True, **DEPTH, **PACK)
    store = D.DeviceEpisodeStore(files(raw), range(3), list(CAMS), stats, DEV, **common)
    e, t = np.asarray([0, 1]), np.asarray([2, 1])
    good = store.gather(e, t, 4)[4].cpu().numpy()
    store.check_decoded()
    q, H = 1, 17
    row = int(store._frame_row(q, 0, 0)) + 2                          # episode 0, depth camera 0, step 2: item 0 of the batch
    rec = store._ptab[q]["rec"][row]
    first_row = int(rec["seg_off"]) + 4 * (H + 1)                     # the header byte of group 0 of row 0
    store.arena[first_row] = 17
    bad = store.gather(e, t, 4)[4].cpu().numpy()
    assert good[0, 0, 0, 0].any() and not bad[0, 0, 0, 0].any() and np.array_equal(bad[0, 0, 0, 1:], good[0, 0, 0, 1:])
    assert np.array_equal(bad[0, 1], good[0, 1]) and np.array_equal(bad[1], good[1])
    with pytest.raises(RuntimeError, match="packed depth.*status 2.*invalid group header"):
        store.check_decoded()
    assert E.DEPTH_PACK_MODE not in ops.JPEG_MODES.values()


def test_training_steps_give_the_same_loss_bits(tmp_path):
    import imitate_episodes as ie
    from policy import ACTPolicy
    cams = ["a", "b"]
    raw, cams_dir = dirs(tmp_path, (64, 96), cams=cams, lengths=(12, 9, 8), action_dim=16)
    load = lambda d, **kw: D.load_data(d, lambda n: True, cams, 2, 2, 8, policy_class="ACT", num_workers=0,  # noqa: E731
                                       rng=np.random.default_rng(7), device_dataset=True, device=DEV, **kw)[0]
    depth = dict(depth_camera_names=cams, use_depth=True)
    packed = dict(device_decode=True, store_compressed=True)
    pack_dl = load(raw, **depth, **packed, **PACK)
    cam_dl, dec_dl = load(cams_dir, **packed), load(raw, **depth)

    def parent_batches():                                             # the parent's stores: cameras compressed, depth decoded
        for c, d in zip(cam_dl, dec_dl):
            yield tuple(c) + (d[4],)
    losses = []
    for feed in (iter(pack_dl), parent_batches()):
        pol = ACTPolicy({"use_depth": True, "depth_camera_names": cams, "kl_weight": 10, "lr": 1e-5, "num_queries": 8, "hidden_dim": 64,
                         "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2, "nheads": 4, "camera_names": cams, "image_h": 64,
                         "image_w": 96, "base_width": 8}, max_batch=2)
        pol.train()
        opt = ie.make_optimizer("ACT", pol)
        steps = []
        for step in range(2):
            opt.zero_grad()
            pol.next_eps = torch.randn(2, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(20 + step)).to(DEV)
            out = ie.forward_pass(next(feed), pol, None)
            out["loss"].backward()
            opt.step()
            steps.append({k: float(v) for k, v in out.items()})
        pol.model.check_flags()
        losses.append(steps)
    pack_dl.store.check_decoded()
    print(f"depth_pack store {losses[0]}, the parent's stores {losses[1]}")
    assert all(np.isfinite(v) for s in losses[0] for v in s.values())
    assert losses[0] == losses[1] and losses[0][0] != losses[0][1]
