"""Host side of the farthest-point sampling of the RGB-D fusion (actmi.ops.rgbd_fps_select, RGBDFusion(sampling="fps")): the
numpy statement of the definition against a brute-force float32 loop, the exclusion, tie and pool rules, everything RGBDFusion
refuses about the new arguments on the host, and the C boundary of the new entry points -- no GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from actmi import lib as L
from actmi import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "include")
f32 = np.float32


def brute_force(xyz, key, quota, pool):
    """the definition, point by point in Python: float32 scalars, one rounding per operation, first maximum wins"""
    M = len(xyz)
    if M <= quota:
        return list(range(M)), list(range(M))
    order = sorted(range(M), key=lambda i: int(key[i]))
    members = sorted(order[:pool]) if M > pool else list(range(M))
    dist = [f32(np.inf)] * len(members)
    s = min(range(len(members)), key=lambda j: int(key[members[j]]))
    seq = []
    for it in range(quota):
        seq.append(members[s])
        dist[s] = f32(-1.0)
        if it + 1 == quota:
            break
        ps = xyz[members[s]]
        best, nxt = f32(-2.0), -1
        for j, i in enumerate(members):
            if j != s and dist[j] >= 0:
                dx, dy, dz = f32(xyz[i][0] - ps[0]), f32(xyz[i][1] - ps[1]), f32(xyz[i][2] - ps[2])
                d = f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))
                dist[j] = min(dist[j], d)
            if dist[j] > best:                                          # strictly: the lowest index among equals
                best, nxt = dist[j], j
        s = nxt
    return sorted(seq), seq


@pytest.mark.parametrize("M,quota,pool,seed", [(40, 7, 40, 0), (64, 64, 64, 1), (97, 13, 32, 2), (97, 32, 32, 3), (30, 1, 8, 4),
                                               (12, 20, 24, 5), (150, 40, 151, 6)])
def test_select_matches_a_brute_force_float32_loop(M, quota, pool, seed):
    g = np.random.default_rng(seed)
    xyz = g.uniform(-1.5, 1.5, size=(M, 3)).astype(f32)
    key = g.permutation(4096)[:M].astype(np.uint32)
    kept, seq = ops.rgbd_fps_select(xyz, key, quota, pool)
    bk, bs = brute_force(xyz, key, quota, pool)
    assert kept.tolist() == bk and seq.tolist() == bs
    assert len(seq) == min(M, quota) and len(set(seq.tolist())) == len(seq) and (np.diff(kept) > 0).all()
    if M > quota:
        members = np.arange(M) if M <= pool else np.argsort(key, kind="stable")[:pool]
        assert seq[0] == members[np.argmin(key[members])]               # the start: the pool's smallest key
        assert np.isin(seq, members).all()


def test_duplicated_points_are_never_picked_twice():
    """five distinct places, each held by eight coincident points: the first five picks visit the five places, after that every
    remaining distance is 0 and the picks go to the lowest unpicked indices"""
    g = np.random.default_rng(7)
    places = g.uniform(-1, 1, size=(5, 3)).astype(f32)
    xyz = np.repeat(places, 8, axis=0)[g.permutation(40)]
    key = g.permutation(64)[:40].astype(np.uint32)
    kept, seq = ops.rgbd_fps_select(xyz, key, 12, 40)
    assert len(set(seq.tolist())) == 12
    assert len({xyz[i].tobytes() for i in seq[:5]}) == 5
    rest = sorted(set(range(40)) - set(seq[:5].tolist()))
    assert seq[5:].tolist() == rest[:7]
    assert (kept.tolist(), seq.tolist()) == brute_force(xyz, key, 12, 40)
    # every point the same: the start, then 0, 1, 2, .. without it
    same = np.tile(places[:1], (9, 1))
    kept, seq = ops.rgbd_fps_select(same, np.array([5, 3, 8, 1, 9, 2, 7, 6, 4], np.uint32), 4, 9)
    assert seq.tolist() == [3, 0, 1, 2]


def test_ties_on_a_lattice_go_to_the_lowest_index():
    """a 5 x 5 lattice with spacing 1/4 (every distance exact in float32), started at its centre: the four corners are equally far,
    and the lowest index wins; the sequence is the brute-force loop's"""
    v, u = np.divmod(np.arange(25), 5)
    xyz = np.stack([u * 0.25, v * 0.25, np.ones(25)], 1).astype(f32)
    key = np.arange(25, dtype=np.uint32) + 1
    key[12] = 0                                                         # the centre starts
    kept, seq = ops.rgbd_fps_select(xyz, key, 9, 25)
    assert seq[:5].tolist() == [12, 0, 4, 20, 24]                       # corners in index order
    assert seq[5:].tolist() == [2, 10, 14, 22]                          # then the edge midpoints, equally far again
    assert (kept.tolist(), seq.tolist()) == brute_force(xyz, key, 9, 25)


def test_pool_is_the_smallest_keys():
    g = np.random.default_rng(11)
    xyz = g.uniform(-1, 1, size=(200, 3)).astype(f32)
    key = g.permutation(1024)[:200].astype(np.uint32)
    pool = np.argsort(key, kind="stable")[:48]
    kept, seq = ops.rgbd_fps_select(xyz, key, 48, 48)                   # quota == pool: the pool itself
    assert np.array_equal(kept, np.sort(pool))
    kept, seq = ops.rgbd_fps_select(xyz, key, 20, 48)
    assert np.isin(kept, pool).all() and seq[0] == pool[0]
    # the selection over the pool alone is the same selection
    members = np.sort(pool)
    k2, s2 = ops.rgbd_fps_select(xyz[members], key[members], 20, 48)
    assert np.array_equal(members[k2], kept) and np.array_equal(members[s2], seq)
    with pytest.raises(ValueError, match="rgbd_fps_select"):
        ops.rgbd_fps_select(xyz, key, 49, 48)
    with pytest.raises(ValueError, match="rgbd_fps_select"):
        ops.rgbd_fps_select(xyz, key[:-1], 20, 48)


# ---- RGBDFusion's new arguments ------------------------------------------------------------------------------------------------
K, H, W = 2, 64, 96
GOOD = dict(K=K, H=H, W=W, cam_index=[1, 0], intrinsics=[[80.0, 80.0, 48.0, 32.0]] * 2, depth_scale=1e-3,
            extrinsics=np.tile(np.eye(4)[:3], (2, 1, 1)), box=(-1, 1, -1, 1, 0, 3), quota=[32, 20], max_batch=3)


def _make(**over):
    return ops.RGBDFusion("cuda:0", **{**GOOD, **over})


@pytest.mark.parametrize("over,word", [
    (dict(sampling="random"), "sampling"),
    (dict(sampling=None), "sampling"),
    (dict(sampling="fps", fps_pool=31), "fps_pool"),                    # below max(quota)
    (dict(sampling="fps", fps_pool=0), "fps_pool"),
    (dict(sampling="fps", fps_pool=L.RGBD_FPS_MAX_POOL + 1), "fps_pool"),
    (dict(sampling="fps", fps_pool=64.0), "fps_pool"),
    (dict(sampling="fps", quota=[L.RGBD_FPS_MAX_POOL + 1, 8]), "fps_pool"),       # no admissible default pool
    (dict(sampling="key", fps_pool=64), "fps_pool"),
    (dict(fps_pool=64), "fps_pool"),
])
def test_constructor_refuses_the_new_arguments_on_the_host(over, word):
    with pytest.raises(ValueError, match="RGBDFusion.*" + word):
        _make(**over)


def test_fps_pool_default_and_bounds():
    assert L.RGBD_FPS_MAX_POOL == 16384
    assert _make(sampling="fps").fps_pool == 128                        # 4 * max(quota)
    assert _make(sampling="fps", quota=[4096, 4096]).fps_pool == 16384
    assert _make(sampling="fps", quota=[8000, 100]).fps_pool == 16384   # capped
    assert _make(sampling="fps", fps_pool=32).fps_pool == 32            # == max(quota)
    assert _make(sampling="fps", fps_pool=np.int64(16384)).fps_pool == 16384


def test_key_sampling_constructs_exactly_as_before():
    import torch
    gpu = torch.cuda.is_available()                              # (with a GPU the constructor allocates: the fields are the same)
    a, b = _make(), _make(sampling="key")
    for f in (a, b):
        assert f.sampling == "key" and f.fps_pool is None and f.P == 52 and f.quota == [32, 20] and (gpu or f._calib is None)
        assert not gpu or f.order is None
    assert bytes(a._host) == bytes(b._host) and bytes(a._host) == bytes(_make(sampling="fps")._host)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    names = L.declared_symbols(os.path.join(HEADER_DIR, "actmi.h"))
    lib = L.load()
    for n in ("actmi_op_rgbd_cloud_fps", "actmi_op_rgbd_cloud_fps_workspace_bytes"):
        assert n in names and hasattr(lib, n)
    assert "ACTMI_RGBD_FPS_MAX_POOL 16384" in open(os.path.join(HEADER_DIR, "actmi.h")).read()
    # the size query needs no device: the key draw's workspace plus counts, 16-byte points, pixels and pick turns
    base = lib.actmi_op_rgbd_cloud_workspace_bytes(3, 2, 64, 96)
    small, large = (lib.actmi_op_rgbd_cloud_fps_workspace_bytes(3, 2, 64, 96, p) for p in (256, 16384))
    assert base > 0 and small >= base + 3 * 2 * 256 * 24 and large - small == 3 * 2 * (16384 - 256) * 24
    for bad in (0, -1, L.RGBD_FPS_MAX_POOL + 1):
        assert lib.actmi_op_rgbd_cloud_fps_workspace_bytes(3, 2, 64, 96, bad) < 0
    assert lib.actmi_op_rgbd_cloud_fps_workspace_bytes(3, 9, 64, 96, 256) < 0
    assert lib.actmi_op_rgbd_cloud_fps(None, None) == -1 and b"null descriptor" in lib.actmi_op_last_error()
    empty = L.RgbdFpsDesc()                                             # refused on the host, before anything is launched
    assert lib.actmi_op_rgbd_cloud_fps(C.byref(empty), None) == -1 and lib.actmi_op_last_error()


def test_fps_descriptor_matches_the_header_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "actmi.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(actmi_rgbd_fps_desc), sizeof(actmi_rgbd_desc),\n'
                   '         offsetof(actmi_rgbd_fps_desc, pool), offsetof(actmi_rgbd_fps_desc, reserved),\n'
                   '         offsetof(actmi_rgbd_fps_desc, order));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.RgbdFpsDesc
    assert out == [C.sizeof(D), C.sizeof(L.RgbdDesc), D.pool.offset, D.reserved.offset, D.order.offset]
