"""What a batch out of the device-resident episode store LAUNCHES: the parity tests of the store prove the bytes of a batch, this one
that the same work is issued for them -- which ops, in which order, over how many items, in which form -- and that every index
tensor of one batch is a slice of ONE upload.  The ops are recorded through the ``actmi.ops`` attributes and then run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402
from test_device_clouds_cpu import NAME, RULE, write_cloud_dataset  # noqa: E402
from test_device_clouds_cpu import CAMS as CLOUD_CAMS  # noqa: E402
from test_device_dataset_cpu import write_dataset  # noqa: E402

DEV = "cuda:0"
CAMS = ["top", "wrist"]


@pytest.fixture
def launches(monkeypatch):
    """-> (calls, indices): every launch as (op, items, form ...) and the index tensors it was handed"""
    calls, indices = [], []
    real = {n: getattr(ops, n) for n in ("gather_frames", "gather_frames_mirror", "gather_clouds", "gather_chunks")}

    def gather_frames(arena, src_off, item_bytes, out=None, aligned=0):
        calls.append(("gather_frames", int(src_off.numel()), int(aligned)))
        indices.append(src_off)
        return real["gather_frames"](arena, src_off, item_bytes, out=out, aligned=aligned)

    def gather_frames_mirror(arena, src_off, flip, H, W, px_bytes, out=None, aligned=0):
        calls.append(("gather_frames_mirror", int(src_off.numel()), int(aligned), int(px_bytes)))
        indices.extend([src_off, flip])
        return real["gather_frames_mirror"](arena, src_off, flip, H, W, px_bytes, out=out, aligned=aligned)

    def gather_clouds(arena, items, P, rgb_fmt, mirror=None, out=None, aligned=0):
        calls.append(("gather_clouds", items.numel() * items.element_size() // ops.cloud_item_dtype().itemsize, int(aligned), int(P),
                      int(rgb_fmt)))
        indices.append(items)
        return real["gather_clouds"](arena, items, P, rgb_fmt, mirror=mirror, out=out, aligned=aligned)

    def gather_chunks(actions, qpos, episodes, samples, *rest):
        calls.append(("gather_chunks", int(samples.shape[0])))
        indices.append(samples)
        return real["gather_chunks"](actions, qpos, episodes, samples, *rest)

    for name, fn in (("gather_frames", gather_frames), ("gather_frames_mirror", gather_frames_mirror), ("gather_clouds", gather_clouds),
                     ("gather_chunks", gather_chunks)):
        monkeypatch.setattr(ops, name, fn)
    return calls, indices


def _issued(launches, call):
    """the launches of one call into the store; its index tensors must all be slices of one upload"""
    calls, indices = launches
    del calls[:], indices[:]
    call()
    torch.cuda.synchronize()
    assert len({t.untyped_storage().data_ptr() for t in indices}) == 1, "more than one index upload for one batch"
    return list(calls)


def _check(launches, store, e, t, form):
    """gather at B = len(e) with both load forms and one replay of episode e[0]; `form(a)` -> the expected launches, a the 16-byte
    form's number (2 non-temporal, 1 plain) where a launch may take it"""
    e, t = np.asarray(e), np.asarray(t)
    assert _issued(launches, lambda: store.gather(e, t, 4, nontemporal=True)) == form(2)
    assert _issued(launches, lambda: store.gather(e, t, 4, nontemporal=False)) == form(1)
    assert _issued(launches, lambda: store.gather(e, t, 4)) == form(2)                    # the default is the non-temporal form


def frames(n, a):
    return ("gather_frames", n, a)


def mirror(n, a, px):
    return ("gather_frames_mirror", n, a, px)


def chunks(n):
    return ("gather_chunks", n)


def clouds(n, a, P):
    return ("gather_clouds", n, a, P, 0)


# ---- frames, with and without depth, with and without twins ----------------------------------------------------------------------
# hw, depth, twins -> the launches of a batch of 3 at the 16-byte form number a.  Frames of 4 x 16 x 3 are 192 bytes and depth frames
# of 4 x 16 128: both 16-byte forms; 5 x 7 frames are 105 / 70 bytes: the general form.  The mirrored op's 16-byte form also needs
# rows of whole 16-pixel (px 3) or 8-pixel (px 2) groups: at 4 x 8 (96 / 64 bytes) only the depth launch takes it
FRAME_CASES = [
    ((4, 16), False, False, lambda a: [frames(6, a), chunks(3)]),
    ((5, 7), False, False, lambda a: [frames(6, 0), chunks(3)]),
    ((4, 16), True, False, lambda a: [frames(6, a), chunks(3), frames(3, a)]),
    ((5, 7), True, False, lambda a: [frames(6, 0), chunks(3), frames(3, 0)]),
    ((4, 16), False, True, lambda a: [mirror(6, a, 3), chunks(3)]),
    ((4, 16), True, True, lambda a: [mirror(6, a, 3), chunks(3), mirror(3, a, 2)]),
    ((4, 8), True, True, lambda a: [mirror(6, 0, 3), chunks(3), mirror(3, a, 2)]),
    ((5, 7), True, True, lambda a: [mirror(6, 0, 3), chunks(3), mirror(3, 0, 2)]),
]


@pytest.mark.parametrize("hw,depth,twins,form", FRAME_CASES,
                         ids=[f"{h}x{w}{'-depth' if d else ''}{'-twins' if tw else ''}" for (h, w), d, tw, _f in FRAME_CASES])
def test_frame_stores_launch_what_they_always_did(tmp_path, launches, hw, depth, twins, form):
    paths = write_dataset(tmp_path, lengths=(6, 5, 7), cams=CAMS, hw=hw, base=True, depth_cams=("top",) if depth else ())
    kw = dict(depth_camera_names=["top"], use_depth=True) if depth else {}
    if twins:                                                        # the top camera (and the depth camera of its name) is flipped
        paths = D.mirror_twin_paths(paths, D.MirrorSpec(flip=("top",)))
    stats, _ = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, range(len(paths)), CAMS, stats, DEV, **kw)
    assert store.has_twins == twins and store.Kd == (1 if depth else 0)
    e = [0, 4, 2] if twins else [0, 1, 2]                            # episode 4 is the twin of file 1
    assert not twins or store.twin[4]
    _check(launches, store, e, [0, 1, 2], form)
    out = []
    assert _issued(launches, lambda: out.append(store.replay_batch(e[1], [0, 2, 3, 4]))) == \
        [(c[0], c[1] // 3 * 4) + c[2:] for c in form(2)]            # a batch of 4 steps of ONE episode, the same launches
    assert len(out[0]) == (3 if depth else 2)


# ---- stored clouds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("twins", [False, True], ids=["files", "twins"])
def test_cloud_stores_launch_the_clouds_first(tmp_path, launches, twins):
    """3 cameras of 12 x 16 x 3 (576 bytes: the 16-byte forms) and clouds of N = 8 and 6 stored rows: P is the batch's largest, and
    the cloud launch takes its 16-byte form only where P is a multiple of 4"""
    paths = write_cloud_dataset(tmp_path, Ns=(8, 6), T=6)
    if twins:
        paths = D.mirror_twin_paths(paths, cloud_mirror=RULE)        # episode_0, episode_1, mirror_episode_0, mirror_episode_1
    stats, _ = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, range(len(paths)), list(CLOUD_CAMS), stats, DEV, use_pcd=True, pointcloud_names=[NAME])
    assert store.has_clouds and store.has_twins == twins and store.cloud_rgb_fmt == 0

    def form(P, cloud_form):
        def launched(a):
            return [clouds(3, a if cloud_form else 0, P), mirror(9, a, 3) if twins else frames(9, a), chunks(3)]
        return launched
    long, short = ([0, 3, 1], [1, 3, 1]) if twins else ([0, 1, 1], [1, 1, 1])
    _check(launches, store, long, [0, 5, 2], form(8, True))
    _check(launches, store, short, [0, 5, 2], form(6, False))
    out = []
    assert _issued(launches, lambda: out.append(store.replay_batch(short[1], [1, 2, 4]))) == form(6, False)(2)
    assert _issued(launches, lambda: out.append(store.replay_batch(0, [1, 2, 4]))) == form(8, True)(2)
    assert len(out[0]) == 5 and out[1][2].shape == (3, 8, 3)
