"""Baseline JPEG encode, the parts that need no GPU: the numpy statement (actmi.ops.jpeg_encode_ref) against PIL's whole file, the
host twin (actmi_jpeg_encode_host, the kernels' core on the CPU) against the statement, the contract at the C boundary, and
compress_episode with the host twin on fabricated .npz episodes.  PIL (libjpeg-turbo) is the definition."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from actmi import data as D
from actmi import lib as L
from actmi import ops
from test_device_dataset_cpu import write_dataset

HS = (1, 2, 7, 8, 9, 10, 15, 16, 17, 24, 31, 33)
WS = (1, 7, 8, 9, 16, 17, 33, 40)
SUB = {"420": 2, "444": 0}


def pil_file(frame, quality, mode, form="rgb"):
    from PIL import Image
    rgb = np.ascontiguousarray(frame if form == "rgb" else frame[..., ::-1])
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=SUB[mode])
    return buf.getvalue()


def frames_of(H, W, n, seed=0):
    """n frames of different content: noise, posterised noise, smooth"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    for i in range(n):
        if i % 3 == 1:
            f[i] = f[i] // 64 * 64
        elif i % 3 == 2:
            yy, xx = np.mgrid[:H, :W]
            f[i] = ((yy * 5 + xx * 3)[..., None] + np.asarray([0, 80, 160])) % 256
    return f


def content(H, W):
    yy, xx = np.mgrid[:H, :W]
    flat = np.empty((H, W, 3), dtype=np.uint8)
    flat[:] = (10, 200, 90)
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    ramp = np.repeat((xx * 255 // max(W - 1, 1)).astype(np.uint8)[..., None], 3, axis=2)
    return {"flat": flat, "checker": checker, "ramp": ramp}


def zrl_frame(mode):
    """R, G, B, 32 x 64, made so that runs of 16 and more zeros lie ahead of a nonzero coefficient on both AC tables: the left half
    is gray with ONE high-frequency luma coefficient a block (natural position (5, 6), zigzag 51) over a flat field; the right half
    has constant luma and one such Cb coefficient a chroma block (a chroma sample covers 2 x 2 pixels in 4:2:0)"""
    k = 2 if mode == "420" else 1
    i = np.arange(8)
    basis = np.outer(np.cos((2 * i + 1) * 5 * np.pi / 16), np.cos((2 * i + 1) * 6 * np.pi / 16))
    H, W = 32, 64
    cb = 100 * np.kron(np.tile(basis, (H // (8 * k), W // (16 * k))), np.ones((k, k)))
    f = np.empty((H, W, 3))
    f[:, :W // 2] = (128 + 100 * np.tile(basis, (H // 8, W // 16)))[..., None]
    f[:, W // 2:, 0] = 128
    f[:, W // 2:, 1] = 128 - 0.344136 * cb
    f[:, W // 2:, 2] = 128 + 1.772 * cb
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def segment(file_bytes, H, W, quality, mode):
    return file_bytes[len(ops.jpeg_file_header(H, W, quality, mode)):-2]


# ---- the statement against PIL -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["420", "444"])
def test_ref_equals_pil_over_the_size_grid(mode):
    rng = np.random.default_rng(1)
    for H in HS:
        for W in WS:
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            if (H + W) & 1:
                a = a // 32 * 32                                  # posterised noise
            assert ops.jpeg_encode_ref(a, 50, mode, "rgb") == pil_file(a, 50, mode), (H, W)


@pytest.mark.parametrize("quality", [1, 25, 75, 90, 95, 100])
def test_ref_equals_pil_at_other_qualities(quality):
    rng = np.random.default_rng(quality)
    for H, W in ((16, 16), (17, 33), (9, 24)):
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for mode in ("420", "444"):
            assert ops.jpeg_encode_ref(a, quality, mode, "rgb") == pil_file(a, quality, mode), (H, W, mode)


def test_ref_equals_pil_on_flat_checker_ramp_and_stuffed_noise():
    H, W = 24, 40
    for name, a in content(H, W).items():
        for quality in (50, 100):
            for mode in ("420", "444"):
                assert ops.jpeg_encode_ref(a, quality, mode, "rgb") == pil_file(a, quality, mode), (name, quality, mode)
    noise = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    f = ops.jpeg_encode_ref(noise, 100, "444", "rgb")
    assert f == pil_file(noise, 100, "444") and b"\xff\x00" in segment(f, H, W, 100, "444")


@pytest.mark.parametrize("mode", ["420", "444"])
def test_zrl_is_emitted_on_both_ac_tables_and_the_bytes_are_pils(mode):
    """the horizontal ramp above leaves no run of 16 zeros ahead of a nonzero coefficient (its blocks end after a few low
    frequencies), so 0xF0 is checked on content made for it, and the statement is asked which symbols it emitted"""
    a = zrl_frame(mode)
    symbols = []
    seg = ops.jpeg_encode_segment_ref(a, 50, mode, "rgb", symbols=symbols)
    luma, chroma = symbols.count((1, 0xF0)), symbols.count((3, 0xF0))
    print(f"{mode}: 0xF0 emitted {luma} times from the luma AC table, {chroma} times from the chroma AC table")
    assert luma >= 3 * 16 and chroma >= 3 * (4 if mode == "420" else 16)     # three a block: a run of 51 zeros
    whole = pil_file(a, 50, mode)
    assert ops.jpeg_assemble(ops.jpeg_file_header(32, 64, 50, mode), seg) == whole
    assert ops.jpeg_encode_host(a, 50, mode, "rgb") == [whole]                # the core's `while (run >= 16)`, on both tables
    assert ops.jpeg_encode_host(a[..., ::-1], 50, mode, "bgr") == [whole]
    ramp = []
    ops.jpeg_encode_segment_ref(content(24, 40)["ramp"], 50, mode, "rgb", symbols=ramp)
    assert (1, 0xF0) not in ramp and (3, 0xF0) not in ramp


def test_form_bgr_is_the_stores_channel_order_and_bad_arguments_raise():
    a = np.random.default_rng(2).integers(0, 256, (9, 17, 3), dtype=np.uint8)
    assert ops.jpeg_encode_ref(a, 50, "420", "bgr") == pil_file(a[..., ::-1], 50, "420")
    assert np.array_equal(ops.jpeg_quant_tables(50), np.asarray(ops._JPEG_STD_Q, dtype=np.uint16))
    for mode in ("422", "gray", "411"):
        with pytest.raises(ValueError):
            ops.jpeg_encode_ref(a, 50, mode)
        with pytest.raises(ValueError):
            ops.jpeg_encode_host(a, 50, mode)
        with pytest.raises(ValueError):
            ops.jpeg_file_header(9, 17, 50, mode)
    for bad in (dict(quality=0), dict(quality=101), dict(form="u16")):
        with pytest.raises(ValueError):
            ops.jpeg_encode_ref(a, **bad)
    with pytest.raises(ValueError):
        ops.jpeg_encode_ref(a[..., :2])


# ---- the host twin against the statement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bgr", "rgb"])
@pytest.mark.parametrize("mode", ["420", "444"])
def test_host_twin_equals_ref_over_the_size_grid(mode, form):
    for H in HS:
        for W in WS:
            f = frames_of(H, W, 3, seed=H * 64 + W)
            got = ops.jpeg_encode_host(f, 50, mode, form)
            assert got == [ops.jpeg_encode_ref(x, 50, mode, form) for x in f], (H, W)


def test_host_twin_equals_ref_at_other_qualities_and_contents():
    for quality in (1, 25, 75, 90, 95, 100):
        for H, W in ((16, 16), (17, 33), (9, 24), (48, 64)):
            f = frames_of(H, W, 3, seed=quality)
            for mode in ("420", "444"):
                assert ops.jpeg_encode_host(f, quality, mode, "rgb") == [ops.jpeg_encode_ref(x, quality, mode, "rgb") for x in f]
    c = np.stack(list(content(24, 40).values()))
    for quality in (50, 100):
        for mode in ("420", "444"):
            assert ops.jpeg_encode_host(c, quality, mode, "rgb") == [pil_file(x, quality, mode) for x in c]


def test_host_twin_output_parses_and_decodes_to_pils_pixels():
    f = frames_of(17, 33, 3, seed=4)
    for mode in ("420", "444"):
        files = ops.jpeg_encode_host(f, 50, mode, "bgr")
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in files]
        info = ops.jpeg_parse(bufs[0])
        assert (info["H"], info["W"], info["mode"], info["restart_interval"]) == (17, 33, mode, 0)
        assert info["seg_len"] == len(segment(files[0], 17, 33, 50, mode))
        out, status = ops.jpeg_decode_host(bufs)
        assert not status.any()
        for i in range(3):
            assert np.array_equal(out[i], D.imdecode_bgr(np.frombuffer(pil_file(f[i], 50, mode, "bgr"), dtype=np.uint8)))


# ---- the contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["420", "444"])
def test_seg_len_is_true_and_nothing_is_written_outside_the_window(mode):
    H, W = 17, 33
    f = frames_of(H, W, 1, seed=8)
    want = segment(ops.jpeg_encode_ref(f[0], 100, mode, "bgr"), H, W, 100, mode)
    n, guard = len(want), 64
    for cap, st in ((0, ops.JPEG_ST_DEST), (n - 1, ops.JPEG_ST_DEST), (n, 0), (n + 9, 0)):
        dst = np.full(cap + 2 * guard, 0xA5, dtype=np.uint8)
        rec = ops.jpeg_enc_records(1, H, W, cap, dst_off=[guard])
        seg_len, status = ops.jpeg_encode_host_raw(f.reshape(-1), rec, dst, H, W, 100, mode)
        assert seg_len.tolist() == [n] and status.tolist() == [st], cap
        assert np.all(dst[:guard] == 0xA5) and np.all(dst[guard + cap:] == 0xA5), cap
        if st == 0:
            assert dst[guard:guard + n].tobytes() == want and np.all(dst[guard + n:guard + cap] == 0xA5)


def test_a_window_or_source_that_leaves_its_buffer_is_dest():
    H, W = 9, 17
    f = frames_of(H, W, 3, seed=3)
    fb, cap = H * W * 3, ops.jpeg_encode_bound(H, W, "420")
    true = [len(segment(x, H, W, 50, "420")) for x in ops.jpeg_encode_host(f, 50, "420")]
    dst = np.full(3 * cap, 0xA5, dtype=np.uint8)
    rec = ops.jpeg_enc_records(3, H, W, cap, dst_off=[0, 2 * cap + 1, -1])
    seg_len, status = ops.jpeg_encode_host_raw(f.reshape(-1), rec, dst, H, W)
    assert status.tolist() == [0, ops.JPEG_ST_DEST, ops.JPEG_ST_DEST] and seg_len.tolist() == true
    assert np.all(dst[cap:] == 0xA5)
    rec = ops.jpeg_enc_records(3, H, W, cap, src_off=[0, 2 * fb + 1, -1])
    dst[:] = 0xA5
    seg_len, status = ops.jpeg_encode_host_raw(f.reshape(-1), rec, dst, H, W)
    assert status.tolist() == [0, ops.JPEG_ST_DEST, ops.JPEG_ST_DEST] and seg_len.tolist() == [true[0], 0, 0]
    assert np.all(dst[cap:] == 0xA5)
    rec = ops.jpeg_enc_records(1, H, W, -5)                       # a negative capacity
    seg_len, status = ops.jpeg_encode_host_raw(f.reshape(-1), rec, dst, H, W)
    assert status.tolist() == [ops.JPEG_ST_DEST] and seg_len.tolist() == [true[0]] and np.all(dst[cap:] == 0xA5)


def test_the_bound_holds_on_noise_at_quality_100_and_is_what_the_header_derives():
    for mode, per_mcu, edge in (("420", 6, 16), ("444", 3, 8)):
        for H, W in ((16, 16), (17, 33), (48, 64)):
            blocks = -(-H // edge) * -(-W // edge) * per_mcu
            assert ops.jpeg_encode_bound(H, W, mode) == 2 * (blocks * 216 + 1)
            f = np.random.default_rng(H).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
            for x in ops.jpeg_encode_host(f, 100, mode):
                assert len(segment(x, H, W, 100, mode)) <= ops.jpeg_encode_bound(H, W, mode)
    assert ops.jpeg_enc_frame_dtype().itemsize == 32 and C.sizeof(L.JpegEncDesc) == 352


def _desc(n=1, H=8, W=8, mode=3, form=0):
    keep = {"src": np.zeros(n * H * W * 3 + 1, dtype=np.uint8), "dst": np.zeros(4096, dtype=np.uint8),
            "rec": ops.jpeg_enc_records(max(n, 1), H, W, 1024), "ws": ops._aligned_u8(1 << 20),
            "len": np.zeros(max(n, 1), dtype=np.int32), "st": np.zeros(max(n, 1), dtype=np.int32)}
    d = ops._jpeg_enc_desc(H, W, 50, "420", "bgr")
    d.src, d.src_bytes, d.frames, d.dst, d.dst_bytes = keep["src"].ctypes.data, n * H * W * 3, keep["rec"].ctypes.data, keep["dst"].ctypes.data, 4096
    d.ws, d.ws_bytes, d.seg_len, d.status = keep["ws"].ctypes.data, keep["ws"].size, keep["len"].ctypes.data, keep["st"].ctypes.data
    d.n, d.H, d.W, d.mode, d.form = n, H, W, mode, form
    return d, keep


def test_invalid_arguments_are_refused_before_anything_runs():
    lib = L.load()
    assert lib.actmi_version() == 110
    d, _keep = _desc()
    assert lib.actmi_jpeg_encode_host(C.byref(d)) == 0
    assert lib.actmi_jpeg_encode_host(None) == -1 and lib.actmi_op_jpeg_encode(None, None) == -1
    changes = [("src", None), ("frames", None), ("dst", None), ("ws", None), ("seg_len", None), ("status", None), ("n", -1), ("n", 65536),
               ("H", 0), ("H", 65536), ("W", 0), ("W", 65536), ("mode", 0), ("mode", 2), ("mode", 4), ("form", 2), ("form", -1),
               ("ws_bytes", 64)]
    for field, value in changes:
        d, _keep = _desc()
        setattr(d, field, value)
        for call in (lambda: lib.actmi_jpeg_encode_host(C.byref(d)), lambda: lib.actmi_op_jpeg_encode(C.byref(d), None)):
            assert call() == -1, (field, value)             # the device entry validates before it launches: no GPU is touched
            assert b"jpeg_encode" in lib.actmi_op_last_error()
    d, _keep = _desc()
    d.q[1][63] = 0
    assert lib.actmi_jpeg_encode_host(C.byref(d)) == -1 and b"zero" in lib.actmi_op_last_error()
    d, _keep = _desc(n=0)
    d.src = d.dst = None
    assert lib.actmi_jpeg_encode_host(C.byref(d)) == 0
    for mode in (0, 2):
        assert lib.actmi_op_jpeg_encode_workspace_bytes(1, 8, 8, mode) == -1 and lib.actmi_jpeg_encode_bound(8, 8, mode) == -1
    assert lib.actmi_op_jpeg_encode_workspace_bytes(65536, 8, 8, 3) == -1 and lib.actmi_jpeg_encode_bound(0, 8, 3) == -1
    # a geometry whose bound does not fit seg_len's int32 is refused by every entry, the size functions included
    assert lib.actmi_jpeg_encode_bound(65535, 65535, 1) == -1 and lib.actmi_op_jpeg_encode_workspace_bytes(1, 65535, 65535, 1) == -1
    assert lib.actmi_jpeg_encode_bound(4096, 4096, 3) == 2 * (256 * 256 * 6 * 216 + 1)
    d, _keep = _desc()
    d.H, d.W, d.mode = 65535, 65535, 1
    assert lib.actmi_jpeg_encode_host(C.byref(d)) == -1 and b"int32" in lib.actmi_op_last_error()


# ---- the entry point ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compressed(tmp_path_factory):
    root = tmp_path_factory.mktemp("enc")
    cams = ["top", "wrist"]
    paths = write_dataset(root / "raw", lengths=(12, 7, 3), cams=cams, hw=(17, 33))
    enc = ops.JpegHostEncoder(17, 33)
    out = D.compress_dataset_dir(str(root / "raw"), encoder=enc)
    return root, cams, paths, out, enc


def test_compress_episode_writes_pils_files_and_carries_the_rest(compressed, capsys):
    root, cams, paths, out, enc = compressed
    assert [os.path.dirname(o) for o in out] == [str(root / "raw_compressed")] * 3 and enc.stats == {"frames": 2 * 22, "fallback": 0}
    for src, dst, sim in zip(paths, out, (True, False, None)):
        with np.load(src) as a, np.load(dst) as b:
            assert bool(b["attrs_compress"]) is True and ("attrs_sim" in b.files) == (sim is not None)
            if sim is not None:
                assert bool(b["attrs_sim"]) == sim
            assert set(b.files) == set(a.files) | {"attrs_compress", "/compress_len"}
            T = len(a["/action"])
            assert b["/compress_len"].shape == (2, T)
            for k in a.files:
                if not k.startswith("/observations/images/"):
                    assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
            for ci, cam in enumerate(cams):
                files = [pil_file(x, 50, "420", "bgr") for x in a[f"/observations/images/{cam}"]]
                rows = b[f"/observations/images/{cam}"]
                assert rows.dtype == np.uint8 and rows.shape == (T, max(len(f) for f in files))
                assert b["/compress_len"][ci].tolist() == [len(f) for f in files]
                for t, f in enumerate(files):
                    assert rows[t, :len(f)].tobytes() == f and not rows[t, len(f):].any()
    assert D.compress_episode(paths[0], out[0], encoder=enc) is None      # an existing output is skipped
    assert f"The file {out[0]} already exists. Exiting..." in capsys.readouterr().out


def test_episodic_dataset_reads_the_result(compressed):
    root, cams, paths, out, _enc = compressed
    stats, lens = D.get_norm_stats(out)
    ds = D.EpisodicDataset(out, cams, stats, [0, 1, 2], lens, 4, "ACT")
    raw = D.EpisodicDataset(paths, cams, stats, [0, 1, 2], lens, 4, "ACT")
    for i in (0, 11, 12, 21):
        img, qpos, action, is_pad = ds[i]
        assert tuple(img.shape) == (2, 17, 33, 3)
        with np.load(out[0 if i < 12 else (1 if i < 19 else 2)]) as z:
            t = i if i < 12 else (i - 12 if i < 19 else i - 19)
            assert np.array_equal(img[0].numpy(), D.imdecode_bgr(z["/observations/images/top"][t]))
        r = raw[i]
        assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip((qpos, action, is_pad), r[1:]))


def test_compress_episode_refusals(compressed, tmp_path):
    root, cams, paths, out, enc = compressed
    with pytest.raises(ValueError, match="already compressed"):
        D.compress_episode(out[0], str(tmp_path / "a.npz"), encoder=enc)
    with pytest.raises(ValueError, match="mirror twin"):
        D.compress_episode(D.MirrorTwinPath(paths[0]), str(tmp_path / "b.npz"), encoder=enc)
    with pytest.raises(ValueError, match=".npz"):
        D.compress_episode(paths[0], str(tmp_path / "c.hdf5"), encoder=enc)
    depth = write_dataset(tmp_path / "depth", lengths=(3,), sims=(True,), cams=cams, hw=(17, 33), depth_cams=["top"])
    with pytest.raises(ValueError, match="depth"):
        D.compress_episode(depth[0], str(tmp_path / "d.npz"), encoder=enc)
    with np.load(paths[2]) as z:
        ep = {k: z[k] for k in z.files}
    ep["/observations/images/top"] = ep["/observations/images/top"].astype(np.uint16)
    np.savez(tmp_path / "u16.npz", **ep)
    with pytest.raises(ValueError, match=r"not uint8 \[T, H, W, 3\]"):
        D.compress_episode(str(tmp_path / "u16.npz"), str(tmp_path / "e.npz"), encoder=enc)
    ep["/observations/images/top"] = ep["/observations/images/wrist"][..., 0]
    np.savez(tmp_path / "gray.npz", **ep)
    with pytest.raises(ValueError, match=r"not uint8 \[T, H, W, 3\]"):
        D.compress_episode(str(tmp_path / "gray.npz"), str(tmp_path / "f.npz"), encoder=enc)
    with pytest.raises(ValueError, match="the encoder is for"):
        D.compress_episode(paths[0], str(tmp_path / "g.npz"), encoder=ops.JpegHostEncoder(16, 32))
    with pytest.raises(ValueError):
        D.compress_episode(paths[0], str(tmp_path / "h.npz"), mode="422", encoder=enc)
    assert not any(os.path.exists(tmp_path / f"{c}.npz") for c in "abdefgh")
