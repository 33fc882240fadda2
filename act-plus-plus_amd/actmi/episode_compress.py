"""Raw episodes into compressed ones (the reference's ``compress_data.py``): every ``/observations/images/<cam>`` frame becomes the
JPEG file ``cv2.imencode('.jpg', frame, [IMWRITE_JPEG_QUALITY, quality])`` / PIL writes for it, encoded on the device by
``ops.JpegEncoder`` (actmi_op_jpeg_encode), and the result is an episode that ``EpisodicDataset`` and
``DeviceEpisodeStore(device_decode=True, store_compressed=True)`` read as it is.

``compress_episode`` deviates from the reference script in these ways:
* an existing output is skipped with the reference's message;
* the container written is ``.npz`` whatever the source's (h5py is absent where this is built and tested, and an HDF5 writer that
  is never executed helps nobody); the keys and attributes are the HDF5 layout's, as ``open_episode`` reads them;
* no video is written;
* a source with ``/observations/depth_images`` entries is refused (``ValueError``): the ``compress`` attribute covers the whole file,
  and an 8-bit JPEG cannot hold raw uint16 depth;
* a source that is already compressed is refused (``ValueError``);
* frames that are not uint8 ``[T, H, W, 3]`` are refused (``ValueError``);
* a mirror twin path is refused (``ValueError``): a twin is a view, compress its source."""
import os

import numpy as np
import torch

from . import ops
from .episode_files import MirrorTwinPath, _entry_meta, _NpzEpisode, open_episode

IMG, DEPTH = "/observations/images/", "/observations/depth_images/"
STAGE_FRAMES = 64                                               # frames encoded at a time: bounds the pinned and the device staging


def _entries(root):
    """every array entry of an open episode by its full key -> (image cameras in file order, depth entries, the other keys)"""
    if isinstance(root, _NpzEpisode):
        keys = [k for k in root._z.files if not k.startswith("attrs_")]
    else:                                                        # h5py: walk the groups
        keys = []
        root.visititems(lambda name, obj: keys.append("/" + name) if hasattr(obj, "dtype") else None)
    cams = [k[len(IMG):] for k in keys if k.startswith(IMG)]
    depth = [k for k in keys if k.startswith(DEPTH)]
    return cams, depth, [k for k in keys if not k.startswith(IMG)]


def compress_episode(src_path, dst_path, quality=50, mode="420", encoder=None, device=None):
    """One raw episode file -> one compressed ``.npz`` episode at `dst_path`: every non-image entry and attribute copied, every
    camera's frames as uint8 ``[T, max_len]`` rows (one zero-padded JPEG file each), ``attrs_compress = True`` and ``/compress_len``
    ``[cams, T]``.  The frames go through a pinned staging buffer to the device ``STAGE_FRAMES`` at a time.  ``encoder``: an
    ``ops.JpegEncoder`` (or the CPU twin, ``ops.JpegHostEncoder``) for the episode's frame size, quality and mode, reused across
    episodes; without it one is made on `device` (default: the current one).  -> the encoder used, or None when the output exists."""
    if isinstance(src_path, MirrorTwinPath):
        raise ValueError(f"{src_path}: a mirror twin is a view of {src_path.source}; compress that file")
    if not str(dst_path).endswith(".npz"):
        raise ValueError(f"{dst_path}: the compressed episode is written as .npz")
    if os.path.exists(dst_path):
        print(f"The file {dst_path} already exists. Exiting...")
        return None
    ops._jpeg_enc_args(mode, quality=quality)
    out = {}
    with open_episode(src_path) as root:
        attrs = dict(root.attrs)
        if bool(attrs.get("compress", False)):
            raise ValueError(f"{src_path}: the episode is already compressed")
        cams, depth, others = _entries(root)
        if depth:
            raise ValueError(f"{src_path}: {depth[0]} is raw depth, which an 8-bit JPEG cannot hold (the compress attribute covers the whole file)")
        if not cams:
            raise ValueError(f"{src_path}: no {IMG}<cam> entries")
        for cam in cams:
            shape, dtype = _entry_meta(root, IMG + cam)
            if dtype != np.uint8 or len(shape) != 4 or shape[3] != 3 or 0 in shape:
                raise ValueError(f"{src_path}: {IMG}{cam} is {dtype} {shape}, not uint8 [T, H, W, 3]")
            if shape[1:3] != _entry_meta(root, IMG + cams[0])[0][1:3]:
                raise ValueError(f"{src_path}: the cameras' frames differ in size")
        H, W = _entry_meta(root, IMG + cams[0])[0][1:3]
        if encoder is None:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            encoder = ops.JpegEncoder(dev, H, W, max_frames=STAGE_FRAMES, quality=quality, mode=mode)
        elif (encoder.H, encoder.W, encoder.quality, encoder.mode) != (H, W, int(quality), mode):
            raise ValueError(f"{src_path}: frames {H} x {W} at quality {quality}, mode {mode}; the encoder is for {encoder.H} x {encoder.W} "
                             f"at quality {encoder.quality}, mode {encoder.mode}")
        for k in others:
            out[k] = np.asarray(root[k][()])
        on_device = encoder.device is not None
        per = max(1, min(STAGE_FRAMES, encoder.max_frames))
        pin = torch.empty((per, H, W, 3), dtype=torch.uint8, pin_memory=on_device)
        lens = []
        for cam in cams:
            frames = root[IMG + cam]
            frames = frames[()] if isinstance(root, _NpzEpisode) else frames     # an .npz member is decompressed whole on every access
            T = int(frames.shape[0])
            files = []
            for t0 in range(0, T, per):
                n = min(per, T - t0)
                pin.numpy()[:n] = frames[t0:t0 + n]
                src = pin[:n].to(encoder.device, non_blocking=True) if on_device else pin[:n]
                files += encoder.files(src, "bgr")                  # reads back: the staging buffer is free again
            lens.append([len(f) for f in files])
            rows = np.zeros((T, max(lens[-1])), dtype=np.uint8)
            for t, f in enumerate(files):
                rows[t, :len(f)] = np.frombuffer(f, dtype=np.uint8)
            out[IMG + cam] = rows
    if len({len(l) for l in lens}) != 1:
        raise ValueError(f"{src_path}: the cameras differ in length, /compress_len [cams, T] cannot hold them")
    out["/compress_len"] = np.asarray(lens, dtype=np.float32)       # create_dataset's default dtype in the reference script
    for k, v in attrs.items():
        out["attrs_" + k] = np.asarray(v)
    out["attrs_compress"] = np.asarray(True)
    tmp = str(dst_path)[:-4] + ".partial.npz"
    np.savez(tmp, **out)
    os.replace(tmp, dst_path)
    print(f"Compressed dataset saved to {dst_path}")
    return encoder


def compress_dataset_dir(dataset_dir, quality=50, mode="420", device=None, encoder=None):
    """every episode file of `dataset_dir` into ``<dataset_dir>_compressed`` (created), one encoder per frame size -> the outputs"""
    out_dir = str(dataset_dir).rstrip("/") + "_compressed"
    os.makedirs(out_dir, exist_ok=True)
    encoders, written = {}, []
    for name in sorted(os.listdir(dataset_dir)):
        if not name.endswith((".hdf5", ".npz")):
            continue
        src = os.path.join(dataset_dir, name)
        dst = os.path.join(out_dir, os.path.splitext(name)[0] + ".npz")
        if os.path.exists(dst):
            print(f"The file {dst} already exists. Exiting...")
            continue
        with open_episode(src) as root:
            cams = _entries(root)[0]
            key = _entry_meta(root, IMG + cams[0])[0][1:3] if cams else None
        enc = compress_episode(src, dst, quality, mode, encoder=encoder if encoder is not None else encoders.get(key), device=device)
        if enc is not None and encoder is None:
            encoders[key] = enc
        written.append(dst)
    return written
