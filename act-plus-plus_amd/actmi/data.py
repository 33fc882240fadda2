"""Input pipeline of the ACT training loop: the reference's ``utils.py`` dataset logic feeding the
accelerated step.

Mirrors, with the reference's names and argument meaning:
``get_norm_stats`` (utils.py:176-224), ``find_all_hdf5`` (:226-235), ``BatchSampler`` (:237-247),
``EpisodicDataset`` (:41-174; ``_locate_transition``, ``__getitem__``) and ``load_data`` (:249-301).

Differences, all on the host side of the step:
* images stay **u8 NHWC** ``[C, H, W, 3]`` (the engine's fast input format; the ``/255`` and the ImageNet normalisation are
  fused into the conv1 loader) — ``f32_images=True`` reproduces the reference contract (f32 ``[C, 3, H, W]`` in [0, 1]);
* depth frames (``use_depth``; ``/observations/depth_images/<cam>``) stay **raw uint16** ``[Cd, 1, H, W]`` when the episode
  stores an unsigned integer of at most 16 bits: the engine finds every sample's min / max on the device and fuses the
  reference's per-sample ``(d - min) / (max - min + 1e-6)`` into the depth stem's loader -- ``f32_depth=True`` (and any other
  stored dtype) reproduces the reference contract, f32 normalised on the host;
* point clouds (``use_pcd``; the fork's ``/observations/pointcloud/<name>/{xyz, rgb, padding_mask}``, one fused cloud) come
  with their **valid count**: the recorder pads every frame's cloud with zero rows up to the episode's largest, and the stored
  ``padding_mask`` (True = a point) says how many rows are points.  The fork's dataset ignores the mask, so its policy sees the
  zero rows as points; here the mask is honoured unless ``pcd_ignore_mask=True``, because the live cloud of deployment has no
  padding.  ``collate_pcd`` pads a batch's clouds with zero rows to the batch's largest stored row count and the batch becomes
  the 7-tuple ``(image, qpos, action, is_pad, pcd_xyz [B, P, 3] f32, pcd_rgb [B, P, 3] f32, pcd_n [B] int32)``; the engine
  takes the maximum over the first ``pcd_n`` rows of every sample only;
* batches are collated into **pinned** buffers and handed to the device by ``DevicePrefetcher`` on a side stream while
  the previous step computes (the reference moves 944 MB of f32 images per batch-64 step synchronously);
* episode files are opened through ``open_episode``: HDF5 via ``h5py`` when it is importable (the reference's format:
  ``/observations/qpos``, ``/observations/qvel``, ``/observations/images/<cam>``, ``/action``, optional ``/base_action``,
  attrs ``sim`` / ``compress``), or ``.npz`` files with the same keys (``attrs_sim`` / ``attrs_compress`` entries) — what
  the tests use, since neither h5py nor cv2 exists in the build container;
* compressed episodes (attr ``compress``: every frame a zero-padded JPEG byte string, utils.py:104-107) are decoded with PIL
  (libjpeg, like cv2) and flipped to the B, G, R channel order ``cv2.imdecode(buf, 1)`` returns -- **parity unpinned** against
  cv2 itself (absent here); the Diffusion-only augmentations (torchvision transforms, utils.py:141-156) are not handled.
  Everything else is checked against an independent restatement in ``tests/test_data_pipeline_cpu.py``;
* ``EpisodeReplay`` reads ONE episode in time order for the open-loop replay evaluation (``imitate_episodes.replay_bc``): the
  same tensors as ``EpisodicDataset.__getitem__`` without the action chunk, in batches of consecutive steps;
* ``DeviceEpisodeStore`` (``load_data(..., device_dataset=True)``, opt-in) reads every episode ONCE into a device arena; a
  training batch is then two device gathers (three with depth) that give the tensors of ``EpisodicDataset.__getitem__`` + the
  default collation bit for bit, with no host work, loader worker or PCIe traffic per step;
* ``DeviceEpisodeReplay`` is ``EpisodeReplay`` out of such a store (``DeviceEpisodeStore.replay_batch``): one stored episode in
  time order, the same tensors bit for bit, already on the device -- what ``--replay_every`` replays while training;
* ``load_data(..., mirror_twins=True)`` joins every episode file by its **mirrored twin** (``MirrorTwinPath``, ``MirrorSpec``): the
  episode the reference's ``postprocess_episodes.py`` writes beside it -- arms swapped with a per-joint sign vector, the base's
  turn rate negated, the wrist cameras swapped and flipped, the top camera flipped -- computed from the file as it is read
  instead of stored.  Two deviations from the reference's files: the twin is the exact mirror image (the script re-encodes every
  mirrored frame as JPEG at quality 50) and its rows are float32.  Depth cameras, which the reference does not mirror, follow
  their RGB camera.  In a ``DeviceEpisodeStore`` a twin shares its source's frames: ``actmi_op_gather_frames_mirror`` flips them
  inside the batch's gather;
* ``load_data(..., device_clouds=True)`` (with ``device_dataset`` and ``use_pcd``, opt-in) puts the stored clouds into the store as
  well: the device loaders then deliver ``collate_pcd``'s 7-tuples, the clouds gathered by ``actmi_op_gather_clouds``; and a stored
  cloud gets a **mirror rule** (``MirrorTwinPath(..., cloud_mirror=(axis, offset))``, ``load_data(..., cloud_mirror=...)``: one
  coordinate reflected across a plane of the clouds' frame), with which ``mirror_twins`` and ``use_pcd`` go together, on the host
  loader and in the store alike."""
import fnmatch
import os

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------------------
# episode files
# ---------------------------------------------------------------------------------------------------------------------
class _NpzEpisode:
    """read-only view of an ``.npz`` episode with the HDF5 key layout"""

    def __init__(self, path):
        self._z = np.load(path, allow_pickle=False)
        self.attrs = {k[len("attrs_"):]: self._z[k].item() for k in self._z.files if k.startswith("attrs_")}

    def __contains__(self, key):
        return key in self._z.files

    def __getitem__(self, key):
        return self._z[key]          # ndarray: supports [()] and [index] like an h5py dataset

    def meta(self, key):
        """(shape, dtype) of an entry from its ``.npy`` header: nothing is decompressed"""
        from numpy.lib import format as fmt
        with self._z.zip.open(key + ".npy") as f:
            version = fmt.read_magic(f)
            if version == (1, 0):
                shape, _, dtype = fmt.read_array_header_1_0(f)
            elif version == (2, 0):
                shape, _, dtype = fmt.read_array_header_2_0(f)
            else:                                                  # a header this reader does not know: load the entry
                a = self._z[key]
                shape, dtype = a.shape, a.dtype
        return tuple(int(v) for v in shape), np.dtype(dtype)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self._z.close()
        return False


# ---------------------------------------------------------------------------------------------------------------------
# mirrored twin episodes (``load_data(..., mirror_twins=True)``; DESIGN.md "Mirrored twin episodes")
# ---------------------------------------------------------------------------------------------------------------------
class MirrorSpec:
    """What the mirror image of a two-arm episode is (the reference's postprocess_episodes.py:15-19, 67-86).

    ``swap``: pairs of cameras that change places; ``flip``: the cameras whose frames are flipped along W (a swapped camera is
    named by the place it ends up in; the reference flips both of a pair); every other camera passes through.  A state row
    (qpos, qvel, action) becomes ``x[:, state_perm] * state_sign`` and a ``/base_action`` row ``x * base_sign``, as float32."""

    STATE_MULTIPLY = (-1, 1, 1, -1, 1, -1, 1)                    # MIRROR_STATE_MULTIPLY, per arm
    BASE_MULTIPLY = (1, -1)                                      # MIRROR_BASE_MULTIPLY: the base's turn rate changes sign

    def __init__(self, swap=(), flip=(), state_perm=None, state_sign=None, base_sign=None):
        self.swap = tuple((str(a), str(b)) for a, b in swap)
        self.flip = frozenset(str(c) for c in flip)
        self.state_perm = np.asarray(list(range(7, 14)) + list(range(7)) if state_perm is None else state_perm, dtype=np.int64)
        self.state_sign = np.asarray(self.STATE_MULTIPLY * 2 if state_sign is None else state_sign, dtype=np.float32)
        self.base_sign = np.asarray(self.BASE_MULTIPLY if base_sign is None else base_sign, dtype=np.float32)
        if self.state_perm.shape != self.state_sign.shape or self.state_perm.ndim != 1 or \
                sorted(self.state_perm.tolist()) != list(range(len(self.state_perm))):
            raise ValueError("MirrorSpec: state_perm must be a permutation and state_sign as long as it")
        names = [c for pair in self.swap for c in pair]
        if len(set(names)) != len(names):
            raise ValueError(f"MirrorSpec: a camera is named in more than one swap pair: {self.swap}")
        self._source = {a: b for a, b in self.swap}
        self._source.update({b: a for a, b in self.swap})

    @classmethod
    def from_camera_names(cls, camera_names):
        """the reference's rule for the cameras an episode holds: the wrist pair is swapped and both are flipped, the top camera
        is flipped, any other camera passes through; no wrist pair or no top camera: ValueError (the script raises there)"""
        names = list(camera_names)
        for pair in (("left_wrist", "right_wrist"), ("cam_left_wrist", "cam_right_wrist")):
            if pair[0] in names:
                if pair[1] not in names:
                    raise ValueError(f"mirror twins: {pair[0]} without {pair[1]} among the cameras {names}")
                break
        else:
            raise ValueError(f"mirror twins: no left_wrist or cam_left_wrist among the cameras {names}")
        for top in ("top", "cam_high"):
            if top in names:
                break
        else:
            raise ValueError(f"mirror twins: no top or cam_high among the cameras {names}")
        return cls(swap=(pair,), flip=pair + (top,))

    def source_camera(self, cam):
        """the camera of the source episode whose frames the twin shows as ``cam``"""
        return self._source.get(cam, cam)

    def flips(self, cam):
        return cam in self.flip

    def mirror_state(self, x, where=""):
        x = np.asarray(x)
        if x.ndim != 2 or x.shape[1] != len(self.state_perm):
            raise ValueError(f"{where}: a mirror twin needs state rows {len(self.state_perm)} wide, got {x.shape}")
        return np.ascontiguousarray(x[:, self.state_perm] * self.state_sign, dtype=np.float32)

    def mirror_base(self, x, where=""):
        x = np.asarray(x)
        if x.ndim != 2 or x.shape[1] != len(self.base_sign):
            raise ValueError(f"{where}: a mirror twin needs /base_action rows {len(self.base_sign)} wide, got {x.shape}")
        return np.ascontiguousarray(x * self.base_sign, dtype=np.float32)


class MirrorTwinPath(str):
    """The handle of the mirrored twin of an episode file: a ``str`` whose value is the virtual path ``<dir>/mirror_<basename>``
    (where postprocess_episodes.py writes the twin, so filters, sorting and printing treat it like that file) and which carries
    ``.source`` (the file it is the image of), ``.spec`` (a ``MirrorSpec``, or None: the reference's rule for the cameras the file
    holds) and ``.depth_follows`` (depth camera -> the RGB camera whose swap and flip it shares; None: the camera of its own
    name) and ``.cloud_mirror`` (``(axis, offset)``: the twin's stored point clouds are the source's reflected across the plane
    ``x[axis] = offset`` of the clouds' frame, ``cloud_mirror_rule``; None: the twin holds no clouds).  ``open_episode`` gives a view
    of the source file; nothing is written."""

    def __new__(cls, source, spec=None, depth_follows=None, cloud_mirror=None):
        source = str(source)
        self = super().__new__(cls, os.path.join(os.path.dirname(source), "mirror_" + os.path.basename(source)))
        self.source, self.spec = source, spec
        self.depth_follows = dict(depth_follows) if depth_follows else None
        self.cloud_mirror = None if cloud_mirror is None else cloud_mirror_rule(cloud_mirror)[:2]
        return self

    def __reduce__(self):                                        # loader workers receive the dataset pickled
        return (MirrorTwinPath, (self.source, self.spec, self.depth_follows, self.cloud_mirror))


def cloud_mirror_rule(cloud_mirror):
    """``(axis, offset)`` checked -> (axis 0..2, offset as a float, c2 = float32(2 * offset)).  The mirror image of a stored cloud:
    ``xyz[..., axis] -> c2 - xyz[..., axis]`` over EVERY stored row (the recorder's zero rows too), one float32 subtract; colours
    and ``padding_mask`` are unchanged."""
    try:
        axis, offset = cloud_mirror
        axis = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
        ok = int(axis) == axis and 0 <= int(axis) <= 2 and bool(np.isfinite(float(offset)))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"cloud_mirror must be (axis 0..2 or 'x' / 'y' / 'z', a finite offset), got {cloud_mirror!r}")
    with np.errstate(over="ignore"):
        c2 = np.float32(2.0 * float(offset))
    if not np.isfinite(c2):
        raise ValueError(f"cloud_mirror: 2 * offset {offset!r} is not a finite float32")
    return int(axis), float(offset), c2


def mirror_cloud_xyz(xyz, cloud_mirror):
    """the xyz rows of a twin's cloud: float32, coordinate ``axis`` of every row reflected (``cloud_mirror_rule``)"""
    axis, _offset, c2 = cloud_mirror_rule(cloud_mirror)
    out = np.array(xyz, dtype=np.float32)                        # a copy, float32 as the dataset converts
    if out.ndim < 1 or out.shape[-1] != 3:
        raise ValueError(f"a point cloud's xyz ends in 3 coordinates, got {out.shape}")
    out[..., axis] = c2 - out[..., axis]
    return out


class _MirrorCloud:
    """the xyz entry of a twin's cloud: the source entry, read where it is indexed and reflected there"""

    def __init__(self, entry, cloud_mirror):
        self._entry, self._rule = entry, cloud_mirror

    def __getitem__(self, sel):
        return mirror_cloud_xyz(self._entry[sel], self._rule)

    def __array__(self, dtype=None, copy=None):
        a = self[()]
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return int(self._entry.shape[0])

    @property
    def shape(self):
        return tuple(int(v) for v in self._entry.shape)

    @property
    def dtype(self):
        return np.dtype(np.float32)


class _MirrorFrames:
    """the frames of one camera of a twin: the source entry, read where it is indexed, decoded where the source is compressed,
    flipped along W where the spec says so"""

    def __init__(self, entry, flip, compressed, meta=None):
        self._entry, self._flip, self._compressed, self._meta = entry, bool(flip), bool(compressed), meta

    def _frames(self, raw):
        raw = np.asarray(raw)
        if self._compressed:                                      # utils.py:104-107: one zero-padded JPEG per frame
            raw = imdecode_bgr(raw) if raw.ndim == 1 else np.stack([imdecode_bgr(buf) for buf in raw])
            fdim = 3
        else:
            fdim = len(self._entry.shape) - 1
        if self._flip:
            raw = np.flip(raw, axis=raw.ndim - fdim + 1)          # axis 1 of a frame [H, W(, C)]
        return np.ascontiguousarray(raw)

    def __getitem__(self, sel):
        return self._frames(self._entry[sel])

    def __array__(self, dtype=None, copy=None):
        a = self[()]
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return int(self._entry.shape[0])

    @property
    def shape(self):
        if self._compressed:
            return (len(self),) + tuple(imdecode_bgr(np.asarray(self._entry[0])).shape)
        return tuple(int(v) for v in self._entry.shape)

    @property
    def dtype(self):
        return np.dtype(np.uint8) if self._compressed else np.dtype(self._entry.dtype)


class _MirrorEpisode:
    """read-only view of the mirrored twin of an episode file: the entries postprocess_episodes.py writes (qpos, qvel, action,
    ``/base_action`` when the source has it, the cameras) computed from the source as they are read, as an UNCOMPRESSED episode
    with float32 rows; depth cameras follow their RGB camera.  ``attrs``: the source's without ``compress``."""

    STATE_KEYS = ("/observations/qpos", "/observations/qvel", "/action")
    IMG, DEPTH, PCD = "/observations/images/", "/observations/depth_images/", "/observations/pointcloud/"

    def __init__(self, twin):
        self.path, self.source = twin, twin.source
        self._root = open_episode(twin.source)
        try:
            self._compressed = bool(self._root.attrs.get("compress", False))
            self.attrs = {k: v for k, v in dict(self._root.attrs).items() if k != "compress"}
            self.cameras = self._names(self.IMG)
            self.spec = twin.spec if twin.spec is not None else MirrorSpec.from_camera_names(self.cameras)
            self.depth_follows = twin.depth_follows or {}
            self.cloud_mirror = getattr(twin, "cloud_mirror", None)
            back = {}
            for d in self._names(self.DEPTH):
                rgb = self.depth_follows.get(d, d)
                if rgb in back:
                    raise ValueError(f"{twin}: depth cameras {back[rgb]} and {d} both follow {rgb}")
                back[rgb] = d
            self._depth_of = back                                 # RGB camera -> the depth camera that follows it
        except Exception:
            self._root.__exit__(None, None, None)
            raise

    def _names(self, prefix):
        root = self._root
        if isinstance(root, _NpzEpisode):
            return [k[len(prefix):] for k in root._z.files if k.startswith(prefix)]
        return list(root[prefix].keys()) if prefix in root else []

    def _resolve(self, key):
        """-> (kind, source key, flip) of an entry the twin holds, None of one it does not"""
        if key in self.STATE_KEYS:
            return ("state", key, False) if key in self._root else None
        if key == "/base_action":
            return ("base", key, False) if key in self._root else None
        if key.startswith(self.IMG):
            cam = key[len(self.IMG):]
            src = self.IMG + self.spec.source_camera(cam)
            return ("frames", src, self.spec.flips(cam)) if key in self._root and src in self._root else None
        if key.startswith(self.DEPTH):
            cam = key[len(self.DEPTH):]
            rgb = self.depth_follows.get(cam, cam)
            src_rgb = self.spec.source_camera(rgb)
            src = self._depth_of.get(src_rgb) if src_rgb != rgb else cam
            if src is None:
                raise ValueError(f"{self.path}: depth camera {cam} follows {rgb}, whose mirror image is {src_rgb}: no depth camera "
                                 f"follows that one")
            return ("frames", self.DEPTH + src, self.spec.flips(rgb)) if key in self._root and self.DEPTH + src in self._root else None
        if key.startswith(self.PCD) and self.cloud_mirror is not None and key in self._root:
            leaf = key.rsplit("/", 1)[1]                           # a twin without a cloud rule holds no clouds
            if leaf == "xyz":
                return ("cloud", key, False)
            if leaf in ("rgb", "padding_mask"):
                return ("same", key, False)
        return None

    def __contains__(self, key):
        return self._resolve(key) is not None

    def keys(self):
        names = [k for k in self.STATE_KEYS + ("/base_action",) if k in self]
        clouds = []                                               # an .npz lists <name>/<leaf>, an HDF5 group its <name>s
        for k in self._names(self.PCD):
            leaves = [k] if "/" in k else [f"{k}/{leaf}" for leaf in ("xyz", "rgb", "padding_mask")]
            clouds += [self.PCD + c for c in leaves if self.PCD + c in self]
        return names + [self.IMG + c for c in self.cameras] + [self.DEPTH + d for d in self._names(self.DEPTH)] + clouds

    def __getitem__(self, key):
        r = self._resolve(key)
        if r is None:
            raise KeyError(f"{self.path}: a mirror twin holds no {key}")
        kind, src, flip = r
        if kind == "state":
            return self.spec.mirror_state(self._root[src][()], f"{self.path}: {key}")
        if kind == "base":
            return self.spec.mirror_base(self._root[src][()], f"{self.path}: {key}")
        if kind == "cloud":
            return _MirrorCloud(self._root[src], self.cloud_mirror)
        if kind == "same":
            return self._root[src]
        return _MirrorFrames(self._root[src], flip, self._compressed)

    def meta(self, key):
        """(shape, dtype) of an entry from the source's headers (a compressed source: its first frame is decoded)"""
        r = self._resolve(key)
        if r is None:
            raise KeyError(f"{self.path}: a mirror twin holds no {key}")
        kind, src, _flip = r
        shape, dtype = _entry_meta(self._root, src)
        if kind == "same":
            return shape, dtype
        if kind != "frames":
            return shape, np.dtype(np.float32)
        if self._compressed:
            return (shape[0],) + tuple(imdecode_bgr(np.asarray(self._root[src][0])).shape), np.dtype(np.uint8)
        return shape, dtype

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self._root.__exit__(*a)
        return False


def mirror_twin_paths(files, spec=None, depth_follows=None, cloud_mirror=None):
    """`files` and the twin of every one of them, sorted by path as ``find_all_hdf5`` sorts: the list a directory gives in which
    postprocess_episodes.py has written ``mirror_<name>`` beside every ``<name>``"""
    return sorted(list(files) + [MirrorTwinPath(f, spec, depth_follows, cloud_mirror) for f in files])


def open_episode(path):
    if isinstance(path, MirrorTwinPath):
        return _MirrorEpisode(path)
    if path.endswith(".npz"):
        return _NpzEpisode(path)
    try:
        import h5py
    except ImportError as e:                                     # pragma: no cover - h5py is absent in the build container
        raise RuntimeError(f"{path}: reading HDF5 episodes needs h5py") from e
    return h5py.File(path, "r")


def imdecode_bgr(buf):
    """``np.array(cv2.imdecode(buf, 1))`` (utils.py:104-107) without cv2: `buf` is a 1-D u8 array holding one JPEG (or PNG) file,
    zero-padded to the episode's common length; the result is H x W x 3 u8 in cv2's B, G, R order."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(np.ascontiguousarray(buf, dtype=np.uint8).tobytes())) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[..., ::-1])


def preprocess_base_action(base_action):
    """utils.py:312-321 (smoothing of the mobile-base action by a length-5 moving average per column)."""
    base_action = np.asarray(base_action)
    return np.stack([np.convolve(base_action[:, i], np.ones(5) / 5, mode="same") for i in range(base_action.shape[1])],
                    axis=-1).astype(np.float32)


def _read_action(root):
    if "/base_action" in root:
        return np.concatenate([root["/action"][()], preprocess_base_action(root["/base_action"][()])], axis=-1)
    return root["/action"][()]


def _list_hdf5(dataset_dir, skip_mirrored_data):
    files = []
    for root, _dirs, names in os.walk(dataset_dir):
        for pat in ("*.hdf5", "*.npz"):
            for filename in fnmatch.filter(names, pat):
                if "features" in filename:
                    continue
                if skip_mirrored_data and "mirror" in filename:
                    continue
                files.append(os.path.join(root, filename))
    files.sort()                                                 # os.walk order is file-system dependent
    return files


def find_all_hdf5(dataset_dir, skip_mirrored_data):
    files = _list_hdf5(dataset_dir, skip_mirrored_data)
    print(f"Found {len(files)} hdf5 files")
    return files


def find_all_hdf5_with_twins(dataset_dir, skip_mirrored_data, spec=None, depth_follows=None, cloud_mirror=None):
    """``find_all_hdf5`` for ``mirror_twins``: the directory's own files (mirrored ones skipped) and the twin of every one of them,
    sorted by path -- the list ``find_all_hdf5(dataset_dir, False)`` gives once postprocess_episodes.py has run there.  Mirrored
    files that are listed (present, and not skipped) are refused: twins of twins and duplicates are never wanted."""
    files = _list_hdf5(dataset_dir, True)
    print(f"Found {len(files)} hdf5 files, each joined by its mirrored twin")
    if not skip_mirrored_data:
        own = set(files)
        listed = [f for f in _list_hdf5(dataset_dir, False) if f not in own]
        if listed:
            raise ValueError(f"mirror_twins: {dataset_dir} already holds {len(listed)} mirrored episode files ({listed[0]}, ...): pass "
                             f"skip_mirrored_data (--skip_mirrored_data) to serve their twins from the originals instead")
    return mirror_twin_paths(files, spec, depth_follows, cloud_mirror)


def get_norm_stats(dataset_path_list):
    all_qpos, all_action, all_episode_len = [], [], []
    qpos = None
    for dataset_path in dataset_path_list:
        with open_episode(dataset_path) as root:
            qpos = np.asarray(root["/observations/qpos"][()])
            action = np.asarray(_read_action(root))
        all_qpos.append(torch.from_numpy(qpos))
        all_action.append(torch.from_numpy(action))
        all_episode_len.append(len(qpos))
    all_qpos = torch.cat(all_qpos, dim=0)
    all_action = torch.cat(all_action, dim=0)
    action_mean = all_action.mean(dim=[0]).float()
    action_std = torch.clip(all_action.std(dim=[0]).float(), 1e-2, np.inf)
    qpos_mean = all_qpos.mean(dim=[0]).float()
    qpos_std = torch.clip(all_qpos.std(dim=[0]).float(), 1e-2, np.inf)
    action_min = all_action.min(dim=0).values.float()
    action_max = all_action.max(dim=0).values.float()
    eps = 0.0001
    stats = {"action_mean": action_mean.numpy(), "action_std": action_std.numpy(),
             "action_min": action_min.numpy() - eps, "action_max": action_max.numpy() + eps,
             "qpos_mean": qpos_mean.numpy(), "qpos_std": qpos_std.numpy(), "example_qpos": qpos}
    return stats, all_episode_len


def BatchSampler(batch_size, episode_len_l, sample_weights, rng=None):
    """utils.py:237-247; ``rng`` (a ``numpy.random.Generator`` or the ``numpy.random`` module) makes it reproducible."""
    rng = rng or np.random
    sample_probs = np.array(sample_weights) / np.sum(sample_weights) if sample_weights is not None else None
    sum_dataset_len_l = np.cumsum([0] + [np.sum(episode_len) for episode_len in episode_len_l])
    randint = rng.integers if hasattr(rng, "integers") else rng.randint
    while True:
        batch = []
        for _ in range(batch_size):
            episode_idx = rng.choice(len(episode_len_l), p=sample_probs)
            batch.append(int(randint(sum_dataset_len_l[episode_idx], sum_dataset_len_l[episode_idx + 1])))
        yield batch


# ---------------------------------------------------------------------------------------------------------------------
# dataset
# ---------------------------------------------------------------------------------------------------------------------
class EpisodicDataset(torch.utils.data.Dataset):
    """utils.py:41-174.  ``__getitem__`` returns (image, qpos, action, is_pad); image is u8 ``[C,H,W,3]`` unless
    ``f32_images``.  With ``use_depth`` (the fork's depth dataset) a fifth entry follows: the frames of ``depth_camera_names``,
    raw uint16 ``[Cd,1,H,W]`` when the episode stores an unsigned integer of at most 16 bits, else (or with ``f32_depth``)
    float32 normalised by the sample's own minimum and maximum over all depth cameras.  With ``use_pcd`` (the fork's point-cloud
    dataset, utils_arm_gripper_all.py:90-99, 153-156) three entries follow the first four instead: xyz ``[N, 3]`` and rgb ``[N, 3]``
    float32 (colours stay 0..255) of the one cloud in ``pointcloud_names``, every stored row of it, and the int64 scalar ``n``, the
    number of rows that are points (the stored ``padding_mask``'s count, or N without a mask or with ``pcd_ignore_mask``); batch
    such samples with ``collate_pcd``."""

    def __init__(self, dataset_path_list, camera_names, norm_stats, episode_ids, episode_len, chunk_size, policy_class,
                 f32_images=False, depth_camera_names=None, use_depth=False, f32_depth=False, pointcloud_names=None, use_pcd=False,
                 max_points=None, pcd_ignore_mask=False):
        self.episode_ids = episode_ids
        self.dataset_path_list = dataset_path_list
        self.camera_names = camera_names
        self.norm_stats = norm_stats
        self.episode_len = episode_len
        self.chunk_size = chunk_size
        self.cumulative_len = np.cumsum(self.episode_len)
        self.max_episode_len = max(episode_len)
        self.policy_class = policy_class
        self.f32_images = f32_images
        self.use_depth = bool(use_depth)
        self.depth_camera_names = list(depth_camera_names) if depth_camera_names else []
        self.f32_depth = f32_depth
        if self.use_depth and not self.depth_camera_names:
            raise ValueError("use_depth needs depth_camera_names (the task config's list of /observations/depth_images/<cam>)")
        self.use_pcd = bool(use_pcd)
        self.pointcloud_names = list(pointcloud_names) if pointcloud_names else []
        self.max_points = None if max_points is None else int(max_points)
        self.pcd_ignore_mask = bool(pcd_ignore_mask)
        if self.use_pcd:
            if len(self.pointcloud_names) != 1:
                # the fork's training step takes the one fused cloud (train_single_arm_gripper_all.py:576-591)
                raise ValueError(f"use_pcd needs exactly one pointcloud name (/observations/pointcloud/<name>), got "
                                 f"{self.pointcloud_names}")
            if self.use_depth:
                raise NotImplementedError("use_depth together with use_pcd is not supported")
            if any(isinstance(p, MirrorTwinPath) and getattr(p, "cloud_mirror", None) is None for p in dataset_path_list):
                raise ValueError("use_pcd with mirror twins: a stored point cloud has no mirror rule (MirrorTwinPath(..., "
                                 "cloud_mirror=(axis, offset)) gives it one)")
        if policy_class == "Diffusion":
            raise NotImplementedError("the Diffusion augmentations (torchvision transforms) are outside this path")
        self._stats_t = {k: torch.as_tensor(np.asarray(norm_stats[k]), dtype=torch.float32)
                         for k in ("action_mean", "action_std", "qpos_mean", "qpos_std")}
        self.is_sim = False          # utils.py:59 (the reference overwrites what __getitem__ observed)

    def __len__(self):
        return int(self.cumulative_len[-1])

    def _locate_transition(self, index):
        assert index < self.cumulative_len[-1]
        episode_index = int(np.argmax(self.cumulative_len > index))       # first True
        start_ts = int(index - (self.cumulative_len[episode_index] - self.episode_len[episode_index]))
        return self.episode_ids[episode_index], start_ts

    def __getitem__(self, index):
        episode_id, start_ts = self._locate_transition(index)
        dataset_path = self.dataset_path_list[episode_id]
        with open_episode(dataset_path) as root:
            attrs = root.attrs
            is_sim = bool(attrs["sim"]) if "sim" in attrs else False         # legacy data lacks the attribute
            compressed = bool(attrs.get("compress", False))
            action = np.asarray(_read_action(root))
            original_action_shape = action.shape
            episode_len = original_action_shape[0]
            qpos = np.asarray(root["/observations/qpos"][start_ts])
            images = [np.asarray(root[f"/observations/images/{cam}"][start_ts]) for cam in self.camera_names]
            depths = [np.asarray(root[f"/observations/depth_images/{cam}"][start_ts]) for cam in self.depth_camera_names] \
                if self.use_depth else None
            cloud = self._read_cloud(root, start_ts, dataset_path) if self.use_pcd else None
        if compressed:                                            # utils.py:104-107
            images = [imdecode_bgr(buf) for buf in images]
            if depths is not None:                                # three equal channels of an 8-bit decode; channel 0 is kept below
                depths = [imdecode_bgr(buf) for buf in depths]
        if is_sim:
            action = action[start_ts:]
            action_len = episode_len - start_ts
        else:                                                     # "hack, to make timesteps more aligned" (utils.py:112-114)
            action = action[max(0, start_ts - 1):]
            action_len = episode_len - max(0, start_ts - 1)
        padded_action = np.zeros((self.max_episode_len, original_action_shape[1]), dtype=np.float32)
        padded_action[:action_len] = action
        is_pad = np.zeros(self.max_episode_len)
        is_pad[action_len:] = 1
        padded_action = padded_action[:self.chunk_size]
        is_pad = is_pad[:self.chunk_size]
        image_data = torch.from_numpy(np.stack(images, axis=0))                # [C,H,W,3] u8
        qpos_data = torch.from_numpy(qpos).float()
        action_data = torch.from_numpy(padded_action).float()
        is_pad = torch.from_numpy(is_pad).bool()
        if self.f32_images:
            image_data = torch.einsum("k h w c -> k c h w", image_data) / 255.0
        t = self._stats_t
        action_data = (action_data - t["action_mean"]) / t["action_std"]
        qpos_data = (qpos_data - t["qpos_mean"]) / t["qpos_std"]
        if depths is not None:
            return image_data, qpos_data, action_data, is_pad, self._depth_data(depths)
        if cloud is not None:
            return (image_data, qpos_data, action_data, is_pad) + cloud
        return image_data, qpos_data, action_data, is_pad

    def _read_cloud(self, root, start_ts, dataset_path):
        """the cloud of one sample: (xyz [N, 3] f32, rgb [N, 3] f32, n) -- every stored row, and how many of them are points"""
        base = f"/observations/pointcloud/{self.pointcloud_names[0]}"
        xyz = np.asarray(root[f"{base}/xyz"][start_ts])
        rgb = np.asarray(root[f"{base}/rgb"][start_ts])
        where = f"{dataset_path} (timestep {start_ts})"
        if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
            raise ValueError(f"{where}: point cloud xyz {xyz.shape} / rgb {rgb.shape}, expected two [N, 3] arrays")
        N = xyz.shape[0]
        n = N
        if not self.pcd_ignore_mask and f"{base}/padding_mask" in root:
            mask = np.asarray(root[f"{base}/padding_mask"][start_ts]).astype(bool).reshape(-1)
            if mask.shape[0] != N:
                raise ValueError(f"{where}: padding_mask of {mask.shape[0]} rows for a cloud of {N}")
            n = int(mask.sum())
            if not mask[:n].all():                                 # the recorder writes the points first, then the zero rows
                raise ValueError(f"{where}: padding_mask is not a prefix (True rows first): the valid points cannot be given as a count")
        if n == 0:
            raise ValueError(f"{where}: the point cloud has no valid point")
        if self.max_points is not None and N > self.max_points:
            raise ValueError(f"{where}: the point cloud stores {N} rows, more than max_points {self.max_points} (no silent truncation: "
                             "raise --max_points or down-sample the recording)")
        return (torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)),       # .float(), utils_arm_gripper_all.py:153-156
                torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.float32)), torch.tensor(n, dtype=torch.int64))

    def _depth_data(self, depths):
        """the depth frames of one sample -> [Cd, 1, H, W]: a 3-D frame keeps channel 0; raw uint16 for the device-side
        normalisation, or the reference's float32 (d - min) / (max - min + 1e-6) over all depth cameras of the sample"""
        d = np.stack([f[:, :, 0] if f.ndim == 3 else f for f in depths], axis=0)[:, None]
        if not self.f32_depth and d.dtype.kind == "u" and d.dtype.itemsize <= 2:
            return torch.from_numpy(np.ascontiguousarray(d, dtype=np.uint16))
        d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))        # torch.from_numpy(...).float(), utils_arm_gripper_all.py:147
        return (d - d.min()) / (d.max() - d.min() + 1e-6)


def collate_pcd(samples):
    """Batches the 7-entry samples of a ``use_pcd`` dataset: the first four entries as the default collation does, the clouds padded
    with ZERO rows to the batch's largest stored row count P (episodes differ in theirs) -> (image, qpos, action, is_pad,
    pcd_xyz [B, P, 3] f32, pcd_rgb [B, P, 3] f32, pcd_n [B] int32)."""
    from torch.utils.data import default_collate
    head = default_collate([s[:4] for s in samples])
    B, P = len(samples), max(int(s[4].shape[0]) for s in samples)
    xyz, rgb = torch.zeros((B, P, 3), dtype=torch.float32), torch.zeros((B, P, 3), dtype=torch.float32)
    for b, s in enumerate(samples):
        xyz[b, :s[4].shape[0]] = s[4]
        rgb[b, :s[5].shape[0]] = s[5]
    n = torch.tensor([int(s[6]) for s in samples], dtype=torch.int32)
    return tuple(head) + (xyz, rgb, n)


class _EpisodeArrays:
    """an open episode whose entries are fetched once: an ``.npz`` member is decompressed whole on every access, an HDF5 entry
    is a handle that reads what is sliced"""

    def __init__(self, root):
        self.root, self.attrs, self._got = root, root.attrs, {}

    def __contains__(self, key):
        return key in self.root

    def __getitem__(self, key):
        if key not in self._got:
            self._got[key] = self.root[key]
        return self._got[key]


class EpisodeReplay:
    """One recorded episode in time order, for open-loop replay: iterating gives batches of ``batch`` consecutive replayed steps
    (the last one ragged) in the layout the policy's inference call takes, the tensors of ``EpisodicDataset.__getitem__`` for the
    same steps without the action chunk: ``(image u8 [b, K, H, W, 3], qpos f32 [b, S] z-scored)``, then with ``use_depth`` the
    depth frames ``[b, Cd, 1, H, W]`` (raw uint16 where the episode stores them so), or with ``use_pcd`` ``(xyz [b, N, 3] f32,
    rgb [b, N, 3] f32, n [b] int32)`` through ``_read_cloud``'s rules.  Compressed episodes are decoded with ``imdecode_bgr``.
    Nothing is augmented.  ``stride``: only the steps 0, stride, 2 * stride, ... are replayed (a policy without temporal
    ensembling is queried once per chunk).  ``batch`` is the caller's: the clouds of a 4096-point batch of 50 are 16 MB.

    ``.actions`` [T, A] f32 in file units (with ``/base_action`` appended as the dataset does), ``.is_sim``, ``.T``, ``.steps``."""

    def __init__(self, dataset_path, camera_names, norm_stats, batch, depth_camera_names=None, use_depth=False, f32_depth=False,
                 pointcloud_names=None, use_pcd=False, max_points=None, pcd_ignore_mask=False, stride=1):
        self.dataset_path, self.batch, self.stride = dataset_path, int(batch), int(stride)
        if self.batch < 1 or self.stride < 1:
            raise ValueError(f"batch {batch} and stride {stride} must be at least 1")
        with open_episode(dataset_path) as root:
            attrs = root.attrs
            self.is_sim = bool(attrs["sim"]) if "sim" in attrs else False
            self.compressed = bool(attrs.get("compress", False))
            self.actions = np.ascontiguousarray(_read_action(root), dtype=np.float32)
        self.T = int(self.actions.shape[0])
        self.steps = list(range(0, self.T, self.stride))
        # the switches, their checks and the per-sample depth / cloud rules are the dataset's
        self._ds = EpisodicDataset([dataset_path], camera_names, norm_stats, [0], [self.T], 1, "ACT", False, depth_camera_names,
                                   use_depth, f32_depth, pointcloud_names, use_pcd, max_points, pcd_ignore_mask)

    def __len__(self):
        return (len(self.steps) + self.batch - 1) // self.batch

    def __iter__(self):
        ds = self._ds
        t = ds._stats_t
        with open_episode(self.dataset_path) as raw:
            root = _EpisodeArrays(raw)
            for b0 in range(0, len(self.steps), self.batch):
                steps = self.steps[b0:b0 + self.batch]
                sel = slice(steps[0], steps[-1] + 1) if self.stride == 1 else steps
                qpos = torch.from_numpy(np.asarray(root["/observations/qpos"][sel])).float()
                frames = [np.asarray(root[f"/observations/images/{cam}"][sel]) for cam in ds.camera_names]
                if self.compressed:                            # utils.py:104-107, frame by frame
                    frames = [np.stack([imdecode_bgr(buf) for buf in f]) for f in frames]
                out = [torch.from_numpy(np.stack(frames, axis=1)), (qpos - t["qpos_mean"]) / t["qpos_std"]]
                if ds.use_depth:
                    depths = [np.asarray(root[f"/observations/depth_images/{cam}"][sel]) for cam in ds.depth_camera_names]
                    if self.compressed:
                        depths = [np.stack([imdecode_bgr(buf) for buf in d]) for d in depths]
                    out.append(torch.stack([ds._depth_data([d[i] for d in depths]) for i in range(len(steps))]))
                if ds.use_pcd:
                    clouds = [ds._read_cloud(root, ts, self.dataset_path) for ts in steps]
                    out += [torch.stack([c[0] for c in clouds]), torch.stack([c[1] for c in clouds]),
                            torch.tensor([int(c[2]) for c in clouds], dtype=torch.int32)]
                yield tuple(out)


def flatten_list(l):
    return [item for sublist in l for item in sublist]


def load_data(dataset_dir_l, name_filter, camera_names, batch_size_train, batch_size_val, chunk_size,
              skip_mirrored_data=False, load_pretrain=False, policy_class=None, stats_dir_l=None, sample_weights=None,
              train_ratio=0.99, num_workers=2, f32_images=False, rng=None, depth_camera_names=None, use_depth=False,
              f32_depth=False, pointcloud_names=None, use_pcd=False, max_points=None, pcd_ignore_mask=False,
              device_dataset=False, device=None, device_budget_bytes=None, mirror_twins=False, mirror_spec=None,
              device_clouds=False, cloud_mirror=None, device_decode=False):
    """utils.py:249-301.  Returns (train_dataloader, val_dataloader, norm_stats, is_sim).  ``use_depth``: the batches are
    5-tuples that end in the depth frames of ``depth_camera_names`` (EpisodicDataset).  ``use_pcd``: 7-tuples that end in the
    padded clouds and their valid counts (collate_pcd).  ``device_dataset``: both loaders come from ONE ``DeviceEpisodeStore``
    on ``device`` (default: the current cuda device) that holds the train and validation episodes; the split, the norm stats
    and the samplers are built as without the flag, so the same ``rng`` gives the same episodes and the same draws, and the
    batches are the same tensors, already on the device (``loader.on_device``).  ``mirror_twins``: every episode file is joined by
    its mirrored twin (``MirrorTwinPath``; ``mirror_spec`` None: the reference's rule for the cameras each file holds), computed
    from the file as it is read -- the results are those of the same call without the flag on a directory in which the twin files
    exist (uncompressed, float32 rows): the same episode ids, stats, draws and batches.  With ``device_dataset`` the twins take no
    frame memory.  ``cloud_mirror`` ``(axis, offset)``: the mirror rule of the stored clouds (``cloud_mirror_rule``), which
    ``mirror_twins`` with ``use_pcd`` needs.  ``device_clouds``: the stored clouds of a ``use_pcd`` dataset go into the store as well
    and the device loaders deliver the 7-tuples of ``collate_pcd``, gathered by ``actmi_op_gather_clouds``.  ``device_decode``: the store
    decodes the frames of compressed episodes on the device (``DeviceEpisodeStore``); the batches are the same bytes."""
    if device_decode and not device_dataset:
        raise ValueError("device_decode decodes the compressed frames of the device-resident store: it needs device_dataset")
    if mirror_twins and use_pcd and cloud_mirror is None:
        raise ValueError("mirror_twins with use_pcd: a stored point cloud has no mirror rule (cloud_mirror=(axis, offset) gives it one)")
    if cloud_mirror is not None:
        if not (mirror_twins and use_pcd):
            raise ValueError("cloud_mirror is the mirror rule of the stored clouds of mirror_twins with use_pcd")
        cloud_mirror = cloud_mirror_rule(cloud_mirror)[:2]
    if device_clouds and not (device_dataset and use_pcd):
        raise ValueError("device_clouds puts the stored clouds of a use_pcd dataset into the device-resident store: it needs "
                         "device_dataset and use_pcd")
    if device_dataset:                                            # refused before any file is read
        if use_pcd and not device_clouds:
            raise NotImplementedError("--device_dataset with use_pcd: point clouds through the device-resident store are not "
                                      "implemented (ragged clouds stay on the host loader); drop --device_dataset")
        if policy_class not in (None, "ACT"):
            raise NotImplementedError(f"--device_dataset: the device-resident store feeds the ACT training path, not {policy_class!r}")
        if f32_images or f32_depth:
            raise NotImplementedError("--device_dataset keeps raw u8 frames and raw uint16 depth: f32_images / f32_depth belong to "
                                      "the host loader")
    rng = rng or np.random
    if isinstance(dataset_dir_l, str):
        dataset_dir_l = [dataset_dir_l]
    if mirror_twins:
        # depth camera i shares the swap and the flip of RGB camera i (the config demands one depth camera per RGB camera)
        follows = dict(zip(depth_camera_names or [], camera_names)) if use_depth else None

        def list_files(d):
            return find_all_hdf5_with_twins(d, skip_mirrored_data, mirror_spec, follows, cloud_mirror)
    else:
        def list_files(d):
            return find_all_hdf5(d, skip_mirrored_data)
    dataset_path_list_list = [list_files(d) for d in dataset_dir_l]
    num_episodes_0 = len(dataset_path_list_list[0])
    dataset_path_list = [n for n in flatten_list(dataset_path_list_list) if name_filter(n)]
    num_episodes_l = [len(l) for l in dataset_path_list_list]
    num_episodes_cumsum = np.cumsum(num_episodes_l)
    shuffled_episode_ids_0 = rng.permutation(num_episodes_0)
    train_episode_ids_0 = shuffled_episode_ids_0[:int(train_ratio * num_episodes_0)]
    val_episode_ids_0 = shuffled_episode_ids_0[int(train_ratio * num_episodes_0):]
    train_episode_ids_l = [train_episode_ids_0] + [np.arange(n) + num_episodes_cumsum[idx]
                                                   for idx, n in enumerate(num_episodes_l[1:])]
    val_episode_ids_l = [val_episode_ids_0]
    train_episode_ids = np.concatenate(train_episode_ids_l)
    val_episode_ids = np.concatenate(val_episode_ids_l)
    print(f"\n\nData from: {dataset_dir_l}\n- Train on {[len(x) for x in train_episode_ids_l]} episodes\n"
          f"- Test on {[len(x) for x in val_episode_ids_l]} episodes\n\n")
    _, all_episode_len = get_norm_stats(dataset_path_list)
    train_episode_len_l = [[all_episode_len[i] for i in ids] for ids in train_episode_ids_l]
    val_episode_len_l = [[all_episode_len[i] for i in ids] for ids in val_episode_ids_l]
    train_episode_len = flatten_list(train_episode_len_l)
    val_episode_len = flatten_list(val_episode_len_l)
    if stats_dir_l is None:
        stats_dir_l = dataset_dir_l
    elif isinstance(stats_dir_l, str):
        stats_dir_l = [stats_dir_l]
    norm_stats, _ = get_norm_stats(flatten_list([list_files(d) for d in stats_dir_l]))
    print(f"Norm stats from: {stats_dir_l}")
    pcd_kw = dict(pointcloud_names=pointcloud_names, use_pcd=use_pcd, max_points=max_points, pcd_ignore_mask=pcd_ignore_mask)
    train_dataset = EpisodicDataset(dataset_path_list, camera_names, norm_stats, train_episode_ids, train_episode_len,
                                    chunk_size, policy_class, f32_images, depth_camera_names, use_depth, f32_depth, **pcd_kw)
    val_dataset = EpisodicDataset(dataset_path_list, camera_names, norm_stats, val_episode_ids, val_episode_len,
                                  chunk_size, policy_class, f32_images, depth_camera_names, use_depth, f32_depth, **pcd_kw)
    if device_dataset:
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        store = DeviceEpisodeStore(dataset_path_list, np.concatenate([train_episode_ids, val_episode_ids]), camera_names, norm_stats,
                                   device, depth_camera_names, use_depth, device_budget_bytes, use_pcd, policy_class,
                                   device_decode=device_decode,
                                   **(dict(pointcloud_names=pointcloud_names, max_points=max_points, pcd_ignore_mask=pcd_ignore_mask)
                                      if device_clouds else {}))
        train_loader = store.loader(train_episode_ids, train_episode_len, chunk_size,
                                    BatchSampler(batch_size_train, train_episode_len_l, sample_weights, rng))
        val_loader = store.loader(val_episode_ids, val_episode_len, chunk_size, BatchSampler(batch_size_val, val_episode_len_l, None, rng))
        return train_loader, val_loader, norm_stats, train_dataset.is_sim
    from torch.utils.data import DataLoader
    kw = dict(pin_memory=torch.cuda.is_available(), num_workers=num_workers)
    if num_workers > 0:
        kw["prefetch_factor"] = 2
    if use_pcd:
        kw["collate_fn"] = collate_pcd
    train_dataloader = DataLoader(train_dataset, batch_sampler=BatchSampler(batch_size_train, train_episode_len_l,
                                                                             sample_weights, rng), **kw)
    val_dataloader = DataLoader(val_dataset, batch_sampler=BatchSampler(batch_size_val, val_episode_len_l, None, rng), **kw)
    return train_dataloader, val_dataloader, norm_stats, train_dataset.is_sim


# ---------------------------------------------------------------------------------------------------------------------
# host -> device hand-off
# ---------------------------------------------------------------------------------------------------------------------
class DevicePrefetcher:
    """Wraps an iterable of host batches (tuples of tensors): batch i+1 is copied to the device on a side stream
    (from pinned memory, ``non_blocking``) while the caller computes on batch i; ``__next__`` makes the compute stream
    wait for the copy it is about to use.  On a CPU-only host it degrades to the plain iterable (tests)."""

    def __init__(self, iterable, device=None, depth=2):
        self.it = iter(iterable)
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        self.cuda = self.device is not None and self.device.type == "cuda"
        self.stream = torch.cuda.Stream(self.device) if self.cuda else None
        self.queue = []
        self.depth = max(1, int(depth))
        for _ in range(self.depth):
            self._push()

    def _push(self):
        try:
            batch = next(self.it)
        except StopIteration:
            return
        if not self.cuda:
            self.queue.append((batch, None))
            return
        with torch.cuda.stream(self.stream):
            staged = tuple(t if t.is_pinned() else t.pin_memory() for t in batch)
            dev = tuple(t.to(self.device, non_blocking=True) for t in staged)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.queue.append((dev, ev))

    def __iter__(self):
        return self

    def __next__(self):
        if not self.queue:
            raise StopIteration
        batch, ev = self.queue.pop(0)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
            for t in batch:
                t.record_stream(torch.cuda.current_stream(self.device))
        self._push()
        return batch


# ---------------------------------------------------------------------------------------------------------------------
# device-resident episode store (load_data(..., device_dataset=True); DESIGN.md "Device-resident episode store")
# ---------------------------------------------------------------------------------------------------------------------
ARENA_ALIGN = 256            # every block of the frame arena (one camera of one episode) starts at a multiple of this
# Device memory the default budget leaves free: the training handle is created AFTER the loaders (imitate_episodes.main), and
# with it come the batches, the augmenter's buffers and the allocator's cache.  Measured at B = 64, 4 cameras of 480x640: the
# free memory drops by 51.5 GB (48 GiB) between the loaded store and the running training step
# (profiles/device_dataset_time.json, memory_beside_the_store_bytes); 64 GiB leaves a third on top.  Pass budget_bytes /
# --device_dataset_gb to decide otherwise (a larger batch needs a larger reserve).
DEVICE_STORE_RESERVE_BYTES = 64 << 30


def arena_layout(block_bytes, align=ARENA_ALIGN):
    """Blocks of ``block_bytes[i]`` bytes back to back, every start padded to ``align`` -> (int64 offsets, total bytes).  Frame t of
    block i lies at ``offsets[i] + t * frame_bytes``: a multiple of 16 whenever ``frame_bytes`` is one."""
    offs, total = np.zeros(len(block_bytes), dtype=np.int64), 0
    for i, n in enumerate(block_bytes):
        offs[i] = total
        total += (int(n) + align - 1) // align * align
    return offs, int(total)


def locate_transitions(indices, episode_len):
    """``EpisodicDataset._locate_transition`` for a batch of flat indices -> (position in ``episode_len`` [B], start_ts [B])"""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    lens = np.asarray(episode_len, dtype=np.int64)
    cum = np.cumsum(lens)
    if len(idx) and (idx.min() < 0 or idx.max() >= cum[-1]):
        raise IndexError(f"flat index outside [0, {int(cum[-1])})")
    ei = np.searchsorted(cum, idx, side="right")                  # the first episode whose cumulative length exceeds the index
    return ei, idx - (cum[ei] - lens[ei])


def _entry_meta(root, key):
    """(shape, dtype) of an episode entry without reading it where the format allows (an .npy header, an h5py handle)"""
    if hasattr(root, "meta"):
        return root.meta(key)
    d = root[key]
    return tuple(int(v) for v in d.shape), np.dtype(d.dtype)


def stored_cloud_counts(root, base, path, T, N, pcd_ignore_mask=False):
    """the valid count of every step of an episode's stored cloud ``base`` ([T, N, 3]) -> int32 [T], by ``_read_cloud``'s rules for
    all steps at once: ``padding_mask`` must be T x N with its True rows first and at least one of them per step (``ValueError``
    naming the file and the first offending timestep); without a mask, or with ``pcd_ignore_mask``, every stored row counts"""
    counts = np.full(T, N, dtype=np.int32)
    if not pcd_ignore_mask and f"{base}/padding_mask" in root:
        mask = np.asarray(root[f"{base}/padding_mask"][()]).astype(bool)
        if mask.shape[0] != T:
            raise ValueError(f"{path}: padding_mask of {mask.shape[0]} steps for an episode of {T}")
        mask = mask.reshape(T, -1)
        if mask.shape[1] != N:
            raise ValueError(f"{path} (timestep 0): padding_mask of {mask.shape[1]} rows for a cloud of {N}")
        counts = mask.sum(axis=1).astype(np.int32)
        bad = np.nonzero((mask != (np.arange(N)[None, :] < counts[:, None])).any(axis=1))[0]
        if len(bad):
            raise ValueError(f"{path} (timestep {int(bad[0])}): padding_mask is not a prefix (True rows first): the valid points "
                             "cannot be given as a count")
    empty = np.nonzero(counts == 0)[0]
    if len(empty):
        raise ValueError(f"{path} (timestep {int(empty[0])}): the point cloud has no valid point")
    return counts


class DeviceEpisodeStore:
    """Every frame of the named episodes in ONE device arena, read from the files once; a training batch is then a device-to-device
    gather (``actmi.ops.gather_frames`` / ``gather_chunks``) and equals what ``EpisodicDataset.__getitem__`` + the default
    collation give for the same flat indices, bit for bit and dtype for dtype.

    Arena: per episode (in ``episode_ids`` order, duplicates dropped), per camera of ``camera_names`` one u8 ``[T, H, W, 3]`` block,
    then with ``use_depth`` per depth camera one raw uint16 ``[T, H, W]`` block (channel 0 of 3-D frames, as ``_depth_data`` keeps);
    block starts padded to 256 bytes (``arena_layout``).  Compressed episodes are decoded once (``imdecode_bgr``).  The blocks reach
    the device through two bounded pinned staging buffers of ``stage_bytes``, never a pinned copy of an episode.  Actions and qpos
    (float32 as the dataset converts them, ``/base_action`` columns included), the episode table and the four stat vectors are
    small device arrays.

    Refused before anything large is allocated: ``use_pcd`` and a policy class other than ACT (``NotImplementedError``), depth that
    is not an unsigned integer of at most 16 bits, cameras or episodes whose frame sizes differ (``ValueError``), and a dataset
    larger than the budget (``MemoryError`` naming both numbers).  ``budget_bytes`` None: the device's free memory now minus
    ``DEVICE_STORE_RESERVE_BYTES``.  The sizes come from the entries' headers (the first episode's frame shape for a compressed
    dataset) and every block is checked against them again as it is loaded.

    Mirrored twins (``MirrorTwinPath`` entries of ``dataset_path_list``) add no frame bytes: ``sources`` are the files whose frames
    the arena holds, each once (a twin's source is loaded for its sake alone when it is not listed itself), a twin's camera blocks
    are its source's, permuted by its spec (``block_off``), with a flag per camera that is flipped (``flip`` / ``depth_flip``), and
    ``nbytes`` counts every source once.  A twin has its own rows in ``actions`` / ``qpos`` (the mirrored ones) and its own episode
    record.  A store that holds a twin gathers frames and depth with ``ops.gather_frames_mirror``; one without launches what it
    always did.  A twin whose source camera is not among ``camera_names`` is refused (``ValueError``).

    Stored point clouds (``use_pcd`` with exactly one name in ``pointcloud_names``; ``has_clouds``): per source file, behind its
    frame blocks, one float32 ``[T, N, 3]`` xyz block and one colour block ``[T, N, 3]`` -- uint8 when every source stores uint8,
    float32 everywhere otherwise (``cloud_rgb_fmt``) -- padded to 256 bytes like every block and counted in ``nbytes``; N may differ
    between episodes.  The valid count of every stored step (``_read_cloud``'s rules on ``padding_mask``, raised at load with the
    file and the timestep) is a host int32 array, ``cloud_n``.  ``gather`` then returns the 7-tuple of ``collate_pcd`` (P = the
    batch's largest stored row count) with ONE more launch, ``ops.gather_clouds``, whose item records ride in the batch's one index
    upload.  A twin's clouds are its source's blocks with the mirror flag set: no bytes; its ``cloud_mirror`` rule -- one for the
    whole store -- is the launch's.  ``use_pcd`` without names keeps the refusal above.

    ``device_decode``: the frames of a compressed source are decoded on the device (``ops.JpegDecoder``, actmi_op_jpeg_decode)
    instead of one by one through PIL: their headers are parsed on the host, the entropy segments go through the staging pair and
    the op writes straight into the block's place in the arena, B, G, R for cameras and the uint16 form for depth, up to
    ``decode_frames`` frames a launch.  A frame the parser refuses, one of another size and one whose status comes back nonzero
    (read once per source file) is decoded by ``imdecode_bgr`` and copied as without the flag, before the store is handed out: the
    flag changes neither what the arena holds nor which error a bad file raises.  ``decode_stats`` counts the frames of both
    kinds.  The decoder's workspace and stream buffer live only during the load.

    Every rank of a data-parallel run holds its own full store."""

    RING = 4                 # pinned index blocks in flight: a block is rewritten only after its copy has executed

    def __init__(self, dataset_path_list, episode_ids, camera_names, norm_stats, device, depth_camera_names=None, use_depth=False,
                 budget_bytes=None, use_pcd=False, policy_class="ACT", stage_bytes=64 << 20, pointcloud_names=None, max_points=None,
                 pcd_ignore_mask=False, device_decode=False, decode_frames=256):
        self.device_decode, self.decode_frames = bool(device_decode), int(decode_frames)
        self.pointcloud_names = list(pointcloud_names) if pointcloud_names else []
        self.has_clouds = bool(use_pcd) and bool(self.pointcloud_names)
        if self.has_clouds and len(self.pointcloud_names) != 1:
            raise ValueError(f"use_pcd needs exactly one pointcloud name (/observations/pointcloud/<name>), got {self.pointcloud_names}")
        if self.has_clouds and use_depth:
            raise NotImplementedError("use_depth together with use_pcd is not supported")
        self.max_points = None if max_points is None else int(max_points)
        self.pcd_ignore_mask = bool(pcd_ignore_mask)
        if use_pcd and not self.has_clouds:
            raise NotImplementedError("--device_dataset with use_pcd: point clouds through the device-resident store are not "
                                      "implemented (ragged clouds stay on the host loader); drop --device_dataset")
        if policy_class not in (None, "ACT"):
            raise NotImplementedError(f"--device_dataset: the device-resident store feeds the ACT training path, not {policy_class!r}")
        self.camera_names = list(camera_names)
        self.use_depth = bool(use_depth)
        self.depth_camera_names = list(depth_camera_names) if depth_camera_names else []
        if self.use_depth and not self.depth_camera_names:
            raise ValueError("use_depth needs depth_camera_names (the task config's list of /observations/depth_images/<cam>)")
        if not self.camera_names:
            raise ValueError("DeviceEpisodeStore: no camera names")
        self.episode_ids = list(dict.fromkeys(int(i) for i in episode_ids))
        if not self.episode_ids:
            raise ValueError("DeviceEpisodeStore: no episodes")
        self.paths = [dataset_path_list[i] for i in self.episode_ids]
        self._local_of = {e: i for i, e in enumerate(self.episode_ids)}
        # the files whose frames the arena holds, each once: an episode file is its own source, a mirrored twin's is the file it is
        # the image of (loaded for the twin's sake alone when it is not listed itself)
        self.twin = [isinstance(p, MirrorTwinPath) for p in self.paths]
        self.has_twins = any(self.twin)
        srcs = [p.source if tw else str(p) for p, tw in zip(self.paths, self.twin)]
        self.sources = list(dict.fromkeys(srcs))
        where = {s: j for j, s in enumerate(self.sources)}
        self._src_of = np.asarray([where[s] for s in srcs], dtype=np.int64)
        self.cloud_mirror = None                                      # (axis, offset, c2): the one rule of the twins' clouds
        if self.has_clouds and self.has_twins:
            rules = {getattr(p, "cloud_mirror", None) for p, tw in zip(self.paths, self.twin) if tw}
            if None in rules:
                raise ValueError("use_pcd with mirror twins: a stored point cloud has no mirror rule (MirrorTwinPath(..., "
                                 "cloud_mirror=(axis, offset)) gives it one)")
            if len(rules) != 1:
                raise ValueError(f"DeviceEpisodeStore: the twins carry different cloud mirror rules {sorted(rules)}: one gather takes one")
            self.cloud_mirror = cloud_mirror_rule(rules.pop())
        self.device = device
        self.stage_bytes = int(stage_bytes)
        self._plan()
        if budget_bytes is None:
            free, _total = torch.cuda.mem_get_info(torch.device(device))
            budget_bytes = free - DEVICE_STORE_RESERVE_BYTES
        self.budget_bytes = int(budget_bytes)
        if self.nbytes > self.budget_bytes:
            raise MemoryError(f"DeviceEpisodeStore: {len(self.paths)} episodes need {self.nbytes} bytes on the device "
                              f"({self.nbytes / 2**30:.2f} GiB), the budget is {self.budget_bytes} bytes "
                              f"({self.budget_bytes / 2**30:.2f} GiB): train without --device_dataset, or raise --device_dataset_gb")
        self._load(norm_stats)

    # ---- sizes, from the headers ---------------------------------------------------------------------------------
    def _plan(self):
        K, Kd = len(self.camera_names), len(self.depth_camera_names) if self.use_depth else 0
        src_T = np.zeros(len(self.sources), dtype=np.int64)
        self.frame_shape = self.depth_shape = None
        src_compressed = []
        src_N, rgb_u8 = np.zeros(len(self.sources), dtype=np.int64), True
        for i, path in enumerate(self.sources):
            with open_episode(path) as root:
                compressed = bool(root.attrs.get("compress", False))
                src_compressed.append(compressed)
                src_T[i] = _entry_meta(root, "/action")[0][0]
                if src_T[i] < 1:
                    raise ValueError(f"{path}: empty episode")
                if self.has_clouds:                                   # _read_cloud's checks of the shapes, from the headers
                    base = f"/observations/pointcloud/{self.pointcloud_names[0]}"
                    if f"{base}/xyz" not in root or f"{base}/rgb" not in root:
                        raise ValueError(f"{path}: no {base}/xyz and {base}/rgb")
                    (xs, _xdt), (cs, cdt) = _entry_meta(root, f"{base}/xyz"), _entry_meta(root, f"{base}/rgb")
                    if len(xs) != 3 or xs[2] != 3 or tuple(cs) != tuple(xs) or xs[1] < 1:
                        raise ValueError(f"{path}: point cloud xyz {tuple(xs)} / rgb {tuple(cs)}, expected two [T, N, 3] arrays")
                    if xs[0] != src_T[i]:
                        raise ValueError(f"{path}: {base}/xyz holds {xs[0]} clouds for an episode of {int(src_T[i])} steps")
                    if self.max_points is not None and xs[1] > self.max_points:
                        raise ValueError(f"{path}: the point cloud stores {xs[1]} rows, more than max_points {self.max_points} (no "
                                         "silent truncation: raise --max_points or down-sample the recording)")
                    src_N[i] = xs[1]
                    rgb_u8 = rgb_u8 and cdt == np.uint8
                for kind, cams, want in (("images", self.camera_names, 4), ("depth_images", self.depth_camera_names[:Kd], None)):
                    for cam in cams:
                        key = f"/observations/{kind}/{cam}"
                        shape, dtype = _entry_meta(root, key)
                        if shape[0] != src_T[i]:
                            raise ValueError(f"{path}: {key} holds {shape[0]} frames for an episode of {int(src_T[i])} steps")
                        if compressed:
                            if i > 0:
                                continue                           # sized by the first episode's frames; checked as it is decoded
                            fshape, dtype = imdecode_bgr(np.asarray(root[key][0])).shape, np.dtype(np.uint8)
                        else:
                            fshape = shape[1:]
                        if kind == "images":
                            if dtype != np.uint8 or len(fshape) != 3 or fshape[2] != 3:
                                raise ValueError(f"{path}: {key} frames are {dtype} {fshape}, expected uint8 [H, W, 3]")
                            fshape = tuple(fshape)
                            if self.frame_shape not in (None, fshape):
                                raise ValueError(f"{path}: {key} frames are {fshape}, others {self.frame_shape}: one batch shape only")
                            self.frame_shape = fshape
                        else:
                            if dtype.kind != "u" or dtype.itemsize > 2:
                                raise ValueError(f"{path}: {key} is {dtype}: the device-resident store keeps raw depth, an unsigned "
                                                 f"integer of at most 16 bits (float depth is normalised on the host: train "
                                                 f"without --device_dataset)")
                            if len(fshape) not in (2, 3):
                                raise ValueError(f"{path}: {key} frames are {fshape}, expected [H, W] or [H, W, C]")
                            fshape = tuple(fshape[:2])
                            if self.depth_shape not in (None, fshape):
                                raise ValueError(f"{path}: {key} frames are {fshape}, others {self.depth_shape}: one batch shape only")
                            self.depth_shape = fshape
        self.K, self.Kd = K, Kd
        self.frame_bytes = int(np.prod(self.frame_shape))
        self.depth_bytes = int(np.prod(self.depth_shape)) * 2 if Kd else 0
        nc = 2 if self.has_clouds else 0                               # an xyz and a colour block per source, behind its frames
        self.cloud_rgb_fmt = 0 if rgb_u8 else 1                        # uint8 colours when every source stores them, f32 otherwise
        self.cloud_rgb_bytes = 3 if rgb_u8 else 12                     # bytes of one stored colour row
        blocks = []
        for T, N in zip(src_T, src_N):
            blocks += [int(T) * self.frame_bytes] * K + [int(T) * self.depth_bytes] * Kd + \
                      [int(T) * int(N) * 12, int(T) * int(N) * self.cloud_rgb_bytes][:nc]
        offs, self.nbytes = arena_layout(blocks)                       # every source once: a twin adds no frame bytes
        ends = [int(o) + int(b) for o, b in zip(offs, blocks)]
        self._padding = [(e, int(n)) for e, n in zip(ends, list(offs[1:]) + [self.nbytes]) if n > e]   # the bytes no block holds
        offs = offs.reshape(len(self.sources), K + Kd + nc)
        self._src_block_off, self._src_depth_block_off, self._src_T = offs[:, :K].copy(), offs[:, K:K + Kd].copy(), src_T
        self._src_N, self._src_cloud_off = src_N, offs[:, K + Kd:].copy()
        self._src_row0 = np.concatenate([[0], np.cumsum(src_T)[:-1]]).astype(np.int64)   # of a source's steps in cloud_n
        self._src_compressed = src_compressed
        # per episode: its source's length and blocks; a twin's cameras are its source's, permuted and flagged by its spec
        self.T = src_T[self._src_of]
        self.compressed = [src_compressed[j] for j in self._src_of]
        self.block_off, self.depth_block_off = self._src_block_off[self._src_of], self._src_depth_block_off[self._src_of]
        self.flip, self.depth_flip = np.zeros(self.block_off.shape, dtype=np.uint8), np.zeros(self.depth_block_off.shape, dtype=np.uint8)
        for i, path in enumerate(self.paths):
            if not self.twin[i]:
                continue
            j = self._src_of[i]
            with open_episode(path) as view:
                for kind, cams, off, src_off, flip in (
                        ("images", self.camera_names, self.block_off, self._src_block_off, self.flip),
                        ("depth_images", self.depth_camera_names[:Kd], self.depth_block_off, self._src_depth_block_off, self.depth_flip)):
                    for k, cam in enumerate(cams):
                        found = view._resolve(f"/observations/{kind}/{cam}")
                        if found is None:
                            raise ValueError(f"{path}: the mirror twin holds no /observations/{kind}/{cam}")
                        src_cam = found[1].rsplit("/", 1)[1]
                        if src_cam not in cams:
                            raise ValueError(f"{path}: /observations/{kind}/{cam} of the twin is the source's {src_cam}, which is not "
                                             f"among the store's cameras {list(cams)}")
                        off[i, k], flip[i, k] = src_off[j, list(cams).index(src_cam)], 1 if found[2] else 0
        # the statement the gather's launcher cannot check for itself (actmi_op_gather_frames, `aligned`)
        self.aligned = 1 if self.frame_bytes % 16 == 0 else 0
        self.depth_aligned = 1 if Kd and self.depth_bytes % 16 == 0 else 0
        self.row0 = np.concatenate([[0], np.cumsum(self.T)[:-1]]).astype(np.int64)

    # ---- the one read of every episode ----------------------------------------------------------------------------
    def _load(self, norm_stats):
        from . import ops
        import time
        dev = torch.device(self.device)
        t_begin = time.perf_counter()
        self.arena = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        for a, b in self._padding:                                    # the padding between blocks is zero: two stores of one
            self.arena[a:b].zero_()                                   # dataset hold the same bytes everywhere
        stage = max(self.stage_bytes, self.frame_bytes, self.depth_bytes, int(self._src_N.max()) * 12 if self.has_clouds else 0)
        self.cloud_n = np.zeros(int(self._src_T.sum()) if self.has_clouds else 0, dtype=np.int32)   # valid rows of every stored step
        self._pin = [torch.empty(stage, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._pin_ev, self._pin_i = [None, None], 0
        self.decode_stats = {"device": 0, "host": 0}
        self.bus_bytes = 0                                            # bytes of frames and clouds that crossed to the device
        self._decoders, self._pending, self._jpeg_stream = {}, [], None
        if self.device_decode and any(self._src_compressed):
            self._jpeg_stream = torch.empty(stage, dtype=torch.uint8, device=dev)
        actions, qposes, sims = [], [], []
        loaded = set()
        for i, path in enumerate(self.paths):
            T = int(self.T[i])
            with open_episode(path) as raw:
                root = _EpisodeArrays(raw)                            # a twin: the view, whose rows are the mirrored ones
                attrs = root.attrs
                sims.append(bool(attrs["sim"]) if "sim" in attrs else False)
                action = np.asarray(_read_action(root))
                qpos = np.asarray(root["/observations/qpos"][()])
                if action.ndim != 2 or action.shape[0] != T or qpos.ndim != 2 or qpos.shape[0] != T:
                    raise ValueError(f"{path}: action {action.shape} / qpos {qpos.shape} for an episode of {T} steps")
                actions.append(action.astype(np.float32))            # padded_action is float32: the assignment converts
                qposes.append(torch.from_numpy(qpos).float().numpy())
                if not self.twin[i]:
                    self._load_source(root, int(self._src_of[i]))
                    loaded.add(int(self._src_of[i]))
        for j in range(len(self.sources)):                            # the sources only twins name
            if j not in loaded:
                with open_episode(self.sources[j]) as raw:
                    self._load_source(_EpisodeArrays(raw), j)
        A, S = actions[0].shape[1], qposes[0].shape[1]
        if any(a.shape[1] != A for a in actions) or any(q.shape[1] != S for q in qposes):
            raise ValueError("DeviceEpisodeStore: episodes differ in their action or qpos width")
        self.A, self.S = int(A), int(S)
        self.actions = torch.from_numpy(np.concatenate(actions, axis=0)).to(dev)
        self.qpos = torch.from_numpy(np.concatenate(qposes, axis=0)).to(dev)
        rec = np.zeros(len(self.paths), dtype=ops.episode_rec_dtype())
        rec["row0"], rec["T"], rec["is_sim"] = self.row0, self.T, np.asarray(sims, dtype=np.int32)
        self.is_sim = sims
        self.episodes = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.norm_stats = norm_stats                                  # as given: what a replay out of the store un-normalises with
        self._stats = [torch.as_tensor(np.asarray(norm_stats[k]), dtype=torch.float32).reshape(-1).contiguous().to(dev)
                       for k in ("action_mean", "action_std", "qpos_mean", "qpos_std")]
        if self._stats[0].numel() != self.A or self._stats[2].numel() != self.S:
            raise ValueError(f"DeviceEpisodeStore: norm stats of {self._stats[0].numel()} action / {self._stats[2].numel()} qpos "
                             f"values for episodes of {self.A} / {self.S}")
        torch.cuda.synchronize(dev)
        self._pin = self._pin_ev = None                               # the staging buffers are the load's alone
        self._decoders = self._jpeg_stream = None                     # and so are the decoder's workspace and stream buffer
        self.load_seconds = time.perf_counter() - t_begin
        self._host, self._host_ev, self._slot = [None] * self.RING, [None] * self.RING, 0

    def _load_source(self, root, j):
        """the frames of source file j, open as `root`, into its blocks of the arena"""
        path, T = self.sources[j], int(self._src_T[j])
        for k, cam in enumerate(self.camera_names):
            self._load_block(root[f"/observations/images/{cam}"], T, self._src_compressed[j], int(self._src_block_off[j, k]), False,
                             f"{path}: /observations/images/{cam}")
        for k, cam in enumerate(self.depth_camera_names[:self.Kd]):
            self._load_block(root[f"/observations/depth_images/{cam}"], T, self._src_compressed[j],
                             int(self._src_depth_block_off[j, k]), True, f"{path}: /observations/depth_images/{cam}")
        self._finish_device_decode()
        if self.has_clouds:
            self._load_clouds(root, j)

    def _load_clouds(self, root, j):
        """the clouds of source file j into its two blocks, and the valid count of every step by ``_read_cloud``'s rules"""
        path, T, N = self.sources[j], int(self._src_T[j]), int(self._src_N[j])
        base = f"/observations/pointcloud/{self.pointcloud_names[0]}"
        f32c = self.cloud_rgb_fmt == 1
        for leaf, off, rb in (("xyz", int(self._src_cloud_off[j, 0]), 12), ("rgb", int(self._src_cloud_off[j, 1]), self.cloud_rgb_bytes)):
            entry = root[f"{base}/{leaf}"]
            per = max(1, self._pin[0].numel() // (N * rb))
            for t0 in range(0, T, per):
                t1 = min(T, t0 + per)
                piece = np.asarray(entry[t0:t1])
                if piece.shape != (t1 - t0, N, 3):
                    raise ValueError(f"{path} (timestep {t0}): point cloud {leaf} {piece.shape[1:]}, the store was sized for {(N, 3)}")
                if leaf == "rgb" and not f32c:
                    if piece.dtype != np.uint8:
                        raise ValueError(f"{path}: {base}/rgb is {piece.dtype}, its header said uint8")
                    flat = np.ascontiguousarray(piece).reshape(-1)
                else:                                                 # np.ascontiguousarray(..., dtype=np.float32), as _read_cloud
                    flat = np.ascontiguousarray(piece, dtype=np.float32).reshape(-1).view(np.uint8)
                n = (t1 - t0) * N * rb
                if off + t0 * N * rb + n > self.nbytes:               # cannot happen with the sizes checked in _plan
                    raise MemoryError(f"{path}: cloud block leaves the arena of {self.nbytes} bytes")
                self._stage(off + t0 * N * rb, n, lambda view, flat=flat: np.copyto(view, flat))
        counts = stored_cloud_counts(root, base, path, T, N, self.pcd_ignore_mask)
        self.cloud_n[int(self._src_row0[j]):int(self._src_row0[j]) + T] = counts

    def _stage(self, dst_off, nbytes, fill, dst=None):
        """one piece through the staging pair: ``fill(view)`` writes `nbytes` bytes into the pinned view, which is then copied to
        the arena (or to `dst`, another device buffer); a buffer is refilled only after the copy that read it has executed"""
        dst = self.arena if dst is None else dst
        self.bus_bytes += int(nbytes)
        j = self._pin_i
        self._pin_i = 1 - j
        if self._pin_ev[j] is not None:
            self._pin_ev[j].synchronize()
        fill(self._pin[j].numpy()[:nbytes])
        dst[dst_off:dst_off + nbytes].copy_(self._pin[j][:nbytes], non_blocking=True)
        self._pin_ev[j] = torch.cuda.Event()
        self._pin_ev[j].record(torch.cuda.current_stream(self.arena.device))

    def _load_block(self, entry, T, compressed, dst_off, depth, where):
        fb = self.depth_bytes if depth else self.frame_bytes
        shape = self.depth_shape if depth else self.frame_shape
        per = max(1, self._pin[0].numel() // fb)
        for t0 in range(0, T, per):
            t1 = min(T, t0 + per)
            piece = np.asarray(entry[t0:t1])
            if compressed and self._jpeg_stream is not None and piece.ndim == 2 and piece.dtype == np.uint8:
                host = self._decode_on_device(piece, dst_off + t0 * fb, depth)
                for i in host:                                        # what the parser refused: as without the flag, frame by frame
                    self._load_host_frame(piece[i], dst_off + (t0 + i) * fb, depth, where)
                continue
            if compressed:                                            # utils.py:104-107, frame by frame
                piece = np.stack([imdecode_bgr(buf) for buf in piece])
            if depth:
                if piece.dtype.kind != "u" or piece.dtype.itemsize > 2:
                    raise ValueError(f"{where} is {piece.dtype}: not raw depth (an unsigned integer of at most 16 bits)")
                if piece.ndim == 4:
                    piece = piece[..., 0]                             # _depth_data: a 3-D frame keeps channel 0
                piece = piece.astype(np.uint16, copy=False)
            if piece.shape != (t1 - t0,) + tuple(shape) or (not depth and piece.dtype != np.uint8):
                raise ValueError(f"{where}: frames {piece.dtype} {piece.shape[1:]}, the store was sized for {tuple(shape)}")
            n = (t1 - t0) * fb
            if dst_off + t0 * fb + n > self.nbytes:                  # cannot happen with the sizes checked above
                raise MemoryError(f"{where}: block leaves the arena of {self.nbytes} bytes")
            flat = np.ascontiguousarray(piece).reshape(-1).view(np.uint8)
            self._stage(dst_off + t0 * fb, n, lambda view, flat=flat: np.copyto(view, flat))

    # ---- compressed frames decoded on the device (device_decode) -------------------------------------------------------
    def _load_host_frame(self, buf, dst_off, depth, where):
        """one compressed frame by the host path: ``_load_block``'s steps and refusals for a piece of one frame"""
        fb = self.depth_bytes if depth else self.frame_bytes
        shape = self.depth_shape if depth else self.frame_shape
        frame = imdecode_bgr(buf)
        if depth:
            frame = frame[..., 0].astype(np.uint16, copy=False)
        if frame.shape != tuple(shape):
            raise ValueError(f"{where}: frames {frame.dtype} {frame.shape}, the store was sized for {tuple(shape)}")
        flat = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
        self._stage(dst_off, fb, lambda view, flat=flat: np.copyto(view, flat))
        self.decode_stats["host"] += 1

    def _decode_on_device(self, piece, dst_off, depth):
        """the frames of `piece` ([n, L] u8, one zero-padded file each) that the parser accepts at the store's size: their entropy
        segments through the staging pair, decoded into arena[dst_off + i * frame bytes]; -> the indices of the other frames.  The
        statuses stay on the device until ``_finish_device_decode``."""
        from . import ops
        fb = self.depth_bytes if depth else self.frame_bytes
        H, W = (self.depth_shape if depth else self.frame_shape)[:2]
        dec = self._decoders.get((H, W))
        if dec is None:
            dec = self._decoders[(H, W)] = ops.JpegDecoder(self.device, H, W, max_frames=self.decode_frames)
        host, todo = [], {}
        for i, buf in enumerate(piece):
            try:
                info = dec.parse(buf)
            except ops.JpegUnsupported:
                host.append(i)
                continue
            if (info["H"], info["W"]) != (H, W):
                host.append(i)
                continue
            todo.setdefault(info["mode"], []).append((i, info))
        cap = int(self._jpeg_stream.numel())
        for mode, items in todo.items():
            k0 = 0
            while k0 < len(items):                                    # as many frames as the stream buffer and one launch hold
                k1, nbytes = k0, 0
                while k1 < len(items) and k1 - k0 < dec.max_frames and nbytes + items[k1][1]["seg_len"] <= cap:
                    nbytes += items[k1][1]["seg_len"]
                    k1 += 1
                if k1 == k0:                                          # one segment larger than the staging buffer
                    host.append(items[k0][0])
                    k0 += 1
                    continue
                part = items[k0:k1]
                frames = np.zeros(len(part), dtype=ops.jpeg_frame_dtype())
                lens = np.asarray([info["seg_len"] for _i, info in part], dtype=np.int64)
                frames["seg_len"], frames["seg_off"] = lens, np.concatenate([[0], np.cumsum(lens)[:-1]])
                frames["dst_off"] = [dst_off + i * fb for i, _info in part]
                frames["restart_interval"] = [info["restart_interval"] for _i, info in part]
                frames["table_set"] = [dec.table_index(info["tables"]) for _i, info in part]

                def fill(view, part=part, frames=frames):
                    for (i, info), o, n in zip(part, frames["seg_off"], frames["seg_len"]):
                        view[o:o + n] = piece[i][info["seg_off"]:info["seg_off"] + n]
                if nbytes:
                    self._stage(0, nbytes, fill, self._jpeg_stream)
                status = dec.decode(self._jpeg_stream, frames, mode, "u16" if depth else "bgr", self.arena)
                self._pending.append((status, [(piece[i], int(o)) for (i, _info), o in zip(part, frames["dst_off"])], depth))
                k0 = k1
        return sorted(host)

    def _finish_device_decode(self):
        """the statuses of a source file's launches, read back once; a frame whose status is not 0 takes the host path"""
        if not self._pending:
            return
        status = torch.cat([st for st, _frames, _depth in self._pending]).cpu().numpy()
        k = 0
        for _st, frames, depth in self._pending:
            for buf, off in frames:
                if status[k]:
                    self._load_host_frame(buf, off, depth, f"a frame at arena byte {off}")
                else:
                    self.decode_stats["device"] += 1
                k += 1
        self._pending = []

    # ---- batches --------------------------------------------------------------------------------------------------
    def device_bytes(self):
        """bytes of device memory the store holds"""
        return int(self.arena.numel() + self.actions.numel() * 4 + self.qpos.numel() * 4 + self.episodes.numel() +
                   sum(s.numel() * 4 for s in self._stats))

    def frame_offsets(self, local_episode, t):
        """byte offsets into the arena of the frames of samples (local_episode[b], t[b]) -> ([B, K], [B, Kd]) int64"""
        e, t = np.asarray(local_episode, dtype=np.int64), np.asarray(t, dtype=np.int64)
        return (self.block_off[e] + t[:, None] * self.frame_bytes,
                self.depth_block_off[e] + t[:, None] * self.depth_bytes)

    def _upload(self, table):
        """the int64 index table of one batch -> a device tensor, by a stream-ordered copy from a pinned block of a ring"""
        n = len(table)
        i = self._slot
        self._slot = (i + 1) % self.RING
        if self._host_ev[i] is not None:
            self._host_ev[i].synchronize()                             # the copy that last read this block has executed
        if self._host[i] is None or self._host[i].numel() < n:
            self._host[i] = torch.empty(max(n, 1024), dtype=torch.int64, pin_memory=True)
        self._host[i].numpy()[:n] = table
        dev = self.arena.device
        tab = torch.empty(n, dtype=torch.int64, device=dev)
        tab.copy_(self._host[i][:n], non_blocking=True)
        self._host_ev[i] = torch.cuda.Event()
        self._host_ev[i].record(torch.cuda.current_stream(dev))
        return tab

    def gather(self, local_episode, t, Q, nontemporal=True):
        """the batch of samples (local_episode[b], t[b]) with chunks of Q steps, on the current stream of the store's device:
        (image u8 [B, K, H, W, 3], qpos f32 [B, S], action f32 [B, Q, A], is_pad bool [B, Q][, depth uint16 [B, Kd, 1, H, W]]).
        ``nontemporal``: the 16-byte form reads the arena with non-temporal loads -- measured 0.77-0.87 of the plain loads' time at
        B = 64 and level with them at B = 8 (profiles/device_dataset_time.json); the bytes are the same either way"""
        from . import ops
        e, t = np.asarray(local_episode, dtype=np.int64).reshape(-1), np.asarray(t, dtype=np.int64).reshape(-1)
        B = len(e)
        if B < 1 or len(t) != B:
            raise ValueError(f"DeviceEpisodeStore.gather: {B} episodes, {len(t)} steps")
        if e.min() < 0 or e.max() >= len(self.paths) or t.min() < 0 or np.any(t >= self.T[e]):
            raise IndexError("DeviceEpisodeStore.gather: a sample outside the stored episodes")
        off, doff = self.frame_offsets(e, t)
        samples = np.ascontiguousarray(np.stack([e, t], axis=1).astype(np.int32)).view(np.int64).reshape(-1)
        items = self._cloud_items(e, t) if self.has_clouds else None
        if self.has_twins:
            return self._gather_mirror(e, off, doff, samples, B, Q, nontemporal, items)
        nk, nd = B * self.K, B * self.Kd
        dev = self.arena.device
        with torch.cuda.device(dev):
            if items is not None:                                     # the item records ride behind the samples in the one upload
                tab = self._upload(np.concatenate([off.reshape(-1), doff.reshape(-1), samples, items.view(np.int64)]))
                clouds = self._gather_clouds(tab[nk + nd + B:], items, nontemporal)
                tab = tab[:nk + nd + B]
            else:
                tab = self._upload(np.concatenate([off.reshape(-1), doff.reshape(-1), samples]))
            image = torch.empty((B, self.K) + tuple(self.frame_shape), dtype=torch.uint8, device=dev)
            ops.gather_frames(self.arena, tab[:nk], self.frame_bytes, out=image,
                              aligned=2 if (nontemporal and self.aligned) else self.aligned)
            qpos, action, is_pad = ops.gather_chunks(self.actions, self.qpos, self.episodes, tab[nk + nd:].view(torch.int32).view(B, 2),
                                                     *self._stats, Q)
            if items is not None:
                return (image, qpos, action, is_pad) + clouds
            if not self.Kd:
                return image, qpos, action, is_pad
            depth = torch.empty((B, self.Kd, 1) + tuple(self.depth_shape), dtype=torch.uint16, device=dev)
            ops.gather_frames(self.arena, tab[nk:nk + nd], self.depth_bytes, out=depth,
                              aligned=2 if (nontemporal and self.depth_aligned) else self.depth_aligned)
        return image, qpos, action, is_pad, depth

    def _cloud_items(self, e, t):
        """the records (``ops.cloud_item_dtype``) of the clouds of samples (e[b], t[b]): where the step's rows lie in its source's two
        blocks, how many there are, how many are points, and the mirror flag of a twin"""
        from . import ops
        j = self._src_of[e]
        N = self._src_N[j]
        items = np.zeros(len(e), dtype=ops.cloud_item_dtype())
        items["xyz_off"] = self._src_cloud_off[j, 0] + t * N * 12
        items["rgb_off"] = self._src_cloud_off[j, 1] + t * N * self.cloud_rgb_bytes
        items["rows"], items["n"] = N, self.cloud_n[self._src_row0[j] + t]
        items["flags"] = np.asarray(self.twin, dtype=np.int32)[e]
        return items

    def _gather_clouds(self, tab, items, nontemporal):
        """the one launch of a batch's clouds -> (xyz [B, P, 3] f32, rgb [B, P, 3] f32, n [B] int32), P the batch's largest stored
        row count as ``collate_pcd`` pads; the 16-byte form where P allows it (torch's allocations are 16-byte aligned)"""
        from . import ops
        P = int(items["rows"].max())
        aligned = (2 if nontemporal else 1) if P % 4 == 0 else 0
        mirror = None if self.cloud_mirror is None else (self.cloud_mirror[0], self.cloud_mirror[2])
        return ops.gather_clouds(self.arena, tab, P, self.cloud_rgb_fmt, mirror=mirror, aligned=aligned)

    def _gather_mirror(self, e, off, doff, samples, B, Q, nontemporal, items=None):
        """``gather`` of a store that holds mirrored twins: the frames (and the depth) come from ``gather_frames_mirror``, whose
        flip flags -- one per item, the twin's cameras that are flipped -- travel in the same index upload, packed eight to a word
        behind the offsets"""
        from . import ops
        nk, nd = B * self.K, B * self.Kd
        dev = self.arena.device
        flags = np.concatenate([self.flip[e].reshape(-1), self.depth_flip[e].reshape(-1)])
        words = np.zeros((len(flags) + 7) // 8 * 8, dtype=np.uint8)
        words[:len(flags)] = flags
        H, W = self.frame_shape[:2]
        # the aligned form's statement: frames at multiples of 16 (the arena's layout) and rows of whole 16- / 8-pixel groups
        aligned = self.aligned if W % 16 == 0 else 0
        with torch.cuda.device(dev):
            if items is not None:
                nw = len(words) // 8
                tab = self._upload(np.concatenate([off.reshape(-1), doff.reshape(-1), samples, words.view(np.int64), items.view(np.int64)]))
                clouds = self._gather_clouds(tab[nk + nd + B + nw:], items, nontemporal)
                tab = tab[:nk + nd + B + nw]
            else:
                tab = self._upload(np.concatenate([off.reshape(-1), doff.reshape(-1), samples, words.view(np.int64)]))
            fl = tab[nk + nd + B:].view(torch.uint8)
            image = torch.empty((B, self.K) + tuple(self.frame_shape), dtype=torch.uint8, device=dev)
            ops.gather_frames_mirror(self.arena, tab[:nk], fl[:nk], H, W, 3, out=image, aligned=2 if (nontemporal and aligned) else aligned)
            qpos, action, is_pad = ops.gather_chunks(self.actions, self.qpos, self.episodes, tab[nk + nd:nk + nd + B].view(torch.int32).view(B, 2),
                                                     *self._stats, Q)
            if items is not None:
                return (image, qpos, action, is_pad) + clouds
            if not self.Kd:
                return image, qpos, action, is_pad
            Hd, Wd = self.depth_shape
            aligned = self.depth_aligned if Wd % 8 == 0 else 0
            depth = torch.empty((B, self.Kd, 1) + tuple(self.depth_shape), dtype=torch.uint16, device=dev)
            ops.gather_frames_mirror(self.arena, tab[nk:nk + nd], fl[nk:nk + nd], Hd, Wd, 2, out=depth,
                                     aligned=2 if (nontemporal and aligned) else aligned)
        return image, qpos, action, is_pad, depth

    def replay_batch(self, local_episode, steps):
        """the steps ``steps`` of ONE stored episode in the layout the policy's inference call takes, on the current stream of
        the store's device: (image u8 [b, K, H, W, 3], qpos f32 [b, S] z-scored[, depth uint16 [b, Kd, 1, H, W]]) -- what
        ``EpisodeReplay`` yields for these steps, bit for bit.  The two gathers of ``gather`` serve it (the qpos rows come from
        ``gather_chunks`` with a chunk of one step, which is dropped)."""
        steps = np.asarray(steps, dtype=np.int64).reshape(-1)
        if len(steps) * max(self.K, self.Kd) > 65535:
            raise ValueError(f"DeviceEpisodeStore.replay_batch: {len(steps)} steps of {max(self.K, self.Kd)} cameras are more than "
                             "the 65535 items of one frame gather")
        out = self.gather(np.full(len(steps), int(local_episode), dtype=np.int64), steps, 1)
        return (out[0], out[1]) + tuple(out[4:])

    def loader(self, episode_ids, episode_len, chunk_size, batch_sampler):
        return DeviceBatchLoader(self, episode_ids, episode_len, chunk_size, batch_sampler)


class DeviceEpisodeReplay:
    """``EpisodeReplay`` out of a ``DeviceEpisodeStore``: one stored episode (``episode_id`` as the store was given it) in time
    order, ``batch`` replayed steps at a time (the last batch ragged), only every ``stride``-th step.  The same iterable with the
    same attributes -- ``.T``, ``.steps``, ``.is_sim``, ``.actions`` (host [T, A] f32 in file units, copied from the device when
    first asked for), ``__len__`` -- and the tensors it yields are bit for bit those ``EpisodeReplay`` yields for the same file,
    batch and stride, but already on the device (``on_device``): no file is opened and nothing is pinned or copied from the host.
    ``.actions_device``: the episode's action rows [T, A] f32, a view of the store's."""

    on_device = True

    def __init__(self, store, episode_id, batch, stride=1):
        self.store, self.batch, self.stride = store, int(batch), int(stride)
        if self.batch < 1 or self.stride < 1:
            raise ValueError(f"batch {batch} and stride {stride} must be at least 1")
        if int(episode_id) not in store._local_of:
            raise ValueError(f"DeviceEpisodeReplay: episode {episode_id} is not in the store (it holds {store.episode_ids})")
        cams = max(store.K, store.Kd)
        if self.batch * cams > 65535:
            raise ValueError(f"DeviceEpisodeReplay: a batch of {self.batch} steps of {cams} cameras is more than the 65535 items of "
                             f"one frame gather: at most {65535 // cams}")
        self.episode_id = int(episode_id)
        self.local = store._local_of[self.episode_id]
        self.dataset_path = store.paths[self.local]
        self.T = int(store.T[self.local])
        self.is_sim = bool(store.is_sim[self.local])
        self.steps = list(range(0, self.T, self.stride))
        row0 = int(store.row0[self.local])
        self.actions_device = store.actions[row0:row0 + self.T]
        self._actions = None

    @property
    def actions(self):
        if self._actions is None:
            self._actions = np.ascontiguousarray(self.actions_device.cpu().numpy(), dtype=np.float32)
        return self._actions

    def __len__(self):
        return (len(self.steps) + self.batch - 1) // self.batch

    def __iter__(self):
        for b0 in range(0, len(self.steps), self.batch):
            yield self.store.replay_batch(self.local, self.steps[b0:b0 + self.batch])


class DeviceBatchLoader:
    """The iterable ``DeviceEpisodeStore.loader`` returns: what a ``DataLoader`` over an ``EpisodicDataset`` of ``episode_ids`` /
    ``episode_len`` / ``chunk_size`` with this ``batch_sampler`` delivers, as device tensors.  Exactly one index batch is drawn
    from the sampler per batch delivered, when it is asked for (no look-ahead): samplers that share a generator, as the train and
    validation samplers of ``load_data`` do, see the same stream of draws as on the host path with ``num_workers=0``."""

    on_device = True

    def __init__(self, store, episode_ids, episode_len, chunk_size, batch_sampler):
        self.store = store
        ids = [int(i) for i in episode_ids]
        self.episode_ids = ids                 # as the store was given them (train_bc replays the validation loader's)
        missing = [i for i in ids if i not in store._local_of]
        if missing:
            raise ValueError(f"DeviceBatchLoader: episodes {missing} are not in the store")
        self.local = np.asarray([store._local_of[i] for i in ids], dtype=np.int64)
        self.episode_len = [int(n) for n in episode_len]
        if len(self.episode_len) != len(ids) or np.any(store.T[self.local] != np.asarray(self.episode_len)):
            raise ValueError("DeviceBatchLoader: episode_len does not match the stored episodes")
        # padded_action[:chunk_size] of a max_episode_len-row table (EpisodicDataset.__getitem__)
        self.Q = min(int(chunk_size), max(self.episode_len))
        self.batch_sampler = iter(batch_sampler)

    def locate(self, indices):
        """flat dataset indices -> (the store's episode numbers, start_ts), as ``EpisodicDataset._locate_transition``"""
        ei, t = locate_transitions(indices, self.episode_len)
        return self.local[ei], t

    def __iter__(self):
        return self

    def __next__(self):
        e, t = self.locate(next(self.batch_sampler))
        return self.store.gather(e, t, self.Q)
