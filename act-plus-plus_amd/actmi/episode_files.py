"""Episode files as the input pipeline reads them, and nothing else: HDF5 via ``h5py`` when it is importable (the reference's format:
``/observations/qpos``, ``/observations/qvel``, ``/observations/images/<cam>``, ``/action``, optional ``/base_action``, attrs ``sim`` /
``compress``) or ``.npz`` files with the same keys (``open_episode``); the mirrored twin of an episode as a view of its file
(``MirrorTwinPath``, ``MirrorSpec``; DESIGN.md "Mirrored twin episodes"); the decode of compressed frames (``imdecode_bgr``); and the
listing of a dataset directory (``find_all_hdf5``).  ``data`` (the host dataset) and ``episode_store`` (the device-resident store)
both read files through this module; it imports neither."""
import fnmatch
import os

import numpy as np


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


def _entry_meta(root, key):
    """(shape, dtype) of an episode entry without reading it where the format allows (an .npy header, an h5py handle)"""
    if hasattr(root, "meta"):
        return root.meta(key)
    d = root[key]
    return tuple(int(v) for v in d.shape), np.dtype(d.dtype)
