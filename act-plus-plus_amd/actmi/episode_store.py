"""Device-resident episode store (``load_data(..., device_dataset=True)``; DESIGN.md "Device-resident episode store"): every episode
read ONCE into a device arena, a training batch then a few device gathers.

Bottom up: ``probe_sources`` reads the files' headers, ``plan_store`` lays the arena out from them and ``batch_table`` builds the index
table of one batch -- plain numpy, no device; ``DeviceEpisodeStore`` loads the arena by such a plan and launches the gathers over
such tables; ``DeviceEpisodeReplay`` and ``DeviceBatchLoader`` are the iterables the training loop sees.  Episode files are read
through ``episode_files``; ``data`` (the host dataset, ``load_data``) imports this module, never the other way round."""
import time
from collections import namedtuple

import numpy as np
import torch

from .episode_files import MirrorTwinPath, _EpisodeArrays, _entry_meta, _read_action, cloud_mirror_rule, imdecode_bgr, open_episode

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


# ---------------------------------------------------------------------------------------------------------------------
# the plan: headers -> layout -> the index table of a batch (numpy alone, no device)
# ---------------------------------------------------------------------------------------------------------------------
# One kind of frame a store holds -- the cameras' u8 B, G, R images or raw uint16 depth -- and, once planned, its blocks.
# What the kind is: ``key``, the group of the episode files (/observations/<key>/<cam>); ``segment``, the name of its offsets in a
# batch's index table; ``is_depth``; ``px_bytes``; ``torch_dtype`` of its tensor in a batch; ``row_unit``, the pixels of a row group
# of the mirrored gather's 16-byte form; ``decode_as``, the device JPEG decoder's output form.
# What ``plan_store`` adds: ``cams``; ``shape`` of a stored frame, (H, W, 3) / (H, W) (channel 0 of 3-D depth frames, as
# ``_depth_data`` keeps); ``frame_bytes``; ``aligned``, 1 where every frame lies at a multiple of 16 bytes -- the statement the
# gather's launcher cannot check for itself (actmi_op_gather_frames, `aligned`); ``src_block_off`` [sources, cams] int64, where each
# camera's [T, *shape] block starts in the arena; ``block_off`` [episodes, cams], its source's, a twin's permuted by its spec;
# ``flip`` [episodes, cams] uint8, 1 where a twin's camera is flipped along W.
# A store that stays compressed (``store_compressed``): ``src_block_off`` of a compressed source is its STREAM block (at most T * L
# bytes, ``stream_cap`` [sources, cams]; 0 for a source kept raw), ``mark_off`` [sources, cams] its mark block behind it and
# ``marks_per_frame`` the M + 1 records a frame has there; all None without the option.
_FrameKind = namedtuple("_FrameKind", "key segment is_depth px_bytes torch_dtype row_unit decode_as cams shape frame_bytes aligned "
                                      "src_block_off block_off flip stream_cap mark_off marks_per_frame",
                        defaults=((), None, 0, 0, None, None, None, None, None, None))
_KINDS = (_FrameKind("images", "frames", False, 3, torch.uint8, 16, "bgr"),
          _FrameKind("depth_images", "depth", True, 2, torch.uint16, 8, "u16"))

# ``tab["mode"]`` of a frame a compressed store keeps as packed depth (actmi_op_depth_pack), beside the JPEG sampling modes and -1
DEPTH_PACK_MODE = 100

# What the plan needs of one source file, from its headers: ``T``; ``compressed``; ``cloud_rows``, N of its stored cloud [T, N, 3] (0:
# the store holds no clouds) and ``cloud_rgb_dtype``; ``frames``, per kind (``_KINDS``) the (shape, dtype) of a frame, None where the
# file did not size it
# ``packed`` (``store_compressed`` and a compressed source; else None): per kind None or (L per camera, marks per frame), L the padded
# file length of a frame, what the entry's header gives
# ``encoded`` (``store_encode`` and a raw source, after the store's encode stage; else None): per kind None or (the exact stream bytes
# of every camera's block, marks per frame); with ``depth_pack`` the depth kind's entry is (the exact bytes of every depth camera's
# packed streams, 0): a stream block of exactly those bytes and an empty mark block
SourceHeader = namedtuple("SourceHeader", "T compressed cloud_rows cloud_rgb_dtype frames packed encoded",
                          defaults=(0, None, (None, None), None, None))


def _checked_frame_shape(kind, path, key, dtype, fshape):
    """the shape the store keeps of frames the headers call `dtype` `fshape`, or the ValueError of what it cannot keep"""
    if not kind.is_depth:
        if dtype != np.uint8 or len(fshape) != 3 or fshape[2] != 3:
            raise ValueError(f"{path}: {key} frames are {dtype} {fshape}, expected uint8 [H, W, 3]")
        return tuple(fshape)
    if dtype.kind != "u" or dtype.itemsize > 2:
        raise ValueError(f"{path}: {key} is {dtype}: the device-resident store keeps raw depth, an unsigned integer of at most 16 "
                         f"bits (float depth is normalised on the host: train without --device_dataset)")
    if len(fshape) not in (2, 3):
        raise ValueError(f"{path}: {key} frames are {fshape}, expected [H, W] or [H, W, C]")
    return tuple(fshape[:2])


def probe_sources(sources, cams, cloud_base=None, max_points=None, store_compressed=False, rows_per_mark=1, store_encode=False,
                  depth_pack=False):
    """Opens every source file once -> [SourceHeader].  `cams`: per kind the camera names; `cloud_base`: the stored cloud's group, None
    without clouds.  The sizes come from the entries' headers (the first file's decoded frames for a compressed dataset: later
    compressed files are checked as they are decoded).  Refused here, before anything large is allocated, each ``ValueError`` naming
    the file: an empty episode, clouds that are not two [T, N, 3] arrays of T steps or store more than `max_points` rows
    (``_read_cloud``'s checks, from the headers), frames that are not T, depth that is not an unsigned integer of at most 16 bits, and
    cameras or files whose frame sizes differ -- checked as the walk reaches the file, so the first bad file is the one named;
    with ``store_encode`` a raw source's depth entry (an 8-bit JPEG cannot hold raw uint16 depth) -- unless ``depth_pack`` admits it:
    the store then packs it losslessly (``DEPTH_PACK_MODE``), and refuses a dataset that holds JPEG-compressed depth beside raw
    depth, since one depth kind has one decode path."""
    headers, sized, marks_of, depth_codec = [], {}, {}, {}
    for i, path in enumerate(sources):
        with open_episode(path) as root:
            compressed = bool(root.attrs.get("compress", False))
            T = int(_entry_meta(root, "/action")[0][0])
            if T < 1:
                raise ValueError(f"{path}: empty episode")
            N, cdt = 0, None
            if cloud_base is not None:
                if f"{cloud_base}/xyz" not in root or f"{cloud_base}/rgb" not in root:
                    raise ValueError(f"{path}: no {cloud_base}/xyz and {cloud_base}/rgb")
                (xs, _xdt), (cs, cdt) = _entry_meta(root, f"{cloud_base}/xyz"), _entry_meta(root, f"{cloud_base}/rgb")
                if len(xs) != 3 or xs[2] != 3 or tuple(cs) != tuple(xs) or xs[1] < 1:
                    raise ValueError(f"{path}: point cloud xyz {tuple(xs)} / rgb {tuple(cs)}, expected two [T, N, 3] arrays")
                if xs[0] != T:
                    raise ValueError(f"{path}: {cloud_base}/xyz holds {xs[0]} clouds for an episode of {T} steps")
                if max_points is not None and xs[1] > max_points:
                    raise ValueError(f"{path}: the point cloud stores {xs[1]} rows, more than max_points {max_points} (no "
                                     "silent truncation: raise --max_points or down-sample the recording)")
                N = int(xs[1])
            frames, packed = [None] * len(_KINDS), [None] * len(_KINDS)
            for q, (kind, names) in enumerate(zip(_KINDS, cams)):
                lens = []
                for cam in names:
                    key = f"/observations/{kind.key}/{cam}"
                    shape, dtype = _entry_meta(root, key)
                    if shape[0] != T:
                        raise ValueError(f"{path}: {key} holds {shape[0]} frames for an episode of {T} steps")
                    if depth_pack and kind.is_depth:
                        depth_codec.setdefault("JPEG-compressed" if compressed else "raw", path)
                        if len(depth_codec) > 1:
                            raise ValueError(f"{path}: {key} is {'JPEG-compressed' if compressed else 'raw'} depth and "
                                             f"{depth_codec['raw' if compressed else 'JPEG-compressed']} holds "
                                             f"{'raw' if compressed else 'JPEG-compressed'} depth: depth_pack keeps one depth codec per store")
                    if compressed:
                        lens.append(int(shape[1]) if len(shape) == 2 else 0)
                        if i > 0 and kind.key in sized and store_compressed and kind.key not in marks_of:
                            # the files before this one were raw (store_encode): the block's marks from this file's first frame
                            marks_of[kind.key] = _marks_per_frame(np.asarray(root[key][0]), sized[kind.key][0], rows_per_mark)
                        if i > 0:
                            continue                               # sized by the first episode's frames; checked as it is decoded
                        first = np.asarray(root[key][0])
                        fshape, dtype = imdecode_bgr(first).shape, np.dtype(np.uint8)
                        if store_compressed and kind.key not in marks_of:
                            marks_of[kind.key] = _marks_per_frame(first, fshape[0], rows_per_mark)
                    else:
                        if store_encode and kind.is_depth and not depth_pack:
                            raise ValueError(f"{path}: {key} is raw depth, which an 8-bit JPEG cannot hold: store_encode takes raw "
                                             "camera frames only (train this dataset without --store_encode)")
                        fshape = shape[1:]
                    fshape = _checked_frame_shape(kind, path, key, dtype, fshape)
                    if sized.setdefault(kind.key, fshape) != fshape:
                        raise ValueError(f"{path}: {key} frames are {fshape}, others {sized[kind.key]}: one batch shape only")
                    frames[q] = (fshape, dtype)
                if store_compressed and compressed and names and all(lens):
                    packed[q] = (tuple(lens), marks_of[kind.key])
        headers.append(SourceHeader(T, compressed, N, cdt, tuple(frames), tuple(packed) if any(p is not None for p in packed) else None))
    return headers


def _marks_per_frame(buf, H, rows_per_mark):
    """M + 1 for the frames of a block, from its first frame: the MCU rows of that frame's sampling mode (a frame of a mode with more
    rows becomes a spill frame), or of 8-line rows when the parser refuses it"""
    from . import ops
    try:
        mode = ops.jpeg_parse(buf)["mode"]
    except ops.JpegUnsupported:
        mode = "444"
    return ops.jpeg_mark_count(H, mode, rows_per_mark) + 1


def twin_camera_map(path, cams):
    """Of the mirrored twin `path`, per kind and camera: (the place among `cams` of the source's camera whose frames it shows, whether
    they are flipped).  A twin whose source camera is not among the store's cameras is refused (``ValueError``)."""
    out = []
    with open_episode(path) as view:
        for kind, names in zip(_KINDS, cams):
            row = []
            for cam in names:
                found = view._resolve(f"/observations/{kind.key}/{cam}")
                if found is None:
                    raise ValueError(f"{path}: the mirror twin holds no /observations/{kind.key}/{cam}")
                src_cam = found[1].rsplit("/", 1)[1]
                if src_cam not in names:
                    raise ValueError(f"{path}: /observations/{kind.key}/{cam} of the twin is the source's {src_cam}, which is not "
                                     f"among the store's cameras {list(names)}")
                row.append((list(names).index(src_cam), bool(found[2])))
            out.append(tuple(row))
    return tuple(out)


def _starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)


# What ``plan_store`` decides: where everything lies in the arena, per source file and -- indexed with ``src_of`` -- per episode.
# ``all_kinds``: a _FrameKind per entry of ``_KINDS`` (one without cameras holds no block); ``nbytes``; ``padding``, the (begin, end)
# byte ranges no block holds; ``src_of`` [episodes], the source file of each; ``twin`` [episodes] bool.  Per source: ``src_T``,
# ``src_compressed``, ``src_N`` (stored rows of its clouds), ``src_cloud_off`` [sources, 2] (its xyz and its colour block; [sources,
# 0] without clouds), ``src_row0`` (of its steps in the host array of valid counts, ``cloud_n``).  ``cloud_rgb_fmt``: 0 uint8 colours
# (every source stores them so), 1 float32 everywhere; ``cloud_rgb_bytes`` of one stored colour row.  Per episode: ``T``,
# ``compressed``, ``row0`` (of its rows in ``actions`` / ``qpos``).  ``kinds``: those of ``all_kinds`` that have cameras; ``has_twins``;
# ``has_clouds``.
# ``src_packed`` [sources] bool: the source's frames stay compressed (None: the store was planned without ``store_compressed``).
StoreLayout = namedtuple("StoreLayout", "all_kinds nbytes padding src_of twin src_T src_compressed src_N src_cloud_off src_row0 "
                                        "cloud_rgb_fmt cloud_rgb_bytes T compressed row0 kinds has_twins has_clouds src_packed", defaults=(None,))


def plan_store(headers, cams, src_of, twin_cams=None):
    """The arena of a store, from its sources' headers -> StoreLayout.  Per source file (each once, in order), per camera of
    ``cams[0]`` one u8 ``[T, H, W, 3]`` block, then per depth camera (``cams[1]``) one raw uint16 ``[T, H, W]`` block, then -- where the
    headers name clouds -- one float32 ``[T, N, 3]`` xyz block and one colour block ``[T, N, 3]``, uint8 when every source stores
    uint8, float32 everywhere otherwise; N may differ between sources.  Every block start is padded to 256 bytes (``arena_layout``).

    ``src_of[i]``: the source of episode i.  ``twin_cams[i]``: None for an episode file; for a mirrored twin its
    ``twin_camera_map``.  A twin adds no bytes: its camera blocks are its source's, permuted, with a flag per camera that is flipped,
    and its clouds are its source's blocks."""
    src_of = np.asarray(src_of, dtype=np.int64)
    twin_cams = [None] * len(src_of) if twin_cams is None else list(twin_cams)
    src_T = np.asarray([h.T for h in headers], dtype=np.int64)
    src_N = np.asarray([h.cloud_rows for h in headers], dtype=np.int64)
    nc = 2 if headers[0].cloud_rows else 0                            # an xyz and a colour block per source, behind its frames
    rgb_bytes = 3 if not nc or all(h.cloud_rgb_dtype == np.uint8 for h in headers) else 12
    shapes = [next((h.frames[q][0] for h in headers if h.frames[q] is not None), None) for q in range(len(_KINDS))]
    fbytes = [int(np.prod(s[:2])) * k.px_bytes if c else 0 for k, c, s in zip(_KINDS, cams, shapes)]
    # ``store_compressed`` (a header says so with ``packed``): a camera or depth block of a compressed source is one stream block of
    # at most T * L bytes, L the padded file length, and behind it a mark block of T * (M + 1) * 32 bytes; a source kept raw has its
    # [T, frame] block and an empty mark block, so that every source has the same number of blocks
    # ``store_encode`` (``encoded``): a camera block of a raw source whose frames the store encoded is a stream block of exactly the
    # bytes its segments take, aligned like every block, and a mark block of T * (M + 1) * 32 bytes
    option = any(h.packed is not None or h.encoded is not None for h in headers)

    def stream_bytes(h, q, k, T):                                    # of camera k's stream block, None for a block kept raw
        if h.encoded is not None and h.encoded[q] is not None:
            return int(h.encoded[q][0][k])
        return T * h.packed[q][0][k] if h.packed is not None and h.packed[q] is not None else None

    def marks_of(h, q):
        pk = h.encoded[q] if h.encoded is not None and h.encoded[q] is not None else (h.packed[q] if h.packed is not None else None)
        return None if pk is None else int(pk[1])
    # one M + 1 per kind, the largest any source names (a frame with fewer marks uses the head of its records)
    mpfs = [max([marks_of(h, q) or 0 for h in headers]) for q in range(len(_KINDS))]
    blocks = []
    for h, T, N in zip(headers, src_T.tolist(), src_N.tolist()):
        for q, (fb, c) in enumerate(zip(fbytes, cams)):
            for k in range(len(c)):
                if not option:
                    blocks.append(T * fb)
                elif stream_bytes(h, q, k, T) is None:
                    blocks += [T * fb, 0]
                else:
                    blocks += [stream_bytes(h, q, k, T), T * mpfs[q] * 32]
        blocks += [T * N * 12, T * N * rgb_bytes][:nc]
    offs, nbytes = arena_layout(blocks)
    ends = [int(o) + int(b) for o, b in zip(offs, blocks)]
    padding = [(e, int(n)) for e, n in zip(ends, list(offs[1:]) + [nbytes]) if n > e]
    offs = offs.reshape(len(headers), -1)
    kinds, col = [], 0
    for q, (proto, c, shape, fb) in enumerate(zip(_KINDS, cams, shapes, fbytes)):
        width = (2 if option else 1) * len(c)
        src_off = offs[:, col:col + width:2 if option else 1].copy()
        extra = {}
        if option and c:
            cap = np.asarray([[stream_bytes(h, q, k, T) or 0 for k in range(len(c))] for h, T in zip(headers, src_T.tolist())], dtype=np.int64)
            mpf = mpfs[q]
            extra = dict(stream_cap=cap, mark_off=offs[:, col + 1:col + width:2].copy(), marks_per_frame=int(mpf))
        col += width
        off, flip = src_off[src_of], np.zeros((len(src_of), len(c)), dtype=np.uint8)
        for i, tw in enumerate(twin_cams):
            for k, (src_k, flipped) in enumerate(tw[q] if tw is not None else ()):
                off[i, k], flip[i, k] = src_off[src_of[i], src_k], 1 if flipped else 0
        kinds.append(proto._replace(cams=tuple(c), shape=shape if c else None, frame_bytes=fb, aligned=1 if c and fb % 16 == 0 else 0,
                                    src_block_off=src_off, block_off=off, flip=flip, **extra))
    compressed, twin = [h.compressed for h in headers], [tw is not None for tw in twin_cams]
    return StoreLayout(tuple(kinds), nbytes, padding, src_of, twin, src_T, compressed, src_N, offs[:, col:].copy(), _starts(src_T),
                       0 if rgb_bytes == 3 else 1, rgb_bytes, src_T[src_of], [compressed[j] for j in src_of], _starts(src_T[src_of]),
                       tuple(k for k in kinds if k.cams), any(twin), nc > 0,
                       np.asarray([h.packed is not None or h.encoded is not None for h in headers]) if option else None)


class BatchTable:
    """Named numpy segments, in the order given, as the ONE int64 table a batch uploads (``host``); ``slices`` cuts the uploaded
    tensor back into the segments by name (an empty segment has no slice).  Every segment is a whole number of 8-byte words."""

    def __init__(self, segments):
        self.bounds, parts, n = {}, [], 0
        for name, v in segments.items():                              # plain Python: this runs once per training step
            parts.append(np.ascontiguousarray(v).reshape(-1).view(np.int64))
            self.bounds[name], n = (n, n + len(parts[-1])), n + len(parts[-1])
        self.host = np.concatenate(parts)

    def slices(self, tab):
        return {name: tab[a:b] for name, (a, b) in self.bounds.items() if b > a}


def cloud_items(layout, e, t, cloud_n):
    """the records (``ops.cloud_item_dtype``) of the clouds of samples (e[b], t[b]): where the step's rows lie in its source's two
    blocks, how many there are, how many are points (``cloud_n``, the valid count of every stored step), and the mirror flag of a
    twin, whose clouds are its source's blocks"""
    from . import ops
    j = layout.src_of[e]
    N = layout.src_N[j]
    items = np.zeros(len(e), dtype=ops.cloud_item_dtype())
    items["xyz_off"] = layout.src_cloud_off[j, 0] + t * N * 12
    items["rgb_off"] = layout.src_cloud_off[j, 1] + t * N * layout.cloud_rgb_bytes
    items["rows"], items["n"] = N, cloud_n[layout.src_row0[j] + t]
    items["flags"] = np.asarray(layout.twin, dtype=np.int32)[e]
    return items


def batch_table(layout, e, t, cloud_n=None, extra=None):
    """The index table of the batch of samples (e[b], t[b]), int64 arrays: ``frames`` and ``depth``, the arena byte offset of every
    camera's frame; ``samples``, the (e, t) pairs as int32; with twins ``flips``, a flag per frame and depth item packed eight to a
    word; with clouds ``cloud_items``."""
    seg = {k.segment: k.block_off[e] + t[:, None] * k.frame_bytes for k in layout.all_kinds}
    seg["samples"] = np.stack([e, t], axis=1).astype(np.int32)
    if layout.has_twins:
        flags = np.concatenate([k.flip[e].reshape(-1) for k in layout.all_kinds])
        seg["flips"] = np.zeros((len(flags) + 7) // 8 * 8, dtype=np.uint8)
        seg["flips"][:len(flags)] = flags
    if layout.has_clouds:
        seg["cloud_items"] = cloud_items(layout, e, t, cloud_n)
    if extra:                                                         # a compressed store: the batch's JPEG records and their marks
        seg.update(extra)
    return BatchTable(seg)


# ---------------------------------------------------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------------------------------------------------
class DeviceEpisodeStore:
    """Every frame of the named episodes (``episode_ids`` order, duplicates dropped) in ONE device arena, read from the files once; a
    training batch is then a device-to-device gather (``gather``) and equals what ``EpisodicDataset.__getitem__`` + the default
    collation (``collate_pcd`` with stored clouds) give for the same flat indices, bit for bit and dtype for dtype.  Actions and qpos
    (float32 as the dataset converts them, ``/base_action`` columns included), the episode table and the four stat vectors are small
    device arrays.  Mirrored twins (``MirrorTwinPath`` entries) add no frame bytes: ``sources`` are the files the arena holds, each
    once; a twin has its own rows in ``actions`` / ``qpos`` and its own episode record.

    Refused before anything large is allocated: ``use_pcd`` without exactly one cloud name and a policy class other than ACT
    (``NotImplementedError``), what ``probe_sources`` and ``twin_camera_map`` refuse, and a dataset larger than the budget
    (``MemoryError`` naming both numbers).  ``budget_bytes`` None: the device's free memory now minus ``DEVICE_STORE_RESERVE_BYTES``.
    ``device_decode`` changes neither what the arena holds nor which error a bad file raises (``_decode_on_device``).
    ``store_compressed`` (with ``device_decode``): the arena holds the entropy segments and, per frame, the marks of one index pass
    (actmi_op_jpeg_index) instead of the decoded frames; a batch is decoded by actmi_op_jpeg_decode_marked and is bit for bit the
    batch of the other stores.  Frames the device does not take stay raw in a spill tensor per kind (``_load_packed``).
    ``store_encode`` (with ``store_compressed``): a source whose camera entries are raw uint8 ``[T, H, W, 3]`` is encoded on the device
    as it is read (``_encode_sources``: B, G, R pixels at ``encode_quality`` / ``encode_subsampling``, as ``compress_episode`` encodes
    them), its marks written by the encoder (actmi_op_jpeg_encode_marked) -- no index launch; raw and compressed sources may be mixed,
    and the batches are those of a compressed store of ``compress_dataset_dir``'s output.  ``encode_stats``: the frames encoded.
    ``depth_pack`` (with ``store_encode`` and ``use_depth``): the raw uint16 depth entries of raw sources, which ``store_encode`` alone
    refuses, are packed losslessly on the device as they are read (``_pack_depth_sources``, actmi_op_depth_pack) and every batch's
    depth is unpacked straight into its tensor by one actmi_op_depth_unpack launch, a twin's flip being the record's flag; the
    depth tensors are bit for bit those of the decoded store.  ``depth_pack_stats``: frames, raw bytes and stream bytes.

    Every rank of a data-parallel run holds its own full store."""

    RING = 4                 # pinned index blocks in flight: a block is rewritten only after its copy has executed

    def __init__(self, dataset_path_list, episode_ids, camera_names, norm_stats, device, depth_camera_names=None, use_depth=False,
                 budget_bytes=None, use_pcd=False, policy_class="ACT", stage_bytes=64 << 20, pointcloud_names=None, max_points=None,
                 pcd_ignore_mask=False, device_decode=False, decode_frames=256, store_compressed=False, rows_per_mark=1,
                 store_encode=False, encode_quality=50, encode_subsampling="420", depth_pack=False):
        self.device_decode, self.decode_frames = bool(device_decode), int(decode_frames)
        self.depth_pack = bool(depth_pack)
        if self.depth_pack and not store_encode:
            raise ValueError("depth_pack packs the raw depth of episodes the store encodes as it loads them: it needs store_encode "
                             "(and store_compressed, device_decode, device_dataset)")
        if self.depth_pack and not use_depth:
            raise ValueError("depth_pack packs depth frames: it needs use_depth")
        self.store_compressed, self.rows_per_mark = bool(store_compressed), int(rows_per_mark)
        self.store_encode, self.encode_quality, self.encode_subsampling = bool(store_encode), encode_quality, str(encode_subsampling)
        if self.store_encode and not self.store_compressed:
            raise ValueError("store_encode encodes raw episodes into the store that stays compressed: it needs store_compressed (and "
                             "device_decode, device_dataset)")
        if self.store_encode:
            from . import ops
            ops._jpeg_enc_args(self.encode_subsampling, quality=encode_quality)
            if self.decode_frames < 1 or self.decode_frames > 65535:
                raise ValueError("store_encode: decode_frames must be in 1..65535")
        if self.store_compressed and not self.device_decode:
            raise ValueError("store_compressed keeps the frames the device decodes: it needs device_decode (and device_dataset)")
        if self.store_compressed and self.rows_per_mark < 1:
            raise ValueError("store_compressed: rows_per_mark must be at least 1")
        self.pointcloud_names = list(pointcloud_names) if pointcloud_names else []
        self.has_clouds = bool(use_pcd) and bool(self.pointcloud_names)
        if self.has_clouds and len(self.pointcloud_names) != 1:
            raise ValueError(f"use_pcd needs exactly one pointcloud name (/observations/pointcloud/<name>), got {self.pointcloud_names}")
        if self.has_clouds and use_depth:
            raise NotImplementedError("use_depth together with use_pcd is not supported")
        self.max_points, self.pcd_ignore_mask = None if max_points is None else int(max_points), bool(pcd_ignore_mask)
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
        self.cloud_mirror = None                                      # (axis, offset, c2): the one rule of the twins' clouds
        if self.has_clouds and self.has_twins:
            rules = {getattr(p, "cloud_mirror", None) for p, tw in zip(self.paths, self.twin) if tw}
            if None in rules:
                raise ValueError("use_pcd with mirror twins: a stored point cloud has no mirror rule (MirrorTwinPath(..., "
                                 "cloud_mirror=(axis, offset)) gives it one)")
            if len(rules) != 1:
                raise ValueError(f"DeviceEpisodeStore: the twins carry different cloud mirror rules {sorted(rules)}: one gather takes one")
            self.cloud_mirror = cloud_mirror_rule(rules.pop())
        self.device, self.stage_bytes = device, int(stage_bytes)
        cams = (tuple(self.camera_names), tuple(self.depth_camera_names) if self.use_depth else ())
        self._cloud_base = f"/observations/pointcloud/{self.pointcloud_names[0]}" if self.has_clouds else None
        headers = probe_sources(self.sources, cams, self._cloud_base, self.max_points, self.store_compressed, self.rows_per_mark,
                                self.store_encode, self.depth_pack)
        if budget_bytes is None:
            free, _total = torch.cuda.mem_get_info(torch.device(device))
            budget_bytes = free - DEVICE_STORE_RESERVE_BYTES
        self.budget_bytes = int(budget_bytes)
        self.bus_bytes = 0                                            # bytes of frames and clouds that crossed to the device
        self._pin, self._pin_ev, self._pin_i = None, [None, None], 0
        self.encode_stats, self._held, self._held_bytes, self._encode_staging = {"device": 0}, {}, 0, 0
        self.depth_pack_stats, self._held_depth = {"frames": 0, "raw_bytes": 0, "stream_bytes": 0}, {}
        if self.store_encode:
            headers = self._encode_sources(headers, cams)
        if self.depth_pack:
            headers = self._pack_depth_sources(headers, cams)
        if self.store_compressed and not all((h.packed is not None and all(p is not None for p, c in zip(h.packed, cams) if c)) or
                                             h.encoded is not None for h in headers):
            raise NotImplementedError("store_compressed: every source must be a compressed episode (a store of compressed and raw "
                                      "sources is planned by plan_store but not loaded); drop --store_compressed")
        self.layout = lay = plan_store(headers, cams, [where[s] for s in srcs],
                                       [twin_camera_map(p, cams) if tw else None for p, tw in zip(self.paths, self.twin)])
        self.kinds, (img, dep) = lay.kinds, lay.all_kinds
        self.K, self.Kd = len(img.cams), len(dep.cams)
        self.frame_shape, self.frame_bytes, self.aligned, self.block_off, self.flip = \
            img.shape, img.frame_bytes, img.aligned, img.block_off, img.flip
        self.depth_shape, self.depth_bytes, self.depth_aligned, self.depth_block_off, self.depth_flip = \
            dep.shape, dep.frame_bytes, dep.aligned, dep.block_off, dep.flip
        self.nbytes, self.T, self.row0, self.compressed = lay.nbytes, lay.T, lay.row0, lay.compressed
        self.cloud_rgb_fmt, self.cloud_rgb_bytes = lay.cloud_rgb_fmt, lay.cloud_rgb_bytes
        # with encoded sources the segments and marks the encode stage holds live beside the arena until they are copied in, and
        # the stage's device staging counts as well (it is released before the arena is allocated: the check is the safe side)
        need = self.nbytes + self._held_bytes + self._encode_staging
        if need > self.budget_bytes:
            self._held, self._held_depth = {}, {}
            raise MemoryError(f"DeviceEpisodeStore: {len(self.paths)} episodes need {need} bytes on the device "
                              f"({need / 2**30:.2f} GiB), the budget is {self.budget_bytes} bytes "
                              f"({self.budget_bytes / 2**30:.2f} GiB): train without --device_dataset, or raise --device_dataset_gb")
        self._load(norm_stats)

    # ---- the one read of every episode ----------------------------------------------------------------------------
    def _load(self, norm_stats):
        """The blocks reach the device through two bounded pinned staging buffers of ``stage_bytes``, never a pinned copy of an
        episode, and every block is checked against the plan again as it is loaded."""
        from . import ops
        lay, dev = self.layout, torch.device(self.device)
        t_begin = time.perf_counter()
        # a compressed store's stream blocks are filled only as far as the segments reach, and a spill frame's marks not at all
        self.arena = (torch.zeros if self.store_compressed else torch.empty)(self.nbytes, dtype=torch.uint8, device=dev)
        for a, b in lay.padding:                                      # the padding between blocks is zero: two stores of one
            self.arena[a:b].zero_()                                   # dataset hold the same bytes everywhere
        stage = max(self.stage_bytes, self.frame_bytes, self.depth_bytes, int(lay.src_N.max()) * 12 if self.has_clouds else 0)
        self.cloud_n = np.zeros(int(lay.src_T.sum()) if self.has_clouds else 0, dtype=np.int32)   # valid rows of every stored step
        self._open_staging(stage)
        self.decode_stats = {"device": 0, "host": 0}
        self._decoders, self._pending, self._jpeg_stream = {}, [], None
        self._init_packed()
        if self.device_decode and any(lay.src_compressed) and not self.store_compressed:
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
                    self._load_source(root, int(lay.src_of[i]))
                    loaded.add(int(lay.src_of[i]))
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
        self._jpeg_stream = None                                      # and so are the decoder's workspace and stream buffer
        if self.store_compressed:
            self._seal_packed()                                       # a compressed store keeps its decoders: every batch decodes
        else:
            self._decoders = None
        self.load_seconds = time.perf_counter() - t_begin
        self._host, self._host_ev, self._slot = [None] * self.RING, [None] * self.RING, 0

    def _load_source(self, root, j):
        """the frames of source file j, open as `root`, into its blocks of the arena"""
        path, T, compressed = self.sources[j], int(self.layout.src_T[j]), self.layout.src_compressed[j]
        for kind in self.kinds:
            for k, cam in enumerate(kind.cams):
                key = f"/observations/{kind.key}/{cam}"
                if (j, k) in self._held and not kind.is_depth:
                    self._load_encoded(kind, T, j, k)                 # read and encoded before the plan: not read again
                elif (j, k) in self._held_depth and kind.is_depth:
                    self._load_packed_depth(kind, T, j, k)            # read and packed before the plan
                elif self.store_compressed:
                    self._load_packed(root[key], kind, T, j, k, f"{path}: {key}")
                else:
                    self._load_block(root[key], kind, T, compressed, int(kind.src_block_off[j, k]), f"{path}: {key}")
        self._finish_device_decode()
        self._finish_index()
        if self.has_clouds:
            self._load_clouds(root, j)

    def _load_clouds(self, root, j):
        """the clouds of source file j into its two blocks, and the valid count of every step by ``_read_cloud``'s rules (raised
        with the file and the timestep) into the host array ``cloud_n``"""
        lay = self.layout
        path, T, N, base = self.sources[j], int(lay.src_T[j]), int(lay.src_N[j]), self._cloud_base
        f32c = self.cloud_rgb_fmt == 1
        for leaf, off, rb in (("xyz", int(lay.src_cloud_off[j, 0]), 12), ("rgb", int(lay.src_cloud_off[j, 1]), self.cloud_rgb_bytes)):
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
                if off + t0 * N * rb + n > self.nbytes:               # cannot happen with the sizes the plan checked
                    raise MemoryError(f"{path}: cloud block leaves the arena of {self.nbytes} bytes")
                self._stage(off + t0 * N * rb, n, lambda view, flat=flat: np.copyto(view, flat))
        counts = stored_cloud_counts(root, base, path, T, N, self.pcd_ignore_mask)
        self.cloud_n[int(lay.src_row0[j]):int(lay.src_row0[j]) + T] = counts

    def _open_staging(self, nbytes):
        """the pinned staging pair, of at least `nbytes` each"""
        if self._pin is None or self._pin[0].numel() < nbytes:
            for ev in self._pin_ev:
                if ev is not None:
                    ev.synchronize()
            self._pin = None
            self._pin = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._pin_ev, self._pin_i = [None, None], 0

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
        self._pin_ev[j].record(torch.cuda.current_stream(dst.device))

    def _load_block(self, entry, kind, T, compressed, dst_off, where):
        """one camera's block, a staging buffer's worth of frames at a time; compressed episodes are decoded once"""
        fb = kind.frame_bytes
        per = max(1, self._pin[0].numel() // fb)
        for t0 in range(0, T, per):
            t1 = min(T, t0 + per)
            piece = np.asarray(entry[t0:t1])
            if compressed and self._jpeg_stream is not None and piece.ndim == 2 and piece.dtype == np.uint8:
                for i in self._decode_on_device(piece, dst_off + t0 * fb, kind):
                    self._decode_on_host(piece[i], kind, dst_off + (t0 + i) * fb, where)    # what the parser refused
                continue
            if compressed:                                            # utils.py:104-107, frame by frame
                piece = np.stack([imdecode_bgr(buf) for buf in piece])
            self._stage_frames(piece, t1 - t0, kind, dst_off + t0 * fb, where)

    def _stage_frames(self, piece, n, kind, dst_off, where):
        """`n` decoded frames of one kind, checked against the plan, to arena[dst_off:]"""
        if kind.is_depth:
            if piece.dtype.kind != "u" or piece.dtype.itemsize > 2:
                raise ValueError(f"{where} is {piece.dtype}: not raw depth (an unsigned integer of at most 16 bits)")
            if piece.ndim == 4:
                piece = piece[..., 0]                                 # _depth_data: a 3-D frame keeps channel 0
            piece = piece.astype(np.uint16, copy=False)
        if piece.shape != (n,) + tuple(kind.shape) or (not kind.is_depth and piece.dtype != np.uint8):
            raise ValueError(f"{where}: frames {piece.dtype} {piece.shape[1:]}, the store was sized for {tuple(kind.shape)}")
        if dst_off + n * kind.frame_bytes > self.nbytes:             # cannot happen with the sizes the plan checked
            raise MemoryError(f"{where}: block leaves the arena of {self.nbytes} bytes")
        flat = np.ascontiguousarray(piece).reshape(-1).view(np.uint8)
        self._stage(dst_off, n * kind.frame_bytes, lambda view: np.copyto(view, flat))

    # ---- compressed frames decoded on the device (device_decode) -------------------------------------------------------
    def _decode_on_host(self, buf, kind, dst_off, where):
        """one compressed frame by the host path, as without ``device_decode``"""
        self._stage_frames(imdecode_bgr(buf)[None], 1, kind, dst_off, where)
        self.decode_stats["host"] += 1

    def _decode_on_device(self, piece, dst_off, kind):
        """``device_decode``: the frames of a compressed source are decoded on the device (``ops.JpegDecoder``, actmi_op_jpeg_decode)
        instead of one by one through PIL.  The frames of `piece` ([n, L] u8, one zero-padded file each) that the parser accepts at
        the store's size: their entropy segments go through the staging pair and the op writes straight into
        arena[dst_off + i * frame bytes], B, G, R for cameras and the uint16 form for depth, up to ``decode_frames`` frames a launch;
        -> the indices of the other frames (refused by the parser, of another size, or larger than the staging buffer), which the
        caller decodes on the host.  The statuses stay on the device until ``_finish_device_decode``.  The decoder's workspace and
        stream buffer live only during the load."""
        from . import ops
        fb = kind.frame_bytes
        H, W = kind.shape[:2]
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
                status = dec.decode(self._jpeg_stream, frames, mode, kind.decode_as, self.arena)
                self._pending.append((status, [(piece[i], int(o)) for (i, _info), o in zip(part, frames["dst_off"])], kind))
                k0 = k1
        return sorted(host)

    def _finish_device_decode(self):
        """the statuses of a source file's launches, read back once; a frame whose status is not 0 takes the host path, before the
        store is handed out.  ``decode_stats`` counts the frames of both paths."""
        if not self._pending:
            return
        status = torch.cat([st for st, _frames, _kind in self._pending]).cpu().numpy()
        k = 0
        for _st, frames, kind in self._pending:
            for buf, off in frames:
                if status[k]:
                    self._decode_on_host(buf, kind, off, f"a frame at arena byte {off}")
                else:
                    self.decode_stats["device"] += 1
                k += 1
        self._pending = []

    # ---- a store that stays compressed (store_compressed) ---------------------------------------------------------------
    def _init_packed(self):
        """per kind the host tables of a compressed store, one row per stored frame (source j, camera k, step t at
        ``_frame_row(q, j, k) + t``): its JPEG record (segment offset in the arena, length, restart interval, table set), the index of
        its mark 0 among the arena's 32-byte words, its sampling mode (-1: a spill frame) and its row in the spill tensor"""
        from . import ops
        self._ptab, self._spill_host, self._spill, self._index_pending = [], [], [], []
        self.stream_bytes_used, self._sticky, self._scratch, self._depth_sticky = 0, None, {}, None
        if not self.store_compressed:
            return
        lay = self.layout
        for kind in lay.all_kinds:
            n = int(lay.src_T.sum()) * len(kind.cams)
            self._ptab.append(dict(rec=np.zeros(n, dtype=ops.jpeg_frame_dtype()), first=np.zeros(n, dtype=np.int64),
                                   mode=np.full(n, -1, dtype=np.int8), spill=np.full(n, -1, dtype=np.int64)))
            self._spill_host.append([])
        # which of its source's cameras an episode's camera shows (a twin's are permuted): the column of its block
        self._src_cam = [np.asarray([[int(np.nonzero(kind.src_block_off[lay.src_of[i]] == kind.block_off[i, k])[0][0])
                                      for k in range(len(kind.cams))] for i in range(len(lay.src_of))], dtype=np.int64).reshape(len(lay.src_of), len(kind.cams))
                         for kind in lay.all_kinds]

    def _frame_row(self, q, j, k):
        lay = self.layout
        return lay.src_row0[j] * len(lay.all_kinds[q].cams) + k * lay.src_T[j]

    def _load_packed(self, entry, kind, T, j, k, where):
        """one camera's block of a compressed store: the entropy segments of the frames the parser accepts at the store's size go
        back to back through the staging pair into the stream block, one index launch per up to ``decode_frames`` frames writes their
        marks into the mark block; the other frames (refused by the parser, of another size or with more MCU rows than the block
        has marks for, a segment larger than the staging buffer or than what is left of the block) are spill frames."""
        from . import ops
        q = self.layout.all_kinds.index(kind)
        tab, fb = self._ptab[q], kind.frame_bytes
        H, W = kind.shape[:2]
        dec = self._decoders.get((H, W))
        if dec is None:
            dec = self._decoders[(H, W)] = ops.JpegDecoder(self.device, H, W, max_frames=self.decode_frames)
        row0 = int(self._frame_row(q, j, k))
        s0, cap = int(kind.src_block_off[j, k]), int(kind.stream_cap[j, k])
        m0, mpf = int(kind.mark_off[j, k]), int(kind.marks_per_frame)
        stage_cap, cursor = int(self._pin[0].numel()), 0
        per = max(1, stage_cap // max(1, cap // max(T, 1)))
        for t0 in range(0, T, per):
            piece = np.asarray(entry[t0:min(T, t0 + per)])
            todo = {}
            for i, buf in enumerate(piece):
                t, info = t0 + i, None
                if piece.ndim == 2 and piece.dtype == np.uint8:
                    try:
                        info = dec.parse(buf)
                    except ops.JpegUnsupported:
                        info = None
                if info is not None and ((info["H"], info["W"]) != (H, W) or info["seg_len"] > stage_cap or
                                         ops.jpeg_mark_count(H, info["mode"], self.rows_per_mark) + 1 > mpf or
                                         cursor + sum(x[2]["seg_len"] for v in todo.values() for x in v) + info["seg_len"] > cap):
                    info = None
                if info is None:
                    self._spill_frame(q, row0 + t, buf, kind, where)
                else:
                    todo.setdefault(info["mode"], []).append((t, buf, info))
            for mode, items in todo.items():
                k0 = 0
                while k0 < len(items):                                # as many frames as the staging buffer and one launch hold
                    k1, nbytes = k0, 0
                    while k1 < len(items) and k1 - k0 < dec.max_frames and nbytes + items[k1][2]["seg_len"] <= stage_cap:
                        nbytes += items[k1][2]["seg_len"]
                        k1 += 1
                    part = items[k0:k1]
                    rows = np.asarray([row0 + t for t, _b, _i in part], dtype=np.int64)
                    lens = np.asarray([info["seg_len"] for _t, _b, info in part], dtype=np.int64)
                    rec = tab["rec"]
                    rec["seg_len"][rows] = lens
                    rec["seg_off"][rows] = s0 + cursor + np.concatenate([[0], np.cumsum(lens)[:-1]])
                    rec["restart_interval"][rows] = [info["restart_interval"] for _t, _b, info in part]
                    rec["table_set"][rows] = [dec.table_index(info["tables"]) for _t, _b, info in part]
                    tab["first"][rows] = [(m0 + t * mpf * 32) // 32 for t, _b, _i in part]
                    tab["mode"][rows] = ops.JPEG_MODES[mode]

                    def fill(view, part=part, lens=lens):
                        o = 0
                        for (_t, buf, info), n in zip(part, lens):
                            view[o:o + n] = buf[info["seg_off"]:info["seg_off"] + n]
                            o += int(n)
                    if nbytes:
                        self._stage(s0 + cursor, nbytes, fill)
                    cursor += nbytes
                    _marks, status = dec.index(self.arena, rec[rows], mode, marks=self.arena[:self.nbytes // 32 * 32], first=tab["first"][rows],
                                               rows_per_mark=self.rows_per_mark)
                    self._index_pending.append((status, q, rows, [b for _t, b, _i in part], kind, where))
                    k0 = k1
        self.stream_bytes_used += cursor

    # ---- raw sources encoded at load (store_encode) --------------------------------------------------------------------
    def _encode_sources(self, headers, cams):
        """The encode stage, between ``probe_sources`` and ``plan_store``: the planner needs every stream block's bytes before the
        arena exists.  Every camera entry of a raw source is read ONCE, at most ``decode_frames`` frames a piece, through the pinned
        staging pair into a device buffer that holds the piece raw.  Per piece: one actmi_op_jpeg_encode launch with windows of 0
        bytes gives every frame's true seg_len (its contract), the lengths are read back once, and one actmi_op_jpeg_encode_marked
        launch with exact windows writes the segments back to back into a tensor of their size and the marks into a [n, M + 1, 32]
        tensor.  The tensors are held until ``_load_encoded`` copies them into the arena.  A nonzero status of the second launch is
        a bug (``RuntimeError``).  -> the headers, a raw source's with ``encoded``: the exact stream bytes per camera."""
        from . import ops
        dev = torch.device(self.device)
        names = cams[0]
        todo = [j for j, h in enumerate(headers) if not h.compressed and h.frames[0] is not None]
        if not todo or not names:
            return headers
        (H, W, _c), mode = headers[todo[0]].frames[0][0], self.encode_subsampling
        fb = H * W * 3
        packed = [h.packed[0][1] for h in headers if h.packed is not None and h.packed[0] is not None]
        mpf = max(packed + [ops.jpeg_mark_count(H, mode, self.rows_per_mark) + 1])
        per = min(self.decode_frames, max(headers[j].T for j in todo))
        ws_bytes = max(16, ops.jpeg_encode_workspace_bytes(per, H, W, mode))
        self._encode_staging = per * fb + ws_bytes
        if self._encode_staging > self.budget_bytes:
            raise MemoryError(f"DeviceEpisodeStore: the encode stage of store_encode needs {self._encode_staging} bytes on the device "
                              f"({self._encode_staging / 2**30:.2f} GiB) for {per} frames a launch, the budget is {self.budget_bytes} bytes "
                              f"({self.budget_bytes / 2**30:.2f} GiB): lower decode_frames, or raise --device_dataset_gb")
        enc = ops.JpegEncoder(dev, H, W, max_frames=per, quality=self.encode_quality, mode=mode)
        raw = torch.empty(per * fb, dtype=torch.uint8, device=dev)
        none = torch.empty(16, dtype=torch.uint8, device=dev)       # the windows of the first launch are empty
        self._open_staging(max(self.stage_bytes, fb))
        step = max(1, self._pin[0].numel() // fb)
        self._encoder_tables = ops.jpeg_parse(ops.jpeg_assemble(enc.header, b""))["tables"]
        out = list(headers)
        for j in todo:
            T, nbytes, checks = headers[j].T, [], []
            with open_episode(self.sources[j]) as raw_root:
                root = _EpisodeArrays(raw_root)
                for k, cam in enumerate(names):
                    key = f"/observations/images/{cam}"
                    entry = root[key]
                    streams, marks, lens = [], [], []
                    for t0 in range(0, T, per):
                        n = min(per, T - t0)
                        piece = np.asarray(entry[t0:t0 + n])
                        if piece.shape != (n, H, W, 3) or piece.dtype != np.uint8:
                            raise ValueError(f"{self.sources[j]}: {key}: frames {piece.dtype} {piece.shape[1:]}, the store was sized for {(H, W, 3)}")
                        for i0 in range(0, n, step):
                            flat = np.ascontiguousarray(piece[i0:i0 + step]).reshape(-1)
                            self._stage(i0 * fb, flat.size, lambda view, flat=flat: np.copyto(view, flat), raw)
                        _d, seg_len, _st = enc.encode(raw[:n * fb], dst=none, records=ops.jpeg_enc_records(n, H, W, 0, dst_off=np.zeros(n, dtype=np.int64)))
                        ln = seg_len.cpu().numpy().astype(np.int64)   # the one read-back of the launch
                        if ln.min() < 1:
                            raise RuntimeError(f"{self.sources[j]}: {key}: the encoder reports a segment of {int(ln.min())} bytes")
                        rec = ops.jpeg_enc_records(n, H, W, 0, dst_off=_starts(ln))
                        rec["dst_cap"] = ln
                        stream = torch.empty(int(ln.sum()), dtype=torch.uint8, device=dev)
                        mk = torch.zeros((n, mpf, 32), dtype=torch.uint8, device=dev)
                        _d, seg_len2, status = enc.encode(raw[:n * fb], dst=stream, records=rec, marks=mk.view(-1),
                                                          first=np.arange(n, dtype=np.int64) * mpf, rows_per_mark=self.rows_per_mark)
                        checks.append((torch.stack([seg_len2, status]), ln, f"{self.sources[j]}: {key} from step {t0}"))
                        streams.append(stream)
                        marks.append(mk)
                        lens.append(ln)
                        self._held_bytes += int(stream.numel() + mk.numel())
                        self.encode_stats["device"] += n
                    self._held[(j, k)] = (streams, marks, np.concatenate(lens))
                    nbytes.append(int(sum(int(l.sum()) for l in lens)))
            for meta, ln, where in checks:                            # read back once per source
                meta = meta.cpu().numpy()
                if meta[1].any() or not np.array_equal(meta[0], ln):
                    raise RuntimeError(f"{where}: the marked encode gave status {meta[1].tolist()} and lengths {meta[0].tolist()} in windows "
                                       f"of the lengths {ln.tolist()} the first launch gave")
            out[j] = headers[j]._replace(encoded=((tuple(nbytes), mpf), None))
        torch.cuda.synchronize(dev)
        return out

    def _load_encoded(self, kind, T, j, k):
        """one camera's block of an encoded source: the held segments and marks copied into its stream and mark block, device to
        device, its rows of the frame tables filled; the held tensors are released"""
        from . import ops
        q = self.layout.all_kinds.index(kind)
        tab = self._ptab[q]
        H, W = kind.shape[:2]
        dec = self._decoders.get((H, W))
        if dec is None:
            dec = self._decoders[(H, W)] = ops.JpegDecoder(self.device, H, W, max_frames=self.decode_frames)
        streams, marks, lens = self._held.pop((j, k))
        row0 = int(self._frame_row(q, j, k))
        s0, cap = int(kind.src_block_off[j, k]), int(kind.stream_cap[j, k])
        m0, mpf = int(kind.mark_off[j, k]), int(kind.marks_per_frame)
        if len(lens) != T or int(lens.sum()) != cap or any(int(m.shape[1]) != mpf for m in marks) or m0 % 32:
            raise RuntimeError(f"{self.sources[j]}: the encoded block of camera {k} does not fit the plan")
        o, t = s0, 0
        for stream, mk in zip(streams, marks):
            self.arena[o:o + stream.numel()].copy_(stream)
            self.arena[m0 + t * mpf * 32:m0 + (t + mk.shape[0]) * mpf * 32].copy_(mk.view(-1))
            self._held_bytes -= int(stream.numel() + mk.numel())
            o, t = o + int(stream.numel()), t + int(mk.shape[0])
        rows = row0 + np.arange(T, dtype=np.int64)
        rec = tab["rec"]
        rec["seg_len"][rows], rec["seg_off"][rows] = lens, s0 + _starts(lens)
        rec["restart_interval"][rows], rec["table_set"][rows] = 0, dec.table_index(self._encoder_tables)
        tab["first"][rows] = (m0 + np.arange(T, dtype=np.int64) * mpf * 32) // 32
        tab["mode"][rows] = ops.JPEG_MODES[self.encode_subsampling]
        self.stream_bytes_used += cap

    # ---- raw depth packed at load (depth_pack) ---------------------------------------------------------------------------
    def _pack_depth_sources(self, headers, cams):
        """The pack stage, beside ``_encode_sources`` and like it ahead of ``plan_store``.  Every depth entry of a raw source is read
        ONCE, at most ``decode_frames`` frames a piece, converted as ``_stage_frames`` converts depth (an unsigned integer of at most
        16 bits as uint16, channel 0 of 3-D frames) and staged through the pinned pair into a device buffer.  Per piece: one
        actmi_op_depth_pack launch with empty windows gives every frame's true length, the lengths are read back once, and one launch
        with exact windows writes the streams back to back into a tensor of their size, held until ``_load_packed_depth`` copies it
        into the arena.  -> the headers, a raw source's ``encoded[1]``: (the exact stream bytes per depth camera, 0 marks)."""
        from . import ops
        dev = torch.device(self.device)
        names, kind = cams[1], _KINDS[1]
        todo = [j for j, h in enumerate(headers) if not h.compressed and h.frames[1] is not None]
        if not todo or not names:
            return headers
        H, W = headers[todo[0]].frames[1][0]
        fb = 2 * H * W
        per = min(self.decode_frames, max(headers[j].T for j in todo))
        staging = per * fb + max(4, ops.depth_pack_workspace_bytes(per, H))
        self._encode_staging = max(self._encode_staging, staging)     # the camera stage's buffers are released by now
        if staging > self.budget_bytes:
            raise MemoryError(f"DeviceEpisodeStore: the pack stage of depth_pack needs {staging} bytes on the device "
                              f"({staging / 2**30:.2f} GiB) for {per} frames a launch, the budget is {self.budget_bytes} bytes "
                              f"({self.budget_bytes / 2**30:.2f} GiB): lower decode_frames, or raise --device_dataset_gb")
        packer = ops.DepthPacker(dev, H, W, max_frames=per)
        raw = torch.empty(per * fb, dtype=torch.uint8, device=dev)
        self._open_staging(max(self.stage_bytes, fb))
        step = max(1, self._pin[0].numel() // fb)
        out = list(headers)
        for j in todo:
            T, nbytes, checks = headers[j].T, [], []
            with open_episode(self.sources[j]) as raw_root:
                root = _EpisodeArrays(raw_root)
                for k, cam in enumerate(names):
                    key = f"/observations/{kind.key}/{cam}"
                    entry, where = root[key], f"{self.sources[j]}: {key}"
                    streams, lens = [], []
                    for t0 in range(0, T, per):
                        n = min(per, T - t0)
                        piece = np.asarray(entry[t0:t0 + n])
                        if piece.dtype.kind != "u" or piece.dtype.itemsize > 2:
                            raise ValueError(f"{where} is {piece.dtype}: not raw depth (an unsigned integer of at most 16 bits)")
                        if piece.ndim == 4:
                            piece = piece[..., 0]                     # _depth_data: a 3-D frame keeps channel 0
                        piece = piece.astype(np.uint16, copy=False)
                        if piece.shape != (n, H, W):
                            raise ValueError(f"{where}: frames {piece.dtype} {piece.shape[1:]}, the store was sized for {(H, W)}")
                        for i0 in range(0, n, step):
                            flat = np.ascontiguousarray(piece[i0:i0 + step]).reshape(-1).view(np.uint8)
                            self._stage(i0 * fb, flat.size, lambda view, flat=flat: np.copyto(view, flat), raw)
                        ln = packer.sizes(raw[:n * fb], n)            # the one read-back of the piece
                        rec = ops.depth_pack_records(n, H, W, 0, dst_off=_starts(ln))
                        rec["dst_cap"] = ln
                        stream = torch.empty(int(ln.sum()), dtype=torch.uint8, device=dev)
                        seg_len2, status = packer.pack(raw[:n * fb], rec, stream)
                        checks.append((torch.stack([seg_len2, status]), ln, f"{where} from step {t0}"))
                        streams.append(stream)
                        lens.append(ln)
                        self._held_bytes += int(stream.numel())
                        self.depth_pack_stats["frames"] += n
                        self.depth_pack_stats["raw_bytes"] += n * fb
                        self.depth_pack_stats["stream_bytes"] += int(ln.sum())
                    self._held_depth[(j, k)] = (streams, np.concatenate(lens))
                    nbytes.append(int(sum(int(l.sum()) for l in lens)))
            for meta, ln, where in checks:                            # read back once per source
                meta = meta.cpu().numpy()
                if meta[1].any() or not np.array_equal(meta[0], ln):
                    raise RuntimeError(f"{where}: the depth pack gave status {meta[1].tolist()} and lengths {meta[0].tolist()} in windows "
                                       f"of the lengths {ln.tolist()} the first launch gave")
            cam_part = out[j].encoded[0] if out[j].encoded is not None else None
            out[j] = out[j]._replace(encoded=(cam_part, (tuple(nbytes), 0)))
        torch.cuda.synchronize(dev)
        return out

    def _load_packed_depth(self, kind, T, j, k):
        """one depth camera's block of a packed source: the held streams copied into its stream block, device to device, its rows of
        the frame table filled (``DEPTH_PACK_MODE``: ``_packed_segments`` gives these rows to the depth unpack); the held tensors
        are released"""
        q = self.layout.all_kinds.index(kind)
        tab = self._ptab[q]
        streams, lens = self._held_depth.pop((j, k))
        row0 = int(self._frame_row(q, j, k))
        s0, cap = int(kind.src_block_off[j, k]), int(kind.stream_cap[j, k])
        if len(lens) != T or int(lens.sum()) != cap:
            raise RuntimeError(f"{self.sources[j]}: the packed block of depth camera {k} does not fit the plan")
        o = s0
        for stream in streams:
            self.arena[o:o + stream.numel()].copy_(stream)
            self._held_bytes -= int(stream.numel())
            o += int(stream.numel())
        rows = row0 + np.arange(T, dtype=np.int64)
        tab["rec"]["seg_len"][rows], tab["rec"]["seg_off"][rows] = lens, s0 + _starts(lens)
        tab["mode"][rows] = DEPTH_PACK_MODE
        self.stream_bytes_used += cap
        self.decode_stats["device"] += T

    def _spill_frame(self, q, row, buf, kind, where):
        """a frame the device does not take: decoded by ``imdecode_bgr`` (a bad file raises what it raises today), kept raw"""
        piece = imdecode_bgr(buf)[None]
        if kind.is_depth:
            if piece.ndim == 4:
                piece = piece[..., 0]
            piece = piece.astype(np.uint16, copy=False)
        if piece.shape != (1,) + tuple(kind.shape):
            raise ValueError(f"{where}: frames {piece.dtype} {piece.shape[1:]}, the store was sized for {tuple(kind.shape)}")
        tab = self._ptab[q]
        tab["mode"][row], tab["spill"][row] = -1, len(self._spill_host[q])
        self._spill_host[q].append(np.ascontiguousarray(piece).reshape(-1).view(np.uint8))
        self.decode_stats["host"] += 1

    def _finish_index(self):
        """the statuses of a source file's index launches, read back once; a frame whose status is not 0 becomes a spill frame"""
        if not self._index_pending:
            return
        status = torch.cat([p[0] for p in self._index_pending]).cpu().numpy()
        n = 0
        for _st, q, rows, bufs, kind, where in self._index_pending:
            for row, buf in zip(rows, bufs):
                if status[n]:
                    self._spill_frame(q, int(row), buf, kind, where)
                else:
                    self.decode_stats["device"] += 1
                n += 1
        self._index_pending = []

    def _seal_packed(self):
        """after the load: the spill tensors, the sticky status word and the decoders' workspaces (the largest sampling mode's,
        ``decode_frames`` slots), allocated once; the spill frames count against the budget like the arena"""
        from . import ops
        dev = self.arena.device
        for kind, frames in zip(self.layout.all_kinds, self._spill_host):
            flat = np.stack(frames) if frames else np.zeros((0, max(kind.frame_bytes, 1)), dtype=np.uint8)
            self._spill.append(torch.from_numpy(flat).to(dev))
        self._spill_host = None
        self._sticky = torch.zeros(1, dtype=torch.int32, device=dev)
        self._depth_sticky = torch.zeros(1, dtype=torch.int32, device=dev) if self.depth_pack else None
        for dec in self._decoders.values():
            need = max(dec.workspace_bytes(m) for m in ops.JPEG_MODES)
            dec._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        spill = sum(int(s.numel()) for s in self._spill)
        if self.nbytes + spill > self.budget_bytes:
            raise MemoryError(f"DeviceEpisodeStore: the compressed store and its spill frames need {self.nbytes + spill} bytes on the "
                              f"device, the budget is {self.budget_bytes} bytes: train without --store_compressed, or raise --device_dataset_gb")

    def check_decoded(self):
        """reads the sticky status word of every batch decoded so far (one small copy; call it where the step synchronises anyway):
        ``RuntimeError`` naming the status if a marked decode flagged a frame (``ops.JPEG_STATUS``), or -- the sticky word of the
        packed depth, read beside it -- if a depth unpack flagged a row (``ops.DEPTH_PACK_STATUS``)"""
        if self._sticky is None:
            return
        from . import ops
        v = int(self._sticky.item())
        if v:
            raise RuntimeError(f"DeviceEpisodeStore: a batch of the compressed store was decoded with status {v} ({ops.JPEG_STATUS.get(v, '?')})")
        v = int(self._depth_sticky.item()) if self._depth_sticky is not None else 0
        if v:
            raise RuntimeError(f"DeviceEpisodeStore: the packed depth of a batch was unpacked with status {v} "
                               f"({ops.DEPTH_PACK_STATUS.get(v, '?')})")

    def _packed_segments(self, e, t):
        """the JPEG side of a batch's index table: per kind and sampling mode present the records (dst_off = item * frame bytes) and
        the mark indices of the compressed items, with twins the scratch offsets of all items -> (segments, per kind the launches
        (mode, records' name, firsts' name) and the (items, spill rows) of the spill items)"""
        from . import ops
        lay, seg, plan = self.layout, {}, []
        modes = {v: m for m, v in ops.JPEG_MODES.items()}
        j = lay.src_of[e]
        for q, kind in enumerate(lay.all_kinds):
            K = len(kind.cams)
            if not K:
                plan.append(([], None))
                continue
            ksrc = self._src_cam[q][e]                                                    # [B, K]
            rows = (lay.src_row0[j][:, None] * K + ksrc * lay.src_T[j][:, None] + t[:, None]).reshape(-1)
            tab = self._ptab[q]
            mode = tab["mode"][rows]
            launches = []
            for m in np.unique(mode[mode >= 0]):
                items = np.nonzero(mode == m)[0]
                if m == DEPTH_PACK_MODE:                              # packed depth: the unpack's records, a twin's flip as their flag
                    rec = np.zeros(len(items), dtype=ops.depth_unpack_frame_dtype())
                    src = tab["rec"][rows[items]]
                    rec["seg_off"], rec["seg_len"], rec["dst_off"] = src["seg_off"], src["seg_len"], items * kind.frame_bytes
                    rec["flags"] = kind.flip[e].reshape(-1)[items].astype(np.int32) * ops.DEPTH_FLIP
                    seg[f"dpack{q}"] = rec
                    launches.append((None, f"dpack{q}", None))
                    continue
                rec = tab["rec"][rows[items]]
                rec["dst_off"] = items * kind.frame_bytes
                seg[f"jpeg{q}_{m}"], seg[f"first{q}_{m}"] = rec, tab["first"][rows[items]]
                launches.append((modes[int(m)], f"jpeg{q}_{m}", f"first{q}_{m}"))
            sp = np.nonzero(mode < 0)[0]
            if self.has_twins and not (len(mode) and (mode == DEPTH_PACK_MODE).all()):
                seg[f"scratch{q}"] = np.arange(len(rows), dtype=np.int64) * kind.frame_bytes
            plan.append((launches, (sp, tab["spill"][rows[sp]]) if len(sp) else None))
        return seg, plan

    def _decode_frames(self, q, kind, seg, plan, flips, flip0, B, nontemporal):
        """the frames of `kind` of a batch of a compressed store: one marked decode per sampling mode present, straight into the
        batch tensor -- with twins into a persistent scratch block of its shape, which the mirrored gather then reads"""
        from . import ops
        dev = self.arena.device
        K, fb = len(kind.cams), kind.frame_bytes
        out = torch.empty((B, K) + ((1,) if kind.is_depth else ()) + kind.shape, dtype=kind.torch_dtype, device=dev)
        target = out
        launches, spill = plan
        if len(launches) == 1 and launches[0][0] is None and spill is None:
            # packed depth: ONE unpack launch straight into the batch tensor, mirrored rows by the records' flag -- no scratch block
            ops.depth_unpack_raw(self.arena, seg[launches[0][1]].view(torch.uint8), out.view(torch.uint8).reshape(-1), kind.shape[0],
                                 kind.shape[1], sticky=self._depth_sticky)
            return out
        if self.has_twins:
            if q not in self._scratch or self._scratch[q].numel() < B * K * fb:
                self._scratch[q] = torch.empty(B * K * fb, dtype=torch.uint8, device=dev)
            target = self._scratch[q][:B * K * fb]
        H, W = kind.shape[:2]
        dec = self._decoders[(H, W)]
        marks = self.arena[:self.nbytes // 32 * 32]
        for mode, rec, first in launches:
            dec.decode_marked(self.arena, seg[rec].view(torch.uint8), marks, seg[first], mode, kind.decode_as, target, sticky=self._sticky,
                              rows_per_mark=self.rows_per_mark)
        if spill is not None:                                         # rare, and plumbing
            items, srows = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in spill)
            target.view(torch.uint8).view(B * K, fb)[items] = self._spill[q][srows]
        if self.has_twins:
            aligned = kind.aligned if kind.shape[1] % kind.row_unit == 0 else 0
            aligned = 2 if (nontemporal and aligned) else aligned
            ops.gather_frames_mirror(target, seg[f"scratch{q}"], flips[flip0:flip0 + B * K], H, W, kind.px_bytes, out=out, aligned=aligned)
        return out

    # ---- batches --------------------------------------------------------------------------------------------------
    def device_bytes(self):
        """bytes of device memory the store holds"""
        packed = 0
        if self.store_compressed:
            packed = sum(int(s.numel()) for s in self._spill) + 4 + (4 if self._depth_sticky is not None else 0) + sum(int(s.numel()) for s in self._scratch.values()) + \
                sum(int(d._ws.numel()) + (int(d._tables.numel()) if d._tables is not None else 0) for d in self._decoders.values())
        return int(self.arena.numel() + self.actions.numel() * 4 + self.qpos.numel() * 4 + self.episodes.numel() +
                   sum(s.numel() * 4 for s in self._stats)) + packed

    def frame_offsets(self, local_episode, t):
        """byte offsets into the arena of the frames of samples (local_episode[b], t[b]) -> ([B, K], [B, Kd]) int64"""
        if self.store_compressed:
            raise ValueError("DeviceEpisodeStore.frame_offsets: a compressed store holds no decoded frames to point at")
        e, t = np.asarray(local_episode, dtype=np.int64), np.asarray(t, dtype=np.int64)
        return tuple(k.block_off[e] + t[:, None] * k.frame_bytes for k in self.layout.all_kinds)

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
        (image u8 [B, K, H, W, 3], qpos f32 [B, S], action f32 [B, Q, A], is_pad bool [B, Q]), then with depth (depth uint16
        [B, Kd, 1, H, W]), or with stored clouds the three entries of ``collate_pcd``.  ONE index upload (``batch_table``), then the
        clouds' launch if any, the frames, the chunks, the depth frames if any.  A store that holds a twin gathers frames and depth with
        ``ops.gather_frames_mirror``; one without launches what it always did.
        ``nontemporal``: the 16-byte form reads the arena with non-temporal loads -- measured 0.77-0.87 of the plain loads' time at
        B = 64 and level with them at B = 8 (profiles/device_dataset_time.json); the bytes are the same either way"""
        from . import ops
        e, t = np.asarray(local_episode, dtype=np.int64).reshape(-1), np.asarray(t, dtype=np.int64).reshape(-1)
        B = len(e)
        if B < 1 or len(t) != B:
            raise ValueError(f"DeviceEpisodeStore.gather: {B} episodes, {len(t)} steps")
        if e.min() < 0 or e.max() >= len(self.paths) or t.min() < 0 or np.any(t >= self.T[e]):
            raise IndexError("DeviceEpisodeStore.gather: a sample outside the stored episodes")
        lay = self.layout
        extra, plan = self._packed_segments(e, t) if self.store_compressed else (None, None)
        table = batch_table(lay, e, t, self.cloud_n, extra)
        with torch.cuda.device(self.arena.device):
            seg = table.slices(self._upload(table.host))
            clouds = ()
            if self.has_clouds:
                # P: the batch's largest stored row count, as ``collate_pcd`` pads; the 16-byte form where P allows it (torch's
                # allocations are 16-byte aligned).  The twins' ``cloud_mirror`` rule -- one for the whole store -- is the launch's
                P = int(lay.src_N[lay.src_of[e]].max())
                mirror = None if self.cloud_mirror is None else (self.cloud_mirror[0], self.cloud_mirror[2])
                clouds = ops.gather_clouds(self.arena, seg["cloud_items"], P, self.cloud_rgb_fmt, mirror=mirror,
                                           aligned=(2 if nontemporal else 1) if P % 4 == 0 else 0)
            flips = seg["flips"].view(torch.uint8) if self.has_twins else None
            if self.store_compressed:
                image = self._decode_frames(0, self.kinds[0], seg, plan[0], flips, 0, B, nontemporal)
            else:
                image = self._gather_frames(self.kinds[0], seg, flips, 0, B, nontemporal)
            qpos, action, is_pad = ops.gather_chunks(self.actions, self.qpos, self.episodes, seg["samples"].view(torch.int32).view(B, 2),
                                                     *self._stats, Q)
            if self.store_compressed:
                depth = tuple(self._decode_frames(1, kind, seg, plan[1], flips, B * self.K, B, nontemporal) for kind in self.kinds[1:])
            else:
                depth = tuple(self._gather_frames(kind, seg, flips, B * self.K, B, nontemporal) for kind in self.kinds[1:])
        return (image, qpos, action, is_pad) + clouds + depth

    def _gather_frames(self, kind, seg, flips, flip0, B, nontemporal):
        """the one launch of a batch's frames of `kind`; `flips`: the batch's flags (a store with twins), this kind's from `flip0`"""
        from . import ops
        out = torch.empty((B, len(kind.cams)) + ((1,) if kind.is_depth else ()) + kind.shape, dtype=kind.torch_dtype, device=self.arena.device)
        # the mirrored gather's aligned form also states rows of whole 16- / 8-pixel groups
        aligned = kind.aligned if not self.has_twins or kind.shape[1] % kind.row_unit == 0 else 0
        aligned = 2 if (nontemporal and aligned) else aligned
        if self.has_twins:
            H, W = kind.shape[:2]
            ops.gather_frames_mirror(self.arena, seg[kind.segment], flips[flip0:flip0 + B * len(kind.cams)], H, W, kind.px_bytes, out=out,
                                     aligned=aligned)
        else:
            ops.gather_frames(self.arena, seg[kind.segment], kind.frame_bytes, out=out, aligned=aligned)
        return out

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
