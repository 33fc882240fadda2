"""The GPU-free parts of the device-resident episode store (actmi/episode_store.py): ``plan_store`` on hand-made header records, the
index table of a batch, and the direction of the imports between the three input-pipeline modules.  No GPU and no library: every
expected number is written out here."""
import os
import subprocess
import sys

import numpy as np
import torch

from actmi import episode_store as ES
from actmi import ops

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "act-plus-plus_amd")
CAMS = (("left", "right"), ("d",))
U8, U16, F32 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32)
FRAMES = (((4, 16, 3), U8), ((4, 16), U16))                         # 192-byte frames, 128-byte depth frames
# the twin of source 1: its "left" shows the source's "right" flipped, its "right" the source's "left" as it is; depth flipped
TWIN = (((1, True), (0, False)), ((0, True),))


def headers(rgb=(U8, U8, U8)):
    """3 sources of T = 5, 3 and 4 steps with clouds of N = 6, 9 and 6 stored rows"""
    return [ES.SourceHeader(T, False, N, dt, FRAMES) for T, N, dt in zip((5, 3, 4), (6, 9, 6), rgb)]


def layout(twin=True, **kw):
    if twin:                                                        # episodes 0, 1, 2 the files, episode 3 the twin of file 1
        return ES.plan_store(headers(**kw), CAMS, [0, 1, 2, 1], [None, None, None, TWIN])
    return ES.plan_store(headers(**kw), CAMS, [0, 1, 2])


# per source: two cameras of T * 192 bytes, one depth camera of T * 128, xyz of T * N * 12, colours of T * N * 3 (uint8)
BLOCKS = [960, 960, 640, 360, 90,
          576, 576, 384, 324, 81,
          768, 768, 512, 288, 72]


def test_plan_store_lays_out_todays_arena():
    lay = layout()
    offs, total = ES.arena_layout(BLOCKS)
    offs = offs.reshape(3, 5)
    assert offs.tolist() == [[0, 1024, 2048, 2816, 3328], [3584, 4352, 5120, 5632, 6144], [6400, 7168, 7936, 8448, 8960]]
    img, dep = lay.all_kinds
    assert lay.kinds == (img, dep) and (img.key, dep.key) == ("images", "depth_images")
    assert np.array_equal(img.src_block_off, offs[:, :2]) and np.array_equal(dep.src_block_off, offs[:, 2:3])
    assert np.array_equal(lay.src_cloud_off, offs[:, 3:]) and lay.has_clouds
    assert lay.nbytes == total == 9216
    assert lay.padding == [(960, 1024), (1984, 2048), (2688, 2816), (3176, 3328), (3418, 3584),
                           (4160, 4352), (4928, 5120), (5504, 5632), (5956, 6144), (6225, 6400),
                           (8736, 8960), (9032, 9216)]
    assert (img.cams, img.shape, img.frame_bytes, img.px_bytes, img.aligned, img.row_unit) == (("left", "right"), (4, 16, 3), 192, 3, 1, 16)
    assert (dep.cams, dep.shape, dep.frame_bytes, dep.px_bytes, dep.aligned, dep.row_unit) == (("d",), (4, 16), 128, 2, 1, 8)
    assert img.torch_dtype == torch.uint8 and dep.torch_dtype == torch.uint16
    assert (lay.cloud_rgb_fmt, lay.cloud_rgb_bytes) == (0, 3)
    assert lay.src_T.tolist() == [5, 3, 4] and lay.src_N.tolist() == [6, 9, 6] and lay.src_row0.tolist() == [0, 5, 8]


def test_plan_store_gives_a_twin_its_sources_blocks_permuted_and_flagged():
    lay = layout()
    img, dep = lay.kinds
    assert lay.twin == [False, False, False, True] and lay.has_twins and lay.src_of.tolist() == [0, 1, 2, 1]
    assert img.block_off.tolist() == [[0, 1024], [3584, 4352], [6400, 7168], [4352, 3584]]
    assert img.flip.tolist() == [[0, 0], [0, 0], [0, 0], [1, 0]] and img.flip.dtype == np.uint8
    assert dep.block_off.tolist() == [[2048], [5120], [7936], [5120]] and dep.flip.tolist() == [[0], [0], [0], [1]]
    assert lay.T.tolist() == [5, 3, 4, 3] and lay.row0.tolist() == [0, 5, 8, 12] and lay.compressed == [False] * 4
    plain = layout(twin=False)                                      # the twin added no byte
    assert plain.nbytes == 9216 and plain.padding == lay.padding and not plain.has_twins
    assert plain.row0.tolist() == [0, 5, 8] and np.array_equal(plain.kinds[0].block_off, img.block_off[:3])


def test_one_float32_colour_entry_makes_every_colour_block_float32():
    lay = layout(rgb=(U8, F32, U8))
    assert (lay.cloud_rgb_fmt, lay.cloud_rgb_bytes) == (1, 12)
    blocks = [960, 960, 640, 360, 360,
              576, 576, 384, 324, 324,
              768, 768, 512, 288, 288]
    offs, total = ES.arena_layout(blocks)
    assert lay.nbytes == total == 9984
    assert lay.src_cloud_off.tolist() == offs.reshape(3, 5)[:, 3:].tolist() == [[2816, 3328], [5888, 6400], [8960, 9472]]


def test_a_store_without_depth_or_clouds_and_frames_that_take_the_general_form():
    hs = [ES.SourceHeader(T, False, frames=(((5, 7, 3), U8), None)) for T in (2, 3)]
    lay = ES.plan_store(hs, (("top",), ()), [0, 1])
    img, dep = lay.all_kinds
    assert lay.kinds == (img,) and not lay.has_clouds and not lay.has_twins
    assert (img.frame_bytes, img.aligned) == (105, 0) and img.src_block_off.tolist() == [[0], [256]]
    assert (dep.cams, dep.shape, dep.frame_bytes, dep.aligned) == ((), None, 0, 0) and dep.block_off.shape == (2, 0)
    assert lay.nbytes == 768 and lay.padding == [(210, 256), (571, 768)] and lay.src_cloud_off.shape == (2, 0)


# ---- the index table of a batch ---------------------------------------------------------------------------------------------------
E, T_ = np.array([0, 3, 2], dtype=np.int64), np.array([4, 1, 2], dtype=np.int64)       # the second sample is the twin's
CLOUD_N = np.array([6, 5, 4, 3, 2, 9, 8, 7, 6, 1, 2, 3], dtype=np.int32)                # valid rows of the 5 + 3 + 4 stored steps


def test_batch_table_names_its_segments_in_todays_order():
    table = ES.batch_table(layout(), E, T_, CLOUD_N)
    assert table.bounds == {"frames": (0, 6), "depth": (6, 9), "samples": (9, 12), "flips": (12, 14), "cloud_items": (14, 26)}
    assert table.host.dtype == np.int64 and table.host.shape == (26,)
    seg = {name: table.host[a:b] for name, (a, b) in table.bounds.items()}
    # block_off[e] + t * frame_bytes
    assert seg["frames"].tolist() == [0 + 4 * 192, 1024 + 4 * 192, 4352 + 192, 3584 + 192, 6400 + 2 * 192, 7168 + 2 * 192]
    assert seg["depth"].tolist() == [2048 + 4 * 128, 5120 + 128, 7936 + 2 * 128]
    assert seg["samples"].view(np.int32).reshape(3, 2).tolist() == [[0, 4], [3, 1], [2, 2]]
    # a flag per frame item, then per depth item, padded to whole words
    assert seg["flips"].view(np.uint8).tolist() == [0, 0, 1, 0, 0, 0] + [0, 1, 0] + [0] * 7
    items = seg["cloud_items"].view(ops.cloud_item_dtype())
    assert items["xyz_off"].tolist() == [2816 + 4 * 6 * 12, 5632 + 1 * 9 * 12, 8448 + 2 * 6 * 12]
    assert items["rgb_off"].tolist() == [3328 + 4 * 6 * 3, 6144 + 1 * 9 * 3, 8960 + 2 * 6 * 3]
    assert items["rows"].tolist() == [6, 9, 6] and items["n"].tolist() == [2, 8, 2] and items["flags"].tolist() == [0, 1, 0]
    assert not items["pad"].any()
    assert np.array_equal(items, ES.cloud_items(layout(), E, T_, CLOUD_N))


def test_the_uploaded_table_is_cut_at_the_same_boundaries():
    table = ES.batch_table(layout(), E, T_, CLOUD_N)
    tab = torch.from_numpy(table.host.copy())                       # stands in for the uploaded tensor
    cut = table.slices(tab)
    assert list(cut) == ["frames", "depth", "samples", "flips", "cloud_items"]
    for name, (a, b) in table.bounds.items():
        assert cut[name].untyped_storage().data_ptr() == tab.untyped_storage().data_ptr()
        assert (cut[name].storage_offset(), cut[name].numel()) == (a, b - a)
        assert np.array_equal(cut[name].numpy(), table.host[a:b])
    assert cut["samples"].view(torch.int32).view(3, 2).tolist() == [[0, 4], [3, 1], [2, 2]]
    assert cut["flips"].view(torch.uint8)[:9].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0]


def test_a_layout_without_twins_uploads_no_flip_words_and_one_without_clouds_no_items():
    e = np.array([0, 1, 2], dtype=np.int64)
    table = ES.batch_table(layout(twin=False), e, T_[[0, 1, 2]], CLOUD_N)
    assert table.bounds == {"frames": (0, 6), "depth": (6, 9), "samples": (9, 12), "cloud_items": (12, 24)}
    hs = [ES.SourceHeader(T, False, frames=(((5, 7, 3), U8), None)) for T in (2, 3)]
    table = ES.batch_table(ES.plan_store(hs, (("top",), ()), [0, 1]), np.array([1, 0, 1]), np.array([2, 1, 0]))
    assert table.bounds == {"frames": (0, 3), "depth": (3, 3), "samples": (3, 6)}
    assert table.host.tolist()[:3] == [256 + 2 * 105, 105, 256]
    # a twin of a store without depth: 3 flags, one word
    lay = ES.plan_store(hs, (("top",), ()), [0, 1, 0], [None, None, (((0, True),), ())])
    table = ES.batch_table(lay, np.array([2, 0, 2]), np.array([1, 1, 0]))
    assert table.bounds == {"frames": (0, 3), "depth": (3, 3), "samples": (3, 6), "flips": (6, 7)}
    assert table.host[6:7].view(np.uint8).tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and table.host[:3].tolist() == [105, 105, 0]


# ---- one direction of imports -----------------------------------------------------------------------------------------------------
def test_the_file_and_store_modules_do_not_import_the_dataset_module():
    for mod in ("actmi.episode_files", "actmi.episode_store"):
        code = f"import sys; import {mod}; assert 'actmi.data' not in sys.modules, sorted(m for m in sys.modules if m.startswith('actmi'))"
        done = subprocess.run([sys.executable, "-c", code], cwd=PKG, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
    code = "import sys; import actmi.episode_files; assert 'actmi.episode_store' not in sys.modules and 'torch' not in sys.modules"
    done = subprocess.run([sys.executable, "-c", code], cwd=PKG, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
