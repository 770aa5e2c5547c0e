"""Box-scaled strength on the CPU: the host call vd_cell_level against the numpy definition
(cells_ref.py), properties of that definition, the new C entry points and the argument checks
of the Python layers (no GPU)."""
import ctypes

import numpy as np
import pytest

import cells_ref as cr
import mask_ref as mr
from oracle import mosaic as omosaic


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- vd_cell_level ---------------------------------------------------------------------

BIG_SIDES = (32767, 32768, 32769, 2**31 - 1)


def test_cell_level_matches_the_reference():
    """W, H in 1..400 (a stride-7 grid of pairs plus every square and every 1 x H, W x 1), the
    sizes around the 32768 clamp and 2^31 - 1, cells 2..64, level in {1, 8, 40000}."""
    from vdmi import _lib
    lib = _lib.load()
    f = lib.vd_cell_level
    small = list(range(1, 401))
    pairs = [(s, s) for s in small] + [(1, s) for s in small] + [(s, 1) for s in small]
    pairs += [(a, b) for a in small[::7] for b in small[::7]]
    pairs += [(a, b) for a in BIG_SIDES for b in (1, 400) + BIG_SIDES] + [(7, a) for a in BIG_SIDES]
    for cells in range(2, 65):
        for lvl in (1, 8, 40000):
            for W, H in pairs:
                got = f(W, H, lvl, cells)
                if got != cr.level(W, H, lvl, cells):
                    raise AssertionError((W, H, lvl, cells, got, cr.level(W, H, lvl, cells)))
    assert _lib.cell_level(480, 300, 8, 16) == 30 and _lib.cell_level(64, 64, 8, 16) == 8
    assert _lib.cell_level(50, 37, 1, 6) == 9
    assert _lib.cell_level(2**31 - 1, 5, 8, 64) == 32768 and _lib.cell_level(32768 * 2 + 1, 5, 8, 2) == 32768
    assert _lib.cell_level(32768 * 2, 5, 8, 2) == 32768 and _lib.cell_level(32768 * 2 - 2, 5, 8, 2) == 32767


def test_cell_level_of_empty_and_inverted_boxes_and_cells_off():
    from vdmi import _lib
    for W, H in [(0, 10), (10, 0), (-5, 10), (10, -2**31), (0, 0), (-1, -1)]:
        for cells in (0, 2, 16, 64):
            assert _lib.cell_level(W, H, 8, cells) == 8 == cr.level(W, H, 8, cells)
    for W, H in [(1, 1), (480, 300), (2**31 - 1, 2**31 - 1)]:
        for lvl in (1, 8, 40000):
            assert _lib.cell_level(W, H, lvl, 0) == lvl == cr.level(W, H, lvl, 0)


@pytest.mark.parametrize("cells", [1, 65, -3])
def test_cell_level_refuses_bad_cells(cells):
    from vdmi import _lib
    assert _lib.load().vd_cell_level(100, 100, 8, cells) == _lib.VD_ERR_ARG
    with pytest.raises(_lib.VdError):
        _lib.cell_level(100, 100, 8, cells)


def test_cell_level_refuses_level_0():
    from vdmi import _lib
    assert _lib.load().vd_cell_level(100, 100, 0, 16) == _lib.VD_ERR_ARG
    assert _lib.load().vd_cell_level(100, 100, -8, 0) == _lib.VD_ERR_ARG


# ---- properties of the reference ------------------------------------------------------

def _edge_and_oversized():
    h, w = mr.EDGE_HW
    return list(mr.EDGE_BOXES) + [(-500, -500, 600, 600), (-3, -3, w + 3, h + 3), (0, 0, w, h),
                                  (-40000, 10, 40000, 30), (10, -70000, 30, 70000), (5, 5, 6, 6), (99, 71, 100, 72)]


@pytest.mark.parametrize("cells", [2, 6, 16, 64])
@pytest.mark.parametrize("lvl", [1, 8])
def test_grid_never_exceeds_cells(cells, lvl):
    """sw, sh <= cells on boxes clipped by every edge, boxes larger than the frame and 1-px
    boxes: the clipped sides are at most max(W, H) <= L * cells."""
    h, w = mr.EDGE_HW
    seen = 0
    for b in _edge_and_oversized():
        g = cr.grid(b, h, w, lvl, cells)
        if g is None:
            continue
        assert 1 <= g[0] <= cells and 1 <= g[1] <= cells, (b, g)
        seen += 1
    assert seen >= 10


def test_pixelation_is_never_weaker_than_the_base_level():
    for W, H in [(1, 1), (64, 64), (480, 300), (5, 900)]:
        for cells in (2, 16, 64):
            L = cr.level(W, H, 8, cells)
            assert L >= 8 and (max(W, H) + L - 1) // L <= max(cells, (max(W, H) + 7) // 8)
    img = _img(40, 56, 0)
    boxes = [(5, 4, 30, 20), (20, 10, 55, 39), (-3, 25, 12, 60), (9, 9, 9, 12)]
    np.testing.assert_array_equal(cr.mosaic_frame_cells(img, boxes, 8, 0), omosaic.mosaic_frame(img, boxes, 8))
    # small boxes under a base level that already gives fewer cells: the old result
    np.testing.assert_array_equal(cr.mosaic_frame_cells(img, boxes, 8, 64), omosaic.mosaic_frame(img, boxes, 8))
    assert not np.array_equal(cr.mosaic_frame_cells(img, boxes, 8, 2), omosaic.mosaic_frame(img, boxes, 8))


def test_f_1_is_the_identity():
    img = _img(24, 36, 1)
    np.testing.assert_array_equal(cr.smooth_region(img, 1), img)
    # level 1 and boxes of at most `cells` px: f = 1
    np.testing.assert_array_equal(cr.smooth_frame(img, [(2, 3, 30, 20), (0, 0, 36, 24)], 1, 64), img)


@pytest.mark.parametrize("f", [1, 2, 3, 7, 8, 9, 16, 50])
def test_constants_are_preserved_and_outputs_stay_in_range(f):
    const = np.empty((23, 31, 3), np.uint8)
    const[:] = (0, 137, 255)
    np.testing.assert_array_equal(cr.smooth_region(const, f), const)
    reg = _img(23, 31, f)
    out = cr.smooth_region(reg, f)
    for c in range(3):
        assert reg[..., c].min() <= out[..., c].min() and out[..., c].max() <= reg[..., c].max()
    # the extremes of the arithmetic
    for v in (0, 255):
        flat = np.full((9, 40, 3), v, np.uint8)
        np.testing.assert_array_equal(cr.smooth_region(flat, f), flat)


def test_smooth_frame_touches_only_the_clipped_boxes():
    h, w = mr.EDGE_HW
    img = _img(h, w, 2)
    boxes = list(mr.EDGE_BOXES)
    out = cr.smooth_frame(img, boxes, 8, 6)
    hit = np.zeros((h, w), bool)
    for b in boxes:
        c = mr.clip(b, h, w)
        if c:
            hit[c[1]:c[3], c[0]:c[2]] = True
    np.testing.assert_array_equal(out[~hit], img[~hit])
    assert (out[hit] != img[hit]).any()


def test_strongest_wins_whatever_the_order_and_ties_go_to_the_lower_index():
    img = _img(72, 100, 3)
    big, small = (5, 5, 95, 65), (30, 20, 50, 40)                     # f = 15 and f = 4 under (1, 6)
    assert cr.box_level(big, 1, 6) == 15 and cr.box_level(small, 1, 6) == 4
    a = cr.smooth_frame(img, [big, small], 1, 6)
    b = cr.smooth_frame(img, [small, big], 1, 6)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, cr.smooth_frame(img, [big], 1, 6))   # the small box never shows
    # equal f, crossing: the overlap belongs to whichever comes first
    p, q = (10, 10, 58, 40), (40, 20, 88, 50)
    assert cr.box_level(p, 1, 6) == cr.box_level(q, 1, 6) == 8
    pq, qp = cr.smooth_frame(img, [p, q], 1, 6), cr.smooth_frame(img, [q, p], 1, 6)
    only_p, only_q = cr.smooth_frame(img, [p], 1, 6), cr.smooth_frame(img, [q], 1, 6)
    np.testing.assert_array_equal(pq[20:40, 40:58], only_p[20:40, 40:58])
    np.testing.assert_array_equal(qp[20:40, 40:58], only_q[20:40, 40:58])
    assert not np.array_equal(pq, qp)


def test_rect_fn_shape_for_the_mask_composite():
    img = _img(48, 64, 4)
    boxes = [(10, 8, 50, 38)]
    fn = lambda im, bl: cr.smooth_frame(im, bl, 8, 4)
    out = mr.shaped_frame(img, boxes, "ellipse", 30, fn)
    grown = mr.grow_list(boxes, 30)
    R = fn(img, grown)
    np.testing.assert_array_equal(out[23, 30], R[23, 30])
    gx1, gy1 = max(0, grown[0][0]), max(0, grown[0][1])
    np.testing.assert_array_equal(out[gy1, gx1], img[gy1, gx1])     # the grown box's corner shows the input


# ---- the C entry points and the Python layers -----------------------------------------

def test_symbols_are_exported_and_bound():
    from vdmi import _lib
    lib = _lib.load()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    P, I, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert sig["vd_cells"] == (I, [P, I])
    assert sig["vd_cell_level"] == (I, [I, I, I, I])
    assert sig["vd_smooth"] == (I, [P, P, P, I, I, I, SZ, I, ctypes.POINTER(_lib.vd_boxes), I, I])
    assert lib.vd_cells.argtypes == [P, I] and lib.vd_cells.restype is I
    assert (_lib.VD_CELLS_MIN, _lib.VD_CELLS_MAX) == (2, 64)
    assert lib.vd_abi_version() == 2
    assert lib.vd_cells(None, 16) == _lib.VD_ERR_ARG                                  # null context
    hb = _lib.HostBoxes(1, 1)
    s = hb.struct()
    assert lib.vd_smooth(None, None, None, 1, 8, 8, 24, 0, ctypes.byref(s), 8, 16) == _lib.VD_ERR_ARG


def test_header_declares_the_contract():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "vdmi.h")).read()
    for needle in ("#define VD_CELLS_MIN 2", "#define VD_CELLS_MAX 64", "int vd_cells(vd_ctx* ctx, int cells);",
                   "int vd_cell_level(int W, int H, int level, int cells);", "int vd_smooth(vd_ctx* ctx,",
                   "#define VDMI_ABI_VERSION 2", "int32_t reserved[1];"):
        assert needle in text, needle


@pytest.mark.parametrize("cells", [1, 65, -3])
def test_bad_cells_raise_before_the_library_is_touched(cells, tmp_path):
    import vdmi
    from vdmi import _lib
    from vdmi.pipeline import batch_process_images
    with pytest.raises(ValueError, match="cells"):
        _lib.check_cells(cells)
    with pytest.raises(ValueError, match="cells"):
        vdmi.Context(cells=cells)
    with pytest.raises(ValueError, match="cells"):
        vdmi.Retinaface(weights="random", cells=cells)
    (tmp_path / "in").mkdir()
    with pytest.raises(ValueError, match="cells"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), object(), object(), cells=cells)


def test_check_cells_accepts_the_range():
    from vdmi import _lib
    assert _lib.check_cells(0) == 0 and _lib.check_cells(2) == 2 and _lib.check_cells(64) == 64
    assert _lib.check_cells(np.int64(16)) == 16
