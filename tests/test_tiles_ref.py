"""Tiled detection, CPU side: the tile geometry (vd_tile_rects, host only) against the numpy
reference and its stated properties, the argument errors, the exports, and hand-made cases of
the reference merge (tests/tiles_ref.py) that the GPU tests compare the kernel against."""
import ctypes

import numpy as np
import pytest

import tiles_ref

F32 = np.float32
VIDEO_SIZES = [480, 576, 640, 720, 1080, 1280, 1440, 1920, 2160, 2560, 3840, 4096, 4320, 7680, 8192, 16384, 32768]
LENGTHS = list(range(1, 400)) + VIDEO_SIZES
OVERLAPS = [0, 1, 10, 20, 33, 50]


def test_axis_properties_over_the_sweep():
    """First tile at 0, last ends at L, origins never decrease, no gap between neighbours, and
    whenever t < L neighbours overlap by at least floor(L * O / (100 * K))."""
    for L in LENGTHS:
        for K in range(1, 5):
            for O in OVERLAPS:
                t, org = tiles_ref._axis(L, K, O)
                assert 1 <= t <= L
                assert org[0] == 0 and org[-1] + t == L, (L, K, O)
                for a, b in zip(org, org[1:]):
                    assert a <= b, (L, K, O)
                    assert b <= a + t, (L, K, O)                       # no gap
                    if t < L:
                        assert a + t - b >= (L * O) // (100 * K), (L, K, O)


def test_issue_examples():
    r = tiles_ref.tile_rects(2160, 3840, 2, 2, 20)
    assert r.tolist() == [[0, 0, 3840, 2160], [0, 0, 2304, 1296], [1536, 0, 2304, 1296], [0, 864, 2304, 1296],
                          [1536, 864, 2304, 1296]]
    r = tiles_ref.tile_rects(1080, 1920, 2, 3, 25)
    assert (r[1:, 2] == 800).all() and (r[1:, 3] == 675).all()
    assert r[1:4, 0].tolist() == [0, 560, 1120] and r[[1, 4], 1].tolist() == [0, 405]


def test_vd_tile_rects_equals_reference_on_the_sweep():
    from vdmi import _lib
    lib = _lib.load()
    out = np.zeros((17, 4), np.int32)
    cnt = ctypes.c_int()
    sizes = [(L, L2) for L, L2 in zip(LENGTHS, LENGTHS[::-1])] + [(L, 7) for L in LENGTHS[::9]]
    for h, w in sizes:
        for rows, cols in ((1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 4), (4, 4), (4, 1), (3, 3)):
            for O in OVERLAPS:
                assert lib.vd_tile_rects(h, w, rows, cols, O, out.ctypes.data, ctypes.byref(cnt)) == _lib.VD_OK
                ref = tiles_ref.tile_rects(h, w, rows, cols, O)
                assert cnt.value == len(ref) == 1 + rows * cols
                assert np.array_equal(out[:cnt.value], ref), (h, w, rows, cols, O)
    assert np.array_equal(_lib.tile_rects(2160, 3840, (2, 2), 20), tiles_ref.tile_rects(2160, 3840, 2, 2, 20))


@pytest.mark.parametrize("args", [(0, 10, 2, 2, 20), (10, 0, 2, 2, 20), (-1, 10, 1, 1, 0), (10, 10, 0, 2, 20),
                                  (10, 10, 5, 2, 20), (10, 10, 2, 0, 20), (10, 10, 2, 5, 20), (10, 10, 2, 2, -1),
                                  (10, 10, 2, 2, 51)])
def test_vd_tile_rects_argument_errors(args):
    from vdmi import _lib
    lib = _lib.load()
    out = np.full((17, 4), -7, np.int32)
    cnt = ctypes.c_int(-7)
    assert lib.vd_tile_rects(*args, out.ctypes.data, ctypes.byref(cnt)) == _lib.VD_ERR_ARG
    assert "vd_tile_rects" in _lib.last_error()
    assert (out == -7).all() and cnt.value == -7
    with pytest.raises(_lib.VdError):
        _lib.tile_rects(args[0], args[1], (args[2], args[3]), args[4])


def test_python_keyword_checks():
    from vdmi import _lib
    assert _lib.check_tiles((2, 3), 25) == ((2, 3), 25)
    for bad in ((0, 1), (5, 1), (1, 5), (1,), 3):
        with pytest.raises(ValueError):
            _lib.check_tiles(bad, 20)
    for ov in (-1, 51):
        with pytest.raises(ValueError):
            _lib.check_tiles((2, 2), ov)


def test_new_exports_exist():
    from vdmi import _lib
    lib = _lib.load()
    for name in ("vd_tile_rects", "vd_tiles", "vd_tiles_merge", "vdt_letterbox_tiles"):
        assert hasattr(lib, name), name
    assert lib.vd_tiles(None, 2, 2, 20) == _lib.VD_ERR_ARG                # null context, reported not raised
    assert lib.vd_tiles_merge(None, None, 1, 8, 8, None) == _lib.VD_ERR_ARG


# ---- the reference merge on hand-made cases -------------------------------------------------

def _l(boxes, scores, labels=None):
    return (np.asarray(boxes, F32).reshape(-1, 4), np.asarray(scores, F32), labels)


ORG = [(0, 0), (0, 0), (100, 0)]      # whole frame, tile at 0, tile at x = 100


def test_duplicate_across_two_tiles_keeps_the_lower_t():
    """The same face at the same score in tiles 1 and 2 (frame coordinates 110..150): one box
    survives and it is tile 1's."""
    lists = [_l([], []), _l([[110, 20, 150, 60]], [0.9], [7]), _l([[10, 20, 50, 60]], [0.9], [3])]
    xi, xf, sc, lab, src = tiles_ref.merge_frame(lists, ORG, 1000, 0.4)
    assert src == [(1, 0)] and lab.tolist() == [1007]
    assert xf.tolist() == [[110, 20, 150, 60]] and xi.tolist() == [[110, 20, 150, 60]]


def test_score_tie_orders_by_input_then_position():
    lists = [_l([[0, 0, 10, 10], [300, 0, 310, 10]], [0.75, 0.75], [1, 2]),
             _l([[200, 0, 210, 10]], [0.75], [3]),
             _l([[0, 100, 10, 110]], [0.8], [4])]
    xi, xf, sc, lab, src = tiles_ref.merge_frame(lists, ORG, 100, 0.4)
    assert src == [(2, 0), (0, 0), (0, 1), (1, 0)]
    assert lab.tolist() == [204, 1, 2, 103]
    assert xf[0].tolist() == [100, 100, 110, 110]                       # mapped by the tile's origin


def test_pair_on_either_side_of_the_iou_threshold():
    """Boxes [0, 0, 10, 10] and [0, 0, 10, k]: IoU = k / 10 in exact binary for k = 4 (0.4 as a
    float32 quotient is 0.4000000059..., > the double 0.4: suppressed) and k = 2.5 (0.25: kept);
    against thr = 0.5, k = 5 gives exactly 0.5, not > 0.5: kept."""
    def run(k, thr):
        lists = [_l([[0, 0, 10, 10]], [0.9]), _l([[0, 0, 10, k]], [0.8]), _l([], [])]
        return tiles_ref.merge_frame(lists, ORG, 10, thr)[4]
    assert run(4.0, 0.4) == [(0, 0)]
    assert run(2.5, 0.4) == [(0, 0), (1, 0)]
    assert run(5.0, 0.5) == [(0, 0), (1, 0)]
    assert run(5.0, np.nextafter(0.5, 0)) == [(0, 0)]


def test_empty_lists():
    xi, xf, sc, lab, src = tiles_ref.merge_frame([_l([], []), _l([], []), _l([], [])], ORG, 10, 0.4)
    assert len(xi) == len(xf) == len(sc) == len(lab) == 0 and src == []
    xi, xf, sc, lab, src = tiles_ref.merge_frame([_l([], []), _l([], []), _l([[1, 2, 3, 4]], [0.5], [9])], ORG, 10,
                                                 0.4)
    assert xf.tolist() == [[101, 2, 103, 4]] and lab.tolist() == [29] and src == [(2, 0)]


def test_negative_zero_is_kept_for_input_0_only():
    """Input 0 is left as it is; a tile box gets one float32 add, which turns -0.0 into +0.0."""
    lists = [_l([[-0.0, -0.0, 5, 5]], [0.9]), _l([[-0.0, 50, 5, 55]], [0.8]), _l([], [])]
    xf = tiles_ref.merge_frame(lists, ORG, 10, 0.4)[1]
    assert np.signbit(xf[0, 0]) and not np.signbit(xf[1, 0])
