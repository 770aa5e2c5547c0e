"""Box-scaled strength on the GPU (vd_cells, vd_smooth; mosaic.hip's per-box level, smooth.hip)
against the numpy definition in cells_ref.py, bit for bit and whole frames (so bytes outside the
boxes are checked too). The smooth box pass gives each box to one workgroup of 256 threads (a
box of more than 16384 px to up to 8), 32 slots per frame, with the cell sums in LDS and a list
of 128 beating boxes; the shapes below straddle those sizes."""
import ctypes

import numpy as np
import pytest

import cells_ref as cr
import mask_ref as mr
from oracle import mosaic as omosaic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    import vdmi
    c = vdmi.Context(max_batch=8)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _cells_off_afterwards(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        c.set_cells(0)
        c.set_mask("rect", 0)


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _arrays(boxes, cap=None):
    n = len(boxes)
    cap = cap or max(1, max(len(b) for b in boxes))
    xy = np.zeros((n, cap, 4), np.int32)
    cnt = np.zeros(n, np.int32)
    for i, bl in enumerate(boxes):
        cnt[i] = len(bl)
        if bl:
            xy[i, :len(bl)] = bl
    return xy, cnt


def _ref(fn, fr, boxes, lvl, cells):
    return np.stack([fn(fr[i], boxes[i], lvl, cells) for i in range(len(fr))])


def _check(ctx, fr, boxes, lvl, cells):
    """mosaic() under set_cells and smooth() of host frames and host lists against the
    reference; the input is untouched. Returns the two outputs."""
    ctx.set_cells(cells)
    xy, cnt = _arrays(boxes)
    keep = fr.copy()
    got_m = ctx.mosaic(fr, xy, cnt, level=lvl)
    got_s = ctx.smooth(fr, xy, cnt, level=lvl)
    np.testing.assert_array_equal(fr, keep)
    np.testing.assert_array_equal(got_m, _ref(cr.mosaic_frame_cells, fr, boxes, lvl, cells), err_msg="mosaic")
    np.testing.assert_array_equal(got_s, _ref(cr.smooth_frame, fr, boxes, lvl, cells), err_msg="smooth")
    return got_m, got_s


SQUARES = [(5 + 12 * s, 6, 5 + 13 * s, 6 + s) for s in (1, 2, 3, 4, 5)]
BOX_50x37 = (24, 30, 74, 67)                                       # cells = 6: f = 9, no power of two
# two frames each: edge-clipped boxes + tiny squares + the 50 x 37 box | the whole frame;
# a box far larger than the frame | the 50 x 37 box under the whole frame
LISTS = {"edges+whole": [list(mr.EDGE_BOXES) + SQUARES + [BOX_50x37], [(0, 0, 100, 72)]],
         "huge+nested": [[(-500, -500, 600, 600)], [BOX_50x37, (0, 0, 100, 72), (3, 3, 4, 4)]]}


@pytest.mark.parametrize("which", sorted(LISTS))
@pytest.mark.parametrize("lvl", [1, 8])
@pytest.mark.parametrize("cells", [2, 6, 16, 64])
def test_mosaic_and_smooth_match_the_reference(ctx, cells, lvl, which):
    h, w = mr.EDGE_HW
    assert cr.box_level(BOX_50x37, 1, 6) == 9
    _check(ctx, _frames(2, h, w, 0), LISTS[which], lvl, cells)


def test_smooth_on_device_frames_and_a_padded_pitch_view(ctx):
    """torch device frames; rows of 100 pixels in a pitch of 112 pixels: smooth() works at the
    view's pitch and the padding of `out` stays as it was."""
    import torch
    h, w = mr.EDGE_HW
    fr = _frames(2, h, w, 1)
    boxes = LISTS["edges+whole"]
    xy, cnt = _arrays(boxes)
    exp = _ref(cr.smooth_frame, fr, boxes, 8, 6)
    ctx.set_cells(6)
    d = torch.from_numpy(fr).cuda()
    got = ctx.smooth(d, xy, cnt, level=8)
    ctx.sync()
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    np.testing.assert_array_equal(d.cpu().numpy(), fr)
    for pad in (112, 101):                                           # 336-B rows (16-B aligned) and 303-B rows
        big_in = torch.full((2, h, pad, 3), 7, dtype=torch.uint8, device="cuda")
        big_out = torch.full((2, h, pad, 3), 9, dtype=torch.uint8, device="cuda")
        big_in[:, :, :w] = d
        ctx.smooth(big_in[:, :, :w], xy, cnt, level=8, out=big_out[:, :, :w])
        ctx.sync()
        got = big_out.cpu().numpy()
        np.testing.assert_array_equal(got[:, :, :w], exp)
        assert (got[:, :, w:] == 9).all()
        assert (big_in.cpu().numpy()[:, :, w:] == 7).all()


def test_overlapping_boxes(ctx):
    """A small box inside a big one in both list orders, two equal-f boxes that cross, a chain
    of four: pixelation in list order, smooth with the strongest box winning."""
    fr = _frames(4, 96, 128, 2)
    big, small = (5, 5, 95, 65), (30, 20, 50, 40)
    p, q = (10, 10, 58, 40), (40, 20, 88, 50)
    chain = [(4, 4, 40, 30), (28, 14, 66, 44), (52, 24, 92, 60), (80, 40, 126, 90)]
    assert cr.box_level(p, 1, 6) == cr.box_level(q, 1, 6) and cr.box_level(big, 1, 6) > cr.box_level(small, 1, 6)
    boxes = [[big, small], [small, big], [p, q], chain]
    _, s = _check(ctx, fr, boxes, 1, 6)
    np.testing.assert_array_equal(s[0], cr.smooth_frame(fr[0], [big], 1, 6))   # the small box never shows
    _check(ctx, fr, [[q, p], chain[::-1], [small, big, p, q], chain + [big]], 8, 2)


def test_cells_wider_than_a_row_tile_and_a_full_lds_grid(ctx):
    """600 x 900 frame, 580 x 860 box: cells = 2 gives f = 430 (one cell spans many 256-byte
    column tiles, its sum is carried across them); cells = 64 gives f = 14 and 62 x 42 cells.
    A 1-px-wide, 500-px-tall box beside it is cut into row groups."""
    fr = _frames(1, 600, 900, 3)
    boxes = [[(20, 10, 880, 590), (890, 50, 891, 550)]]
    assert cr.box_level(boxes[0][0], 8, 2) == 430 and cr.box_level(boxes[0][0], 8, 64) == 14
    assert cr.grid(boxes[0][0], 600, 900, 8, 64) == (62, 42)
    _check(ctx, fr, boxes, 8, 2)
    _check(ctx, fr, boxes, 8, 64)
    # a box of more than 16384 px is shared among workgroups by bands of cell rows: areas of
    # exactly 1 x, just under 2 x, exactly 2 x and 5.5 x that, and fewer cell rows than parts
    parts = [[(470, 20, 598, 148), (5, 5, 187, 185), (200, 10, 456, 138), (10, 200, 310, 500), (400, 200, 880, 560)]]
    assert [(b[2] - b[0]) * (b[3] - b[1]) for b in parts[0][:3]] == [16384, 32760, 32768]
    _check(ctx, fr, parts, 1, 6)
    _check(ctx, fr, parts, 8, 3)


def test_levels_past_4096_and_the_32768_clamp(ctx):
    """Boxes far larger than the frame: f = 10000 (cell sums kept in 64 bits from f = 4097 on)
    and f = 32768 where the clamp binds; the clipped box is one cell, or 2 x 2 of them."""
    h, w = mr.EDGE_HW
    fr = _frames(3, h, w, 9)
    big = 1 << 30
    boxes = [[(-10000, -10000, 10000, 10000)], [(-big, -big, big, big), (10, 10, 30, 30)],
             [(40, 30, 40 + 10000, 30 + 9000), (-8194 + 50, -8194 + 36, 50, 36)]]
    assert [cr.box_level(b[0], 8, 2) for b in boxes] == [10000, 32768, 5000]
    assert cr.box_level(boxes[2][1], 8, 2) == 4097 and cr.grid(boxes[2][1], h, w, 8, 2) == (1, 1)
    _check(ctx, fr, boxes, 8, 2)
    frw = _frames(1, 3, 9000, 10)                                    # a clipped box of 2 x 1 cells of 4500 x 3 px
    wide = [[(0, -4000, 9000, 5000)]]
    assert cr.box_level(wide[0][0], 8, 2) == 4500 and cr.grid(wide[0][0], 3, 9000, 8, 2) == (2, 1)
    _check(ctx, frw, wide, 8, 2)


def test_300_boxes_counts_and_determinism(ctx):
    """300 boxes in one frame (more than the 32 workgroups of a frame, more than the mosaic's
    256-box fast path and than the 128 beating boxes the LDS lists), counts of 0, 1 and many
    across frames, and two runs with identical bytes."""
    rng = np.random.default_rng(4)
    fr = _frames(4, 96, 128, 4)
    x, y = rng.integers(-4, 124, 300), rng.integers(-4, 92, 300)
    bw, bh = rng.integers(1, 14, 300), rng.integers(1, 12, 300)
    many = [(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in zip(x, y, bw, bh)]
    boxes = [many, [], [(30, 22, 61, 47)], many[:9] + [(0, 0, 128, 96)]]
    a_m, a_s = _check(ctx, fr, boxes, 1, 2)
    b_m, b_s = _check(ctx, fr, boxes, 1, 2)
    np.testing.assert_array_equal(a_m, b_m)
    np.testing.assert_array_equal(a_s, b_s)
    np.testing.assert_array_equal(a_s[1], fr[1])                     # no boxes: the frame as it came
    # every small box under one that beats it: the beating list of the last boxes overflows
    under = [many + [(0, 0, 128, 96)] * 1, [(0, 0, 128, 96)] * 140 + [(10, 10, 20, 20)]]
    _check(ctx, fr[:2], under, 1, 2)


def test_device_lists_past_cap_and_host_lists_past_cap(ctx):
    """DeviceBoxes whose count exceeds cap: the first cap boxes are used, as vd_mosaic does; a
    host list with count > cap is refused."""
    import torch
    import vdmi
    from vdmi import _lib
    fr = _frames(2, 72, 100, 5)
    boxes = [[(5, 5, 40, 30), (30, 20, 66, 48), (60, 40, 95, 70)], [(10, 10, 50, 50)]]
    used = [b[:2] for b in boxes]
    xy, cnt = _arrays(used, cap=2)[0], np.asarray([3, 1], np.int32)
    db = vdmi.DeviceBoxes(2, 2, "cuda")
    db.xyxy.copy_(torch.from_numpy(xy))
    db.count.copy_(torch.from_numpy(cnt))
    ctx.set_cells(6)
    d = torch.from_numpy(fr).cuda()
    got_m = ctx.mosaic(d, db, level=1)
    got_s = ctx.smooth(d, db, level=1)
    ctx.sync()
    np.testing.assert_array_equal(got_m.cpu().numpy(), _ref(cr.mosaic_frame_cells, fr, used, 1, 6))
    np.testing.assert_array_equal(got_s.cpu().numpy(), _ref(cr.smooth_frame, fr, used, 1, 6))
    hb = _lib.HostBoxes(1, 2)
    hb.count[0] = 3
    with pytest.raises(_lib.VdCapacityError):
        ctx.smooth(fr[:1], hb)
    with pytest.raises(_lib.VdCapacityError):
        ctx.mosaic(fr[:1], hb)


@pytest.mark.parametrize("shape,g", [("ellipse", 42), ("rect", 30)])
def test_mask_shapes_the_lists_before_the_levels(ctx, shape, g):
    """Both modes under a mask: the reference composite over the grown boxes, whose sizes give
    the levels."""
    fr = _frames(2, 72, 100, 6)
    boxes = [[(30, 22, 61, 47), (50, 40, 99, 71)], [(-5, -5, 20, 20), (40, 10, 88, 30)]]
    grown = mr.grow((30, 22, 61, 47), g)
    assert cr.box_level(grown, 1, 6) > cr.box_level((30, 22, 61, 47), 1, 6)
    ctx.set_mask(shape, g)
    ctx.set_cells(6)
    xy, cnt = _arrays(boxes)
    got_m = ctx.mosaic(fr, xy, cnt, level=1)
    got_s = ctx.smooth(fr, xy, cnt, level=1)
    for i in range(2):
        np.testing.assert_array_equal(got_m[i], mr.shaped_frame(
            fr[i], boxes[i], shape, g, lambda im, bl: cr.mosaic_frame_cells(im, bl, 1, 6)), err_msg="mosaic")
        np.testing.assert_array_equal(got_s[i], mr.shaped_frame(
            fr[i], boxes[i], shape, g, lambda im, bl: cr.smooth_frame(im, bl, 1, 6)), err_msg="smooth")


def test_module_functions_and_the_grouped_pipeline_path(gpu):
    """vdmi.mosaic_frames(cells=...) / vdmi.smooth_frames on the shared contexts, and the
    per-group launches batch_process_images falls back to with foreign detectors."""
    import vdmi
    from vdmi.pipeline import _mosaic_grouped
    fr = _frames(2, 72, 100, 11)
    boxes = [[BOX_50x37, (60, 5, 95, 40)], [(-5, -5, 70, 60)]]
    np.testing.assert_array_equal(vdmi.mosaic_frames(fr, boxes, 1, cells=6), _ref(cr.mosaic_frame_cells, fr, boxes, 1, 6))
    np.testing.assert_array_equal(vdmi.smooth_frames(fr, boxes, 1, 6), _ref(cr.smooth_frame, fr, boxes, 1, 6))
    np.testing.assert_array_equal(vdmi.mosaic_frames(fr, boxes, 8), _ref(cr.mosaic_frame_cells, fr, boxes, 8, 0))
    got = _mosaic_grouped(list(fr), boxes, 1, ("gaussian", 31, 0.0), ("rect", 30), 6)
    for i in range(2):
        np.testing.assert_array_equal(got[i], mr.shaped_frame(
            fr[i], boxes[i], "rect", 30, lambda im, bl: cr.smooth_frame(im, bl, 1, 6)))
    got = _mosaic_grouped(list(fr), boxes, 1, ("pixelate", 31, 0.0), ("rect", 0), 6)
    np.testing.assert_array_equal(np.stack(got), _ref(cr.mosaic_frame_cells, fr, boxes, 1, 6))


def _launches(c, fn):
    c.timing(True)
    c.timing_reset()
    out = fn()
    c.sync()
    n = tuple(c.timing_read(f)[1] for f in range(7))
    c.timing(False)
    return out, n


def test_cells_0_is_the_old_path(ctx):
    """set_cells(0) after a setting: the bytes and the launch counts per timing family of a
    context that never had one; smooth() is two family-1 launches."""
    import vdmi
    fr = _frames(2, 72, 100, 7)
    boxes = [[(30, 22, 61, 47), (50, 40, 99, 71)], [(-5, -5, 90, 60)]]
    xy, cnt = _arrays(boxes)
    ctx.set_cells(2)
    on, n_on = _launches(ctx, lambda: ctx.mosaic(fr, xy, cnt))
    _, n_smooth = _launches(ctx, lambda: ctx.smooth(fr, xy, cnt))
    ctx.set_cells(0)
    got, n_back = _launches(ctx, lambda: ctx.mosaic(fr, xy, cnt))
    got_b, nb_back = _launches(ctx, lambda: ctx.blur(fr, xy, cnt, ksize=9))
    fresh = vdmi.Context(max_batch=8)
    try:
        exp, n_fresh = _launches(fresh, lambda: fresh.mosaic(fr, xy, cnt))
        exp_b, nb_fresh = _launches(fresh, lambda: fresh.blur(fr, xy, cnt, ksize=9))
    finally:
        fresh.close()
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(got_b, exp_b)
    for i in range(2):
        np.testing.assert_array_equal(got[i], omosaic.mosaic_frame(fr[i], boxes[i], 8))
    assert n_back == n_fresh and nb_back == nb_fresh
    assert n_on == n_fresh                                           # the per-box level adds no launch
    assert not np.array_equal(on, got)
    assert n_smooth[1] == 2 and n_smooth[3] == n_fresh[3] and n_smooth[6] == 0   # the copy and the box pass
    with pytest.raises(ValueError, match="cells"):
        ctx.smooth(fr, xy, cnt)                                      # the context's setting is 0


def test_refusals_keep_the_setting(ctx):
    import torch
    from vdmi import _lib
    lib, h = ctx._lib, ctx._h
    ctx.set_cells(6)
    for bad in (1, 65, -3):
        assert lib.vd_cells(h, bad) == _lib.VD_ERR_ARG
    fr = _frames(1, 72, 100, 8)
    boxes = [[BOX_50x37]]
    xy, cnt = _arrays(boxes)
    np.testing.assert_array_equal(ctx.mosaic(fr, xy, cnt, level=1), _ref(cr.mosaic_frame_cells, fr, boxes, 1, 6))
    s = _lib.vd_boxes(1, _lib.VD_HOST, cnt.ctypes.data, xy.ctypes.data, None, None, None)
    out = np.empty_like(fr)
    call = lambda i, o, hh, ww, where, lvl, cells: lib.vd_smooth(h, i, o, 1, hh, ww, ww * 3, where, ctypes.byref(s),
                                                                 lvl, cells)
    p, q = fr.ctypes.data, out.ctypes.data
    assert call(p, q, 72, 100, _lib.VD_HOST, 8, 6) == _lib.VD_OK
    assert call(p, q, 72, 100, _lib.VD_HOST, 8, 0) == _lib.VD_ERR_ARG          # cells = 0
    assert call(p, q, 72, 100, _lib.VD_HOST, 8, 65) == _lib.VD_ERR_ARG
    assert call(p, p, 72, 100, _lib.VD_HOST, 8, 6) == _lib.VD_ERR_ARG          # out == in
    assert call(p, q, 72, 100, _lib.VD_HOST, 0, 6) == _lib.VD_ERR_ARG          # level = 0
    assert call(p, q, 72, 100, _lib.VD_HOST, 32769, 6) == _lib.VD_ERR_ARG
    wide = np.zeros((1, 1, 32769, 3), np.uint8)
    wout = np.empty_like(wide)
    assert call(wide.ctypes.data, wout.ctypes.data, 1, 32769, _lib.VD_HOST, 8, 6) == _lib.VD_ERR_ARG
    d = torch.zeros((2 * 72 * 300,), dtype=torch.uint8, device="cuda")
    assert call(d.data_ptr(), d.data_ptr() + 300, 72, 100, _lib.VD_DEVICE, 8, 6) == _lib.VD_ERR_ARG   # overlapping
    assert call(d.data_ptr(), d.data_ptr() + 72 * 300, 72, 100, _lib.VD_DEVICE, 8, 6) == _lib.VD_OK
    ctx.sync()
    assert ctx.cells == 6
    np.testing.assert_array_equal(ctx.smooth(fr, xy, cnt, level=1), _ref(cr.smooth_frame, fr, boxes, 1, 6))


# ---- end to end through vd_process -------------------------------------------------------

PROCESS_HW = (120, 160)
PROCESS_LEVEL, PROCESS_CELLS = 1, 16       # boxes longer than 16 px get a level of their own
_NETS = {}


@pytest.fixture(scope="module")
def net_ctx(gpu):
    """fp32 contexts with seeded RetinaFace + YOLO weights by (blur mode, hold)."""
    import vdmi
    from vdmi import weights

    def make(blur, hold):
        key = (blur, hold)
        if key not in _NETS:
            c = vdmi.Context(precision="fp32", max_batch=4, hold=hold, blur=blur, mosaic_level=PROCESS_LEVEL)
            c.load_weights(0, weights.retinaface_state_dict(0))
            c.load_weights(1, weights.yolov8n_state_dict(0))
            _NETS[key] = c
        c = _NETS[key]
        c.hold_reset()
        c.set_mask("rect", 0)
        c.set_cells(0)
        return c

    yield make
    for c in _NETS.values():
        c.close()
    _NETS.clear()


def _process_frames():
    """Three 120 x 160 frames (60 x 80 noise, pixels doubled) on which the seeded weights keep a
    face in the first and plates in all."""
    from vdmi import synth
    h, w = PROCESS_HW
    return [np.repeat(np.repeat(synth.frame(h // 2, w // 2, i, seed=0), 2, 0), 2, 1) for i in range(3)]


def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


_REF = {"pixelate": cr.mosaic_frame_cells, "gaussian": cr.smooth_frame}


@pytest.mark.parametrize("blur", ["pixelate", "gaussian"])
def test_process_applies_the_levels_to_the_complete_keep_lists(net_ctx, blur):
    """vd_process with cells = 16: the output is the reference over read_boxes' lists, faces
    then plates; the returned lists are those of the context with cells off."""
    from vdmi import _lib
    fr = np.stack(_process_frames()[:2])
    c = net_ctx(blur, 0)
    out0, faces0, plates0 = c.process(fr, flags=_flags())
    c.set_cells(PROCESS_CELLS)
    out, faces, plates = c.process(fr, flags=_flags())
    ff = c.read_boxes(_lib.VD_NET_RETINAFACE, 2)
    pp = c.read_boxes(_lib.VD_NET_YOLOV8N, 2)
    total = 0
    for b in range(2):
        bl = _lists(ff, b) + _lists(pp, b)
        total += len(bl)
        np.testing.assert_array_equal(out[b], _REF[blur](fr[b], bl, PROCESS_LEVEL, PROCESS_CELLS))
        assert _lists(faces, b) == _lists(faces0, b) == _lists(ff, b)
        assert _lists(plates, b) == _lists(plates0, b) == _lists(pp, b)
    assert int(ff.count.sum()) > 0 and int(pp.count.sum()) > 0 and total == int(ff.count.sum() + pp.count.sum())
    assert not np.array_equal(out, out0)
    # without MOSAIC_PLATES the blur runs before the plate branch joins, on the faces alone
    out2, faces2, _ = c.process(fr, flags=_flags() & ~_lib.VD_PROC_MOSAIC_PLATES)
    for b in range(2):
        np.testing.assert_array_equal(out2[b], _REF[blur](fr[b], _lists(faces2, b), PROCESS_LEVEL, PROCESS_CELLS))


@pytest.mark.parametrize("blur", ["pixelate", "gaussian"])
def test_process_under_hold_uses_the_merged_lists(net_ctx, blur):
    """hold = 2 over [A, A, B, B, C, A] in calls of 4 + 2: every output is the reference over
    D_t ++ read_held, in that order."""
    a, b, cc = _process_frames()
    frames = [a, a, b, b, cc, a]
    c = net_ctx(blur, 2)
    c.set_cells(PROCESS_CELLS)
    lo, held_total = 0, 0
    for n in (4, 2):
        out, faces, plates = c.process(np.stack(frames[lo:lo + n]), flags=_flags())
        held = c.read_held(n)
        for i in range(n):
            k = int(held.count[i])
            assert k <= held.cap
            H = [tuple(int(v) for v in r) for r in held.xyxy[i, :k]]
            held_total += k
            bl = _lists(faces, i) + _lists(plates, i) + H
            np.testing.assert_array_equal(out[i], _REF[blur](frames[lo + i], bl, PROCESS_LEVEL, PROCESS_CELLS),
                                          err_msg=f"frame {lo + i}")
        lo += n
    assert held_total > 0


@pytest.mark.parametrize("blur", ["pixelate", "gaussian"])
def test_batch_process_images_one_call_and_per_group_paths(gpu, tmp_path, blur):
    """batch_process_images(cells=4): with a face detector built with the same setting the
    one-call vd_process path runs, with a default one the per-group launches; both write the
    reference over the detector's boxes."""
    import os
    import vdmi
    from vdmi import synth, weights
    from vdmi.pipeline import batch_process_images
    frames = {f"f{i:03d}.png": synth.frame(360, 640, i, seed=3) for i in range(3)}
    for name in frames:
        (tmp_path / name).write_bytes(b"")
    plate = vdmi.YOLO(weights="random", max_batch=4)
    sd = weights.retinaface_state_dict(0)
    boxes = None
    for built_with in (4, 0):
        face = vdmi.Retinaface(input_shape=[640, 640, 3], nms_iou=0.4, max_batch=4, weights=sd, blur=blur,
                               cells=built_with)
        assert face.ctx.cells == built_with
        saved = {}
        n, nf, _ = batch_process_images(str(tmp_path), str(tmp_path / "out"), face, plate, batch_size=2, blur=blur,
                                        cells=4, loader=lambda p: frames[os.path.basename(p)],
                                        saver=lambda img, p: saved.__setitem__(os.path.basename(p), img))
        assert n == 3 and len(saved) == 3
        if boxes is None:
            boxes = {name: [tuple(int(v) for v in b) for b in face.detect_images([img])[0][1]]
                     for name, img in frames.items()}
            assert nf == sum(len(b) for b in boxes.values()) > 0
            assert any(cr.box_level(b, 8, 4) > 8 for bl in boxes.values() for b in bl)
        for name, img in frames.items():
            np.testing.assert_array_equal(saved[f"processed_{name}"], _REF[blur](img, boxes[name], 8, 4),
                                          err_msg=f"{name}, detector built with cells={built_with}")
