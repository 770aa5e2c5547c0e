"""Mask shaping on the GPU (vd_mask, vd_mask_boxes; mask.hip) against the numpy definition in
mask_ref.py, bit for bit and whole frames (so bytes outside the boxes are checked too). Every
case runs through ctx.mosaic and through ctx.blur; the restore pass works on bands of 16 rows
with a band list of 64 boxes, which the shapes below straddle."""
import numpy as np
import pytest

import gaussian_ref as gr
import hold_ref as hr
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
def _default_mask_afterwards(request):
    yield
    if "ctx" in request.fixturenames:
        request.getfixturevalue("ctx").set_mask("rect", 0)


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


_Q = {}


def _rect_fn(k):
    """The rectangular pass of the reference: the oracle mosaic (k None) or the Gaussian blur
    with the library's own tap weights."""
    if k is None:
        return lambda img, bl: omosaic.mosaic_frame(img, bl, 8)
    if k not in _Q:
        from vdmi import _lib
        _Q[k] = _lib.blur_weights(k, 0.0)
    return lambda img, bl: gr.blur_frame(img, bl, k, 0.0, q=_Q[k])


def _ref(fr, boxes, shape, g, k):
    return np.stack([mr.shaped_frame(fr[i], boxes[i], shape, g, _rect_fn(k)) for i in range(len(fr))])


def _check(ctx, fr, boxes, shape, g, k=9):
    """mosaic() and blur(ksize=k) of host frames and host lists under mask (shape, g) against
    the reference; the input is untouched. Returns the two outputs."""
    ctx.set_mask(shape, g)
    xy, cnt = _arrays(boxes)
    keep = fr.copy()
    got_m = ctx.mosaic(fr, xy, cnt)
    got_b = ctx.blur(fr, xy, cnt, ksize=k)
    np.testing.assert_array_equal(fr, keep)
    np.testing.assert_array_equal(got_m, _ref(fr, boxes, shape, g, None), err_msg="mosaic")
    np.testing.assert_array_equal(got_b, _ref(fr, boxes, shape, g, k), err_msg="blur")
    return got_m, got_b


@pytest.mark.parametrize("shape", ["ellipse", "rect"])
@pytest.mark.parametrize("g", [0, 30, 42])
def test_interior_box(ctx, shape, g):
    fr = _frames(1, 72, 100, 0)
    boxes = [[(30, 22, 61, 47)]]
    got_m, _ = _check(ctx, fr, boxes, shape, g)
    if shape == "ellipse":                                # the grown box's corner shows the input
        x1, y1, _, _ = mr.grow(boxes[0][0], g)
        np.testing.assert_array_equal(got_m[0, y1, x1], fr[0, y1, x1])


@pytest.mark.parametrize("g", [0, 30])
def test_sides_1_to_5(ctx, g):
    fr = _frames(1, 72, 100, 1)
    boxes = [[(5 + 12 * s, 6, 5 + 13 * s, 6 + s) for s in (1, 2, 3, 4, 5)] +             # s x s
             [(8, 30, 9, 35), (20, 30, 25, 31), (40, 30, 42, 34), (60, 40, 64, 43)]]     # 1x5, 5x1, 2x4, 4x3
    _check(ctx, fr, boxes, "ellipse", g)


@pytest.mark.parametrize("g", [0, 42])
def test_boxes_clipped_by_each_edge(ctx, g):
    """Centres of the ellipses off the frame, a box wholly outside, an empty and an inverted
    box; k = 31 reflects several times in the narrow clipped boxes."""
    h, w = mr.EDGE_HW
    fr = _frames(1, h, w, 2)
    _check(ctx, fr, [list(mr.EDGE_BOXES)], "ellipse", g, k=31)


def test_growth_leaves_the_frame(ctx):
    fr = _frames(2, 72, 100, 3)
    boxes = [[(2, 3, 95, 68)], [(0, 0, 100, 72), (90, 60, 99, 71)]]
    _check(ctx, fr, boxes, "ellipse", 30)
    _check(ctx, fr, boxes, "rect", 200)


def test_row_bands_and_wide_boxes(ctx):
    """Boxes over two and three 16-row bands, rows that end on band borders, a box wider than
    one wave's 64 columns and one wider than the workgroup's 256 threads."""
    fr = _frames(1, 96, 128, 4)
    boxes = [[(4, 10, 30, 28), (36, 10, 60, 41), (66, 16, 90, 32), (96, 31, 120, 33), (3, 50, 125, 70),
              (10, 80, 50, 96)]]
    _check(ctx, fr, boxes, "ellipse", 0)
    _check(ctx, fr, boxes, "ellipse", 30)
    wide = _frames(1, 40, 300, 5)
    _check(ctx, wide, [[(10, 3, 290, 37), (0, 20, 300, 22)]], "ellipse", 0)


def test_overlapping_boxes(ctx):
    """A chain of three, two identical boxes, a small box in a large one's corner whose own
    corner is restored by neither box, and a small box inside a large one's ellipse."""
    fr = _frames(2, 96, 128, 6)
    chain = [(4, 4, 40, 30), (28, 14, 66, 44), (52, 24, 92, 60)]
    large = (10, 50, 90, 94)
    boxes = [chain + [(100, 10, 124, 40), (100, 10, 124, 40)],
             [large, (8, 48, 16, 56), (40, 60, 52, 70)] + chain[::-1]]
    assert not mr.inside(large, 10, 50) and not mr.inside((8, 48, 16, 56), 8, 48)
    got_m, _ = _check(ctx, fr, boxes, "ellipse", 0)
    assert not mr.inside(large, 15, 55) and not mr.inside((8, 48, 16, 56), 15, 55)
    np.testing.assert_array_equal(got_m[1, 55, 15], fr[1, 55, 15])         # in both rectangles, in neither ellipse
    assert mr.inside((8, 48, 16, 56), 11, 51) and not mr.inside(large, 11, 51)
    R = omosaic.mosaic_frame(fr[1], boxes[1], 8)
    np.testing.assert_array_equal(got_m[1, 51, 11], R[51, 11])             # the large box's corner, the small one's ellipse
    _check(ctx, fr, boxes, "ellipse", 30)


def test_side_over_32768_hides_its_rectangle(ctx):
    fr = _frames(1, 72, 100, 7)
    boxes = [[(-20000, 5, 20000, 40), (30, 30, 60, 60)]]
    got_m, _ = _check(ctx, fr, boxes, "ellipse", 0)
    np.testing.assert_array_equal(got_m[0, 5:30], omosaic.mosaic_frame(fr[0], boxes[0], 8)[5:30])


def test_300_boxes_in_one_frame(ctx):
    """Past the mosaic's 256-box fast path and the restore pass's 64-box band list."""
    rng = np.random.default_rng(8)
    fr = _frames(1, 96, 128, 8)
    x, y = rng.integers(-4, 124, 300), rng.integers(-4, 92, 300)
    bw, bh = rng.integers(1, 14, 300), rng.integers(1, 12, 300)
    boxes = [[(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in zip(x, y, bw, bh)]]
    _check(ctx, fr, boxes, "ellipse", 30, k=7)
    _check(ctx, fr, boxes, "ellipse", 0, k=7)


def test_counts_0_1_many_and_determinism(ctx):
    rng = np.random.default_rng(9)
    fr = _frames(4, 75, 101, 9)                           # pitch 303: no 16-byte alignment
    boxes = []
    for c in (0, 1, 9, 3):
        bl = []
        for _ in range(c):
            x1, y1 = int(rng.integers(-8, 90)), int(rng.integers(-8, 66))
            bl.append((x1, y1, x1 + int(rng.integers(2, 40)), y1 + int(rng.integers(2, 30))))
        boxes.append(bl)
    a_m, a_b = _check(ctx, fr, boxes, "ellipse", 30)
    b_m, b_b = _check(ctx, fr, boxes, "ellipse", 30)      # two calls: identical bytes
    np.testing.assert_array_equal(a_m, b_m)
    np.testing.assert_array_equal(a_b, b_b)
    np.testing.assert_array_equal(a_m[0], fr[0])          # no boxes: the frame as it came


def test_device_boxes_with_count_over_cap(ctx):
    """DeviceBoxes whose count exceeds cap: the first cap boxes are used, as without a mask."""
    import torch
    import vdmi
    fr = _frames(2, 72, 100, 10)
    boxes = [[(5, 5, 40, 30), (30, 20, 66, 48), (60, 40, 95, 70)], [(10, 10, 50, 50)]]
    used = [b[:2] for b in boxes]                          # what the arrays hold of each list
    xy, cnt = _arrays(used, cap=2)[0], np.asarray([3, 1], np.int32)
    db = vdmi.DeviceBoxes(2, 2, "cuda")
    db.xyxy.copy_(torch.from_numpy(xy))
    db.count.copy_(torch.from_numpy(cnt))
    ctx.set_mask("ellipse", 30)
    d = torch.from_numpy(fr).cuda()
    got_m = ctx.mosaic(d, db)
    got_b = ctx.blur(d, db, ksize=9)
    ctx.sync()
    np.testing.assert_array_equal(got_m.cpu().numpy(), _ref(fr, used, "ellipse", 30, None))
    np.testing.assert_array_equal(got_b.cpu().numpy(), _ref(fr, used, "ellipse", 30, 9))
    np.testing.assert_array_equal(d.cpu().numpy(), fr)


def test_padded_pitch_device_view(ctx):
    """Rows of 50 pixels in a pitch of 64: blur() works at the view's pitch and the padding of
    `out` stays as it was; mosaic() packs the view."""
    import torch
    fr = _frames(2, 33, 50, 11)
    boxes = [[(5, 4, 30, 20), (20, 10, 49, 33)], [(-3, 25, 12, 40)]]
    big_in = torch.full((2, 33, 64, 3), 7, dtype=torch.uint8, device="cuda")
    big_out = torch.full((2, 33, 64, 3), 9, dtype=torch.uint8, device="cuda")
    big_in[:, :, :50] = torch.from_numpy(fr).cuda()
    xy, cnt = _arrays(boxes)
    ctx.set_mask("ellipse", 30)
    ctx.blur(big_in[:, :, :50], xy, cnt, ksize=9, out=big_out[:, :, :50])
    got = big_out.cpu().numpy()
    np.testing.assert_array_equal(got[:, :, :50], _ref(fr, boxes, "ellipse", 30, 9))
    assert (got[:, :, 50:] == 9).all()
    got_m = ctx.mosaic(big_in[:, :, :50], xy, cnt)
    ctx.sync()
    np.testing.assert_array_equal(got_m.cpu().numpy(), _ref(fr, boxes, "ellipse", 30, None))
    assert (big_in.cpu().numpy()[:, :, 50:] == 7).all()


def test_mask_boxes_is_grow(ctx):
    """Host and device lists; counts as given (also past cap), nothing but xyxy written."""
    import torch
    import vdmi
    from vdmi import _lib
    big = 1 << 30
    lists = [[(10, 20, 17, 30), (0, 0, 8, 20), (5, 5, 6, 6), (60, 30, 60, 50), (70, 50, 65, 58)],
             [], [(big - 10, 0, big - 2, 10), (-2**31, -2**31, 2**31 - 1, 2**31 - 1), (-9, -9, 30, 3)]]
    for g in (0, 30, 200):
        ctx.set_mask("ellipse" if g else "rect", g)
        out = ctx.mask_boxes(lists)
        assert isinstance(out, _lib.HostBoxes) and out.cap == 5
        for i, bl in enumerate(lists):
            assert int(out.count[i]) == len(bl)
            assert [tuple(int(v) for v in r) for r in out.xyxy[i, :len(bl)]] == mr.grow_list(bl, g)
        assert not out.label.any() and not out.score.any() and not out.xyxy_f.any()
    ctx.set_mask("rect", 30)
    xy, cnt = _arrays(lists)
    db = vdmi.DeviceBoxes(3, 5, "cuda")
    db.xyxy.copy_(torch.from_numpy(xy))
    db.count.copy_(torch.from_numpy(np.asarray([7, 0, 3], np.int32)))     # frame 0: count past cap
    dev = ctx.mask_boxes(db)
    ctx.sync()
    assert isinstance(dev, vdmi.DeviceBoxes)
    assert dev.count.cpu().tolist() == [7, 0, 3]
    got = dev.xyxy.cpu().numpy()
    for i, bl in enumerate(lists):
        assert [tuple(int(v) for v in r) for r in got[i, :len(bl)]] == mr.grow_list(bl, 30)
    np.testing.assert_array_equal(db.xyxy.cpu().numpy(), xy)              # the input lists are untouched
    hb = _lib.HostBoxes(1, 2)
    hb.count[0] = 3
    with pytest.raises(_lib.VdCapacityError):
        ctx.mask_boxes(hb)


def test_refusals_keep_the_setting(ctx):
    from vdmi import _lib
    ctx.set_mask("ellipse", 30)
    assert ctx._lib.vd_mask(ctx._h, 2, 0) == _lib.VD_ERR_ARG
    assert ctx._lib.vd_mask(ctx._h, _lib.VD_MASK_RECT, 201) == _lib.VD_ERR_ARG
    assert ctx._lib.vd_mask(ctx._h, _lib.VD_MASK_RECT, -1) == _lib.VD_ERR_ARG
    fr = _frames(1, 72, 100, 12)
    _check(ctx, fr, [[(30, 22, 61, 47)]], "ellipse", 30)                   # set again by _check: still valid
    hb = _lib.HostBoxes(1, 2)
    hb.count[0] = 3
    with pytest.raises(_lib.VdCapacityError):
        ctx.mosaic(fr, hb)
    with pytest.raises(_lib.VdCapacityError):
        ctx.blur(fr, hb, ksize=9)


def _launches(c, fn):
    c.timing(True)
    c.timing_reset()
    out = fn()
    c.sync()
    n = (c.timing_read(1)[1], c.timing_read(3)[1])
    c.timing(False)
    return out, n


def test_back_to_the_default_is_the_old_path(ctx):
    """set_mask("rect", 0) after an ellipse: the bytes and the family-1 / family-3 launch counts
    of a context that never had a mask; a mask adds one grow and one restore launch."""
    import vdmi
    fr = _frames(2, 72, 100, 13)
    boxes = [[(30, 22, 61, 47), (50, 40, 99, 71)], [(-5, -5, 20, 20)]]
    xy, cnt = _arrays(boxes)
    ctx.set_mask("ellipse", 30)
    _, n_ell = _launches(ctx, lambda: ctx.mosaic(fr, xy, cnt))
    ctx.set_mask("rect", 30)
    _, n_rect = _launches(ctx, lambda: ctx.mosaic(fr, xy, cnt))
    ctx.set_mask("rect", 0)
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
    assert n_rect == (n_fresh[0], n_fresh[1] + 1)
    assert n_ell == (n_fresh[0] + 1, n_fresh[1] + 1)


# ---- end to end through vd_process -------------------------------------------------------

PROCESS_HW = (120, 160)
_NETS = {}


@pytest.fixture(scope="module")
def net_ctx(gpu):
    """fp32 contexts with seeded RetinaFace + YOLO weights by hold setting."""
    import vdmi
    from vdmi import weights

    def make(hold):
        if hold not in _NETS:
            c = vdmi.Context(precision="fp32", max_batch=4, hold=hold)
            c.load_weights(0, weights.retinaface_state_dict(0))
            c.load_weights(1, weights.yolov8n_state_dict(0))
            _NETS[hold] = c
        c = _NETS[hold]
        c.hold_reset()
        c.set_mask("rect", 0)
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


def test_process_shapes_the_complete_keep_lists(net_ctx):
    """vd_process under ("ellipse", 30): the output is the reference over read_boxes' lists,
    faces then plates; the returned lists are those of the context without a mask."""
    from vdmi import _lib
    h, w = PROCESS_HW
    fr = np.stack(_process_frames()[:2])
    c = net_ctx(0)
    out0, faces0, plates0 = c.process(fr, flags=_flags())
    c.set_mask("ellipse", 30)
    out, faces, plates = c.process(fr, flags=_flags())
    ff = c.read_boxes(_lib.VD_NET_RETINAFACE, 2)
    pp = c.read_boxes(_lib.VD_NET_YOLOV8N, 2)
    total = 0
    for b in range(2):
        bl = _lists(ff, b) + _lists(pp, b)
        total += len(bl)
        np.testing.assert_array_equal(out[b], mr.shaped_frame(fr[b], bl, "ellipse", 30, _rect_fn(None)))
        np.testing.assert_array_equal(out0[b], omosaic.mosaic_frame(fr[b], bl, 8))
        assert _lists(faces, b) == _lists(faces0, b) == _lists(ff, b)
        assert _lists(plates, b) == _lists(plates0, b) == _lists(pp, b)
    assert int(ff.count.sum()) > 0 and int(pp.count.sum()) > 0 and total == int(ff.count.sum() + pp.count.sum())
    assert not np.array_equal(out, out0)
    # without MOSAIC_PLATES the mosaic runs before the plate branch joins, on the faces alone
    out2, faces2, _ = c.process(fr, flags=_flags() & ~_lib.VD_PROC_MOSAIC_PLATES)
    for b in range(2):
        np.testing.assert_array_equal(out2[b], mr.shaped_frame(fr[b], _lists(faces2, b), "ellipse", 30,
                                                               _rect_fn(None)))


def _held(held, b):
    k = int(held.count[b])
    assert k <= held.cap
    return [tuple(int(v) for v in r) for r in held.xyxy[b, :k]], [int(v) for v in held.label[b, :k]]


def _sequence(c, frames, calls):
    outs, D, H, ages = [], [], [], []
    lo = 0
    for n in calls:
        out, faces, plates = c.process(np.stack(frames[lo:lo + n]), flags=_flags())
        held = c.read_held(n)
        for b in range(n):
            outs.append(out[b])
            D.append(_lists(faces, b) + _lists(plates, b))
            rows, lab = _held(held, b)
            H.append(rows)
            ages.append(lab)
        lo += n
    return outs, D, H, ages


def test_hold_lists_are_shaped_after_the_merge(net_ctx):
    """hold=2 under ("ellipse", 30) over [A, A, B, B, C, A] in calls of 4 + 2: every output is
    the reference over grow(B_t); read_held gives the boxes as stored (ungrown), and H_t and
    the ages are those of the same holding context without a mask."""
    K, P = 2, 30
    h, w = PROCESS_HW
    a, b, cc = _process_frames()
    frames = [a, a, b, b, cc, a]
    c = net_ctx(K)
    _, D0, H0, ages0 = _sequence(c, frames, (4, 2))
    c.hold_reset()
    c.set_mask("ellipse", 30)
    outs, D, H, ages = _sequence(c, frames, (4, 2))
    assert D == D0 and H == H0 and ages == ages0
    B, Hr, ar, _ = hr.hold_lists(D, h, w, K, P)
    assert H == Hr and ages == ar                          # ungrown: the reference over the detections
    for t, fr in enumerate(frames):
        np.testing.assert_array_equal(outs[t], mr.shaped_frame(fr, B[t], "ellipse", 30, _rect_fn(None)),
                                      err_msg=f"frame {t}")
    assert sum(len(d) for d in D) > 0 and sum(len(x) for x in H) > 0
