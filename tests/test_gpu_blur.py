"""The Gaussian-blur mode on the GPU (vd_blur, vd_process with blur="gaussian") against the
numpy definition in gaussian_ref.py, bit for bit, whole frames (so bytes outside the boxes
are checked too), with the library's own tap weights."""
import ctypes

import numpy as np
import pytest

import gaussian_ref as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    import vdmi
    c = vdmi.Context(max_batch=8)
    yield c
    c.close()


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _ref(frames, boxes, k, sigma):
    from vdmi import _lib
    q = _lib.blur_weights(k, sigma)
    return np.stack([gr.blur_frame(frames[i], boxes[i], k, sigma, q=q) for i in range(len(frames))])


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


def _run(ctx, frames, boxes, k, sigma=0.0):
    xy, cnt = _arrays(boxes)
    keep = frames.copy()
    out = ctx.blur(frames, xy, cnt, ksize=k, sigma=sigma)
    np.testing.assert_array_equal(frames, keep)            # the input is untouched
    return out


def test_interior_box(ctx):
    fr = _frames(1, 40, 64, 0)
    boxes = [[(10, 8, 40, 30)]]
    np.testing.assert_array_equal(_run(ctx, fr, boxes, 5), _ref(fr, boxes, 5, 0.0))


def test_degenerate_and_edge_boxes(ctx):
    """k = 31 on boxes narrower than the radius (several reflections), boxes clipped by each
    frame edge, a box outside the frame and an empty one."""
    fr = _frames(1, 72, 100, 1)
    boxes = [[(3, 3, 4, 4), (10, 3, 17, 4), (20, 3, 25, 5), (30, 3, 33, 8),            # 1x1, 1x7, 2x5, 5x3
              (-9, 20, 12, 45), (90, 18, 130, 40), (40, -7, 70, 9), (45, 60, 80, 99),    # left, right, top, bottom
              (200, 200, 240, 230), (-50, -50, -10, -10), (60, 30, 60, 50), (70, 50, 65, 58)]]
    np.testing.assert_array_equal(_run(ctx, fr, boxes, 31), _ref(fr, boxes, 31, 0.0))


def test_overlapping_boxes_in_list_order(ctx):
    """A chain of three, a box met only by a LATER one, two identical boxes -- host lists
    and DeviceBoxes; the reversed chain gives another image (order is observed)."""
    import torch
    import vdmi
    fr = _frames(2, 64, 96, 2)
    chain = [(4, 4, 40, 30), (28, 14, 66, 44), (52, 24, 92, 60)]
    boxes = [chain + [(2, 40, 24, 62), (10, 46, 40, 58)],           # (2,40..) is met only by the later box
             [(20, 10, 70, 50), (20, 10, 70, 50)] + chain[::-1]]
    exp = _ref(fr, boxes, 9, 0.0)
    np.testing.assert_array_equal(_run(ctx, fr, boxes, 9), exp)
    assert not np.array_equal(exp[0], gr.blur_frame(fr[0], boxes[0][::-1], 9, 0.0))
    xy, cnt = _arrays(boxes, cap=7)
    db = vdmi.DeviceBoxes(2, 7, "cuda")
    db.xyxy.copy_(torch.from_numpy(xy))
    db.count.copy_(torch.from_numpy(cnt))
    out = ctx.blur(torch.from_numpy(fr).cuda(), db, ksize=9)
    ctx.sync()                                             # every pointer on the device: the call is asynchronous
    np.testing.assert_array_equal(out.cpu().numpy(), exp)


@pytest.mark.parametrize("k", [9, 127])
def test_wide_dependent_boxes(ctx, k):
    """Dependent boxes of several 64-column strips (in place through the two-strip scratch),
    up to the radius the strip width allows; widths at, below and above strip multiples."""
    fr = _frames(1, 40, 230, 11 + k)
    boxes = [[(0, 0, 200, 40), (0, 0, 200, 40), (3, 5, 131, 33), (100, 2, 229, 38), (10, 10, 75, 30), (-5, 20, 300, 21)]]
    np.testing.assert_array_equal(_run(ctx, fr, boxes, k), _ref(fr, boxes, k, 0.0))


def test_many_boxes(ctx):
    """300 small boxes in one frame, some overlapping: past the 256 boxes one pass of the
    plan kernel classifies."""
    rng = np.random.default_rng(3)
    fr = _frames(1, 96, 128, 3)
    x = rng.integers(-4, 124, 300)
    y = rng.integers(-4, 92, 300)
    bw = rng.integers(1, 14, 300)
    bh = rng.integers(1, 12, 300)
    boxes = [[(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in zip(x, y, bw, bh)]]
    np.testing.assert_array_equal(_run(ctx, fr, boxes, 7), _ref(fr, boxes, 7, 0.0))


def test_geometry_batch_and_determinism(ctx):
    """w = 61 (pitch 183: no 16-byte alignment), counts [0, 1, 7, 0, 3]; a frame alone equals
    the frame in its batch; two runs are identical."""
    rng = np.random.default_rng(4)
    fr = _frames(5, 37, 61, 4)
    counts = [0, 1, 7, 0, 3]
    boxes = []
    for c in counts:
        bl = []
        for _ in range(c):
            x1, y1 = int(rng.integers(-5, 50)), int(rng.integers(-5, 30))
            bl.append((x1, y1, x1 + int(rng.integers(2, 30)), y1 + int(rng.integers(2, 24))))
        boxes.append(bl)
    exp = _ref(fr, boxes, 11, 0.0)
    a = _run(ctx, fr, boxes, 11)
    np.testing.assert_array_equal(a, exp)
    np.testing.assert_array_equal(_run(ctx, fr, boxes, 11), a)
    for i in range(5):
        np.testing.assert_array_equal(_run(ctx, fr[i:i + 1], boxes[i:i + 1], 11)[0], a[i])


def test_padded_pitch_device_tensor(ctx):
    """Rows of 50 pixels in a pitch of 64 pixels: the padding bytes of `out` stay as they were."""
    import torch
    fr = _frames(2, 33, 50, 5)
    boxes = [[(5, 4, 30, 20), (20, 10, 49, 33)], [(-3, 25, 12, 40)]]
    big_in = torch.full((2, 33, 64, 3), 7, dtype=torch.uint8, device="cuda")
    big_out = torch.full((2, 33, 64, 3), 9, dtype=torch.uint8, device="cuda")
    big_in[:, :, :50] = torch.from_numpy(fr).cuda()
    xy, cnt = _arrays(boxes)
    ctx.blur(big_in[:, :, :50], xy, cnt, ksize=9, out=big_out[:, :, :50])
    got = big_out.cpu().numpy()
    np.testing.assert_array_equal(got[:, :, :50], _ref(fr, boxes, 9, 0.0))
    assert (got[:, :, 50:] == 9).all()


def test_largest_kernel(ctx):
    """k = 127, sigma 40 on a 150 x 200 box: the bit-exact definition, itself within 1 of the
    rounded float64 Gaussian."""
    fr = _frames(1, 240, 320, 6)
    boxes = [[(60, 40, 260, 190)]]
    out = _run(ctx, fr, boxes, 127, 40.0)
    np.testing.assert_array_equal(out, _ref(fr, boxes, 127, 40.0))
    exact = gr.blur_frame(fr[0], boxes[0], 127, 40.0, exact=True)
    assert int(np.abs(out[0].astype(np.int16) - exact.astype(np.int16)).max()) <= 1


def test_refusals(ctx):
    import torch
    from vdmi import _lib
    fr = _frames(1, 24, 32, 7)
    xy, cnt = _arrays([[(2, 2, 20, 20)]])
    with pytest.raises(_lib.VdError) as e:
        ctx.blur(fr, xy, cnt, ksize=8)
    assert e.value.code == _lib.VD_ERR_ARG
    with pytest.raises(_lib.VdError) as e:
        ctx.blur(fr, xy, cnt, ksize=9, sigma=float("nan"))
    assert e.value.code == _lib.VD_ERR_ARG
    d = torch.from_numpy(fr).cuda()
    with pytest.raises(_lib.VdError, match="out-of-place") as e:
        ctx.blur(d, xy, cnt, ksize=9, out=d)
    assert e.value.code == _lib.VD_ERR_ARG
    with pytest.raises(_lib.VdError, match="out-of-place"):
        ctx.blur(fr, xy, cnt, ksize=9, out=fr)
    hb = _lib.HostBoxes(1, 2)
    hb.count[0] = 3
    with pytest.raises(_lib.VdCapacityError) as e:
        ctx.blur(fr, hb, ksize=9)
    assert e.value.code == _lib.VD_ERR_CAPACITY
    # vd_mosaic still knows one mode only
    s = hb.struct()
    out = np.empty_like(fr)
    hb.count[0] = 1
    assert ctx._lib.vd_mosaic(ctx._h, _lib.ptr(fr), _lib.ptr(out), 1, 24, 32, 96, _lib.VD_HOST, ctypes.byref(s), 8,
                              1) == _lib.VD_ERR_ARG


def _lists(boxes, b):
    return [tuple(int(v) for v in r) for r in boxes.frame(b)[0]]


def _meet(a, c):
    return a[0] < c[2] and c[0] < a[2] and a[1] < c[3] and c[1] < a[3]


def test_process_gaussian_uses_complete_keep_lists(gpu, face_ctx_factory):
    """vd_process in a blur="gaussian" context: out = the reference over the complete keep
    lists, the box lists those of a pixelate context; the frames keep overlapping boxes
    (dense weights; confirmed with the CPU oracle forward), so the dependent path runs."""
    from vdmi import _lib, synth
    fr = synth.frames(2, 360, 640, seed=PROCESS_SEED)
    g = face_ctx_factory("fp32", 2, "dense", blur="gaussian", blur_ksize=9)
    p = face_ctx_factory("fp32", 2, "dense")
    out, faces, _ = g.process(fr)
    full = g.read_boxes(_lib.VD_NET_RETINAFACE, 2)
    out_p, faces_p, _ = p.process(fr)
    kept, meeting = 0, 0
    for b in range(2):
        bl = _lists(full, b)
        assert len(bl) == int(full.count[b])
        kept += len(bl)
        cl = [c for c in (gr.clip_box(x, 360, 640) for x in bl) if c]
        meeting += sum(_meet(cl[i], cl[j]) for i in range(len(cl)) for j in range(i))
        np.testing.assert_array_equal(out[b], gr.blur_frame(fr[b], bl, 9, 0.0, q=_lib.blur_weights(9, 0.0)))
        np.testing.assert_array_equal(faces.frame(b)[0], faces_p.frame(b)[0])
    np.testing.assert_array_equal(faces.count, faces_p.count)
    assert kept > 0 and meeting > 0
    assert not np.array_equal(out, out_p)


PROCESS_SEED = 0


def test_process_gaussian_faces_then_plates(gpu):
    import vdmi
    from vdmi import _lib, synth, weights
    fr = synth.frames(2, 1080, 1920, seed=8)
    c = vdmi.Context(precision="bf16", max_batch=2, blur="gaussian", blur_ksize=9)
    try:
        c.load_weights(0, weights.retinaface_state_dict(0))
        c.load_weights(1, weights.yolov8n_state_dict(0))
        flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES
        out, faces, plates = c.process(fr, flags=flags)
        q = _lib.blur_weights(9, 0.0)
        for b in range(2):
            fb, pb = _lists(faces, b), _lists(plates, b)
            assert len(fb) == int(faces.count[b]) and len(pb) == int(plates.count[b])
            np.testing.assert_array_equal(out[b], gr.blur_frame(fr[b], fb + pb, 9, 0.0, q=q))
        assert int(plates.count.sum()) > 0
        # without MOSAIC_PLATES the plate boxes are discarded, as in pixelate mode
        out2, faces2, _ = c.process(fr, flags=flags & ~_lib.VD_PROC_MOSAIC_PLATES)
        for b in range(2):
            np.testing.assert_array_equal(out2[b], gr.blur_frame(fr[b], _lists(faces2, b), 9, 0.0, q=q))
    finally:
        c.close()


def test_drop_ins_and_pixelate_unchanged(gpu, face_ctx_factory):
    import vdmi
    from oracle import mosaic as omosaic
    from vdmi import _lib, synth
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)
    got = vdmi.gaussian_blur_region_single(img, 10, -4, 48, 30)
    np.testing.assert_array_equal(got, gr.blur_frame(img, [(10, -4, 48, 30)], 31, 0.0, q=_lib.blur_weights(31, 0.0)))
    fr = _frames(2, 50, 70, 10)
    boxes = [[(5, 5, 40, 30), (30, 20, 66, 48)], []]
    np.testing.assert_array_equal(vdmi.blur_frames(fr, boxes, ksize=7, sigma=1.5), _ref(fr, boxes, 7, 1.5))
    # a default context still pixelates, to the bit
    ctx = face_ctx_factory("fp32", 2, "dense")
    sf = synth.frames(2, 360, 640, seed=PROCESS_SEED)
    out, faces, _ = ctx.process(sf)
    full = ctx.read_boxes(_lib.VD_NET_RETINAFACE, 2)
    for b in range(2):
        np.testing.assert_array_equal(out[b], omosaic.mosaic_frame(sf[b], _lists(full, b), 8))
