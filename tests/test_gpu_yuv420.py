"""8-bit 4:2:0 frames in any layout on the GPU (include/vdmi.h at vd_yuv420; csrc/pre.hip, nv12.hip,
smooth.hip, mask.hip). The oracle is the NV12 path on N(S), the NV12 surface with the same samples
(tests/yuv420_ref.py), itself pinned against tests/nv12_ref.py by the NV12 tests; pixelation of caller
lists is checked against nv12_ref.mosaic directly. Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import nv12_ref as nr
import yuv420_ref as yr

pytestmark = pytest.mark.gpu

# csrc/nv12.hip
NV12_ROWS, NV12_LDS_BOXES, NV12_BAND_BOXES, NV12_CELLS = 16, 256, 32, 4096
GAUSS = dict(blur="gaussian", cells=8, mask="ellipse", mask_grow=42)

_NETS = {}


@pytest.fixture(scope="module")
def nets(gpu):
    """Contexts with seeded RetinaFace + YOLO weights by precision and keyword arguments."""
    import vdmi
    from vdmi import weights

    def make(precision="fp32", **kw):
        key = (precision,) + tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in _NETS:
            c = vdmi.Context(precision=precision, max_batch=4, **kw)
            c.load_weights(0, weights.retinaface_state_dict(0))
            c.load_weights(1, weights.yolov8n_state_dict(0))
            _NETS[key] = c
        c = _NETS[key]
        c.hold_reset()
        c.set_mask(kw.get("mask", "rect"), kw.get("mask_grow", 0))
        c.set_cells(kw.get("cells", 0))
        return c

    yield make
    for c in _NETS.values():
        c.close()
    _NETS.clear()


@pytest.fixture(scope="module")
def plain(gpu):
    """A weight-less context: the stand-alone blurring calls need no network."""
    import vdmi
    c = vdmi.Context(precision="fp32", max_batch=4)
    yield c
    c.close()


def _noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _yuv(buf, fd, h, w):
    """vdmi.Yuv420 over a padded buffer of yuv420_ref.padded (numpy: host; torch: where the tensor lives)."""
    import vdmi
    return vdmi.Yuv420(buf[fd["base"]:], h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"],
                       fd["chroma_step"], fd["frame_stride"])


# ---- letterbox -------------------------------------------------------------------------------------

SIZES = [(1080, 1920), (720, 1280), (480, 640), (334, 518), (48, 64), (2, 2)]
COLOURS = [("bt709", "limited"), ("bt601", "limited"), ("bt709", "full"), ("bt601", "full")]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("h,w", SIZES)
def test_letterbox_equals_the_nv12_letterbox(nets, h, w, precision):
    i = SIZES.index((h, w))
    m, r = COLOURS[i % 4]
    lay = yr.LAYOUTS[(i + (precision == "bf16")) % 4]      # the layouts rotate over the sizes
    nv = _noise(2, h, w, h + w)
    ctx = nets(precision)
    want = ctx.letterbox_nv12(_cuda(nv), matrix=m, range=r)
    assert np.abs(want).max() > 0
    s = yr.from_nv12(nv, lay)
    np.testing.assert_array_equal(ctx.letterbox_yuv420(_cuda(s), layout=lay, matrix=m, range=r), want, err_msg=lay)
    if precision == "fp32":                                 # every layout at every size once
        for other in yr.LAYOUTS:
            got = ctx.letterbox_yuv420(_cuda(yr.from_nv12(nv, other)), layout=other, matrix=m, range=r)
            np.testing.assert_array_equal(got, want, err_msg=other)


def test_letterbox_fp16_f32_canvas_and_a_padded_layout(nets, gpu):
    import torch
    import vdmi
    from vdmi import weights
    h, w = 480, 640
    nv = _noise(2, h, w, 11)
    ctx = nets("fp16")
    want = ctx.letterbox_nv12(nv, matrix="bt601")
    np.testing.assert_array_equal(ctx.letterbox_yuv420(yr.from_nv12(nv, "yv12"), layout="yv12", matrix="bt601"), want)
    # pitch 704, chroma_pitch 353 (odd: unaligned chroma rows), luma padded to 496 rows, V before U,
    # an extra stride; on the device and on the host
    buf, fd = yr.padded(yr.from_nv12(nv, "i420"), "i420", 704, 353, 496, True, 77)
    np.testing.assert_array_equal(ctx.letterbox_yuv420(_yuv(torch.from_numpy(buf).cuda(), fd, h, w), matrix="bt601"), want)
    np.testing.assert_array_equal(ctx.letterbox_yuv420(_yuv(buf, fd, h, w), matrix="bt601"), want)
    # the same with interleaved (V, U) pairs
    buf, fd = yr.padded(yr.from_nv12(nv, "nv21"), "nv21", 704, 706, 496, True, 77)
    np.testing.assert_array_equal(ctx.letterbox_yuv420(_yuv(torch.from_numpy(buf).cuda(), fd, h, w), matrix="bt601"), want)
    # the fp32 plan without the fused stem keeps an f32 NHWC canvas: the per-pixel kernel
    c32 = vdmi.Context(precision="fp32", max_batch=2, options={"stem_pool": 0})
    try:
        c32.load_weights(0, weights.retinaface_state_dict(0))
        for (hh, ww), lay in (((480, 640), "i420"), ((640, 1280), "nv21")):     # linear, exact 2x area
            g = _noise(2, hh, ww, hh)
            np.testing.assert_array_equal(c32.letterbox_yuv420(yr.from_nv12(g, lay), layout=lay), c32.letterbox_nv12(g))
    finally:
        c32.close()


# ---- detection -------------------------------------------------------------------------------------

def _scene(n, h, w, seed):
    """test_gpu_nv12.py::_scene: synthetic scenes on which the seeded weights fire, pixels doubled."""
    from vdmi import synth
    return np.stack([np.repeat(np.repeat(synth.frame(h // 2, w // 2, i, seed=seed), 2, 0), 2, 1) for i in range(n)])


def _fields_equal(a, b, n):
    total = 0
    assert np.array_equal(a.count[:n], b.count[:n])
    for i in range(n):
        for x, y in zip(a.frame(i), b.frame(i)):
            np.testing.assert_array_equal(x, y)
        total += int(a.count[i])
    return total


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("h,w,seed", [(360, 640, 5), (1080, 1920, 1)])
def test_process_yuv420_lists_equal_process_nv12(nets, h, w, seed, precision):
    from vdmi import _lib
    ctx = nets(precision)
    F, P = _lib.VD_PROC_FACES, _lib.VD_PROC_PLATES
    seen = {F: 0, P: 0}
    nv = nr.from_rgb(_scene(2, h, w, seed))
    for flags in (F, P, F | P):                          # F | P: the paired letterbox launch
        _, faces0, plates0 = ctx.process_nv12(nv, flags=flags)
        rb0 = [ctx.read_boxes(net, 2) for net, bit in ((0, F), (1, P)) if flags & bit]
        for lay in ("i420", "nv21"):
            _, faces, plates = ctx.process_yuv420(_cuda(yr.from_nv12(nv, lay)), flags=flags, layout=lay)
            rb = [ctx.read_boxes(net, 2) for net, bit in ((0, F), (1, P)) if flags & bit]
            if flags & F:
                seen[F] += _fields_equal(faces, faces0, 2)
            if flags & P:
                seen[P] += _fields_equal(plates, plates0, 2)
            for x, y in zip(rb, rb0):
                _fields_equal(x, y, 2)
    assert seen[F] > 0 and seen[P] > 0, seen              # the compared lists are not empty


# ---- pixelation of caller lists -----------------------------------------------------------------------

def _box_sets(h, w):
    return {
        "odd": [(3, 5, 41, 37), (w - 31, h - 23, w - 2, h - 1)],
        "chain": [(10, 10, 60, 50), (40, 30, 90, 70), (55, 5, 75, 64)],
        "off_and_empty": [(-20, -9, 17, 13), (w - 9, h - 7, w + 30, h + 30), (w + 5, 5, w + 40, 40), (30, 20, 30, 50),
                          (50, 40, 45, 60), (-50, -50, -10, -10), (20, 20, 44, 41)],
        "one_px": [(7, 9, 8, 10), (w - 1, h - 1, w, h), (0, 0, 1, 1), (12, 3, 13, 30), (2, 40, 70, 41)],
        "frame": [(0, 0, w, h), (11, 13, 50, 47)],
    }


def _mosaic_ref(f, lists, level, cells):
    return np.stack([nr.mosaic(f[i], lists[i], level, cells) for i in range(len(f))])


def _arrays(lists):
    cap = max(1, max(len(b) for b in lists))
    xy = np.zeros((len(lists), cap, 4), np.int32)
    for i, b in enumerate(lists):
        if b:
            xy[i, :len(b)] = np.asarray(b, np.int32)
    return xy, np.asarray([len(b) for b in lists], np.int32)


PAIRS = [("i420", "i420"), ("i420", "nv12"), ("nv12", "yv12"), ("yv12", "nv21")]


@pytest.mark.parametrize("level,cells", [(1, 0), (2, 0), (8, 0), (9, 0), (8, 4)])
@pytest.mark.parametrize("h,w", [(96, 128), (270, 480)])
def test_mosaic_yuv420_matches_the_plane_wise_reference(plain, h, w, level, cells):
    sets = _box_sets(h, w)
    names = sorted(sets)[:4]                                # max_batch = 4
    nv = _noise(len(names), h, w, 3 * h + level)
    lists = [sets[k] for k in names]
    xy, cnt = _arrays(lists)
    plain.set_cells(cells)
    try:
        want = _mosaic_ref(nv, lists, level, cells)
        for li, lo in PAIRS:
            s = yr.from_nv12(nv, li)
            got = plain.mosaic_yuv420(_cuda(s), xy, cnt, level=level, layout=li, out_layout=lo)
            np.testing.assert_array_equal(got.cpu().numpy(), yr.from_nv12(want, lo), err_msg=f"{li}->{lo} device")
        got = plain.mosaic_yuv420(yr.from_nv12(nv, "yv12"), xy, cnt, level=level, layout="yv12", out_layout="i420")
        np.testing.assert_array_equal(got, yr.from_nv12(want, "i420"), err_msg="host frames")
    finally:
        plain.set_cells(0)


@pytest.mark.parametrize("li,lo", PAIRS + [("nv21", "nv12"), ("nv21", "nv21")])
def test_mosaic_yuv420_padded_pairs_byte_and_vector_paths(plain, li, lo):
    """A padded, misaligned pair (odd pitches, a base off the 16-B grid: the byte path) and a padded,
    fully 16-B aligned pair (the vector path, with byte tails: w / 2 = 61 is no multiple of 16). Both
    match the reference, and every pad byte of the output keeps its 0xA5."""
    import torch
    h, w = 96, 122
    sets = _box_sets(h, w)
    lists = [sets["chain"] + sets["odd"], sets["off_and_empty"] + sets["frame"]]
    nv = _noise(2, h, w, 77)
    xy, cnt = _arrays(lists)
    want = _mosaic_ref(nv, lists, 8, 0)
    for pitch, cpi, cpo, extra, base_pad in ((131, 67, 71, 5, 3), (144, 80, 96, 48, 0)):
        step = lambda lay: 2 if lay.startswith("nv") else 1
        ibuf, ifd = yr.padded(yr.from_nv12(nv, li), li, pitch, cpi * step(li), h + 8, li in ("yv12", "nv21"), extra,
                              base_pad=base_pad)
        obuf, ofd = yr.padded(np.full_like(nv, 0xA5), lo, pitch + 16, cpo * step(lo), h + 2, lo in ("yv12", "nv21"),
                              extra + 16, base_pad=base_pad)
        dev_in, dev_out = torch.from_numpy(ibuf).cuda(), torch.from_numpy(obuf).cuda()
        plain.mosaic_yuv420(_yuv(dev_in, ifd, h, w), xy, cnt, level=8, out=_yuv(dev_out, ofd, h, w))
        plain.sync()
        o = dev_out.cpu().numpy()
        np.testing.assert_array_equal(yr.unpadded(o, ofd, 2, h, w, "nv12"), want, err_msg=f"pitch {pitch}")
        assert (o[~yr.picture_mask(ofd, 2, h, w, o.size)] == 0xA5).all(), f"pad bytes written, pitch {pitch}"
        np.testing.assert_array_equal(dev_in.cpu().numpy(), ibuf)


def test_mosaic_yuv420_past_every_capacity(plain):
    """Lists that cross NV12_BAND_BOXES (a band more than 32 boxes meet), NV12_CELLS (a band's slices
    hold more than 4096 cells) and NV12_LDS_BOXES (300 boxes in a frame), next to lists just below: the
    generic path for every step pair."""
    h, w = 96, 128
    rng = np.random.default_rng(9)

    def rand(k, side):
        out = []
        for _ in range(k):
            x1, y1 = int(rng.integers(-8, w - 4)), int(rng.integers(-8, h - 4))
            out.append((x1, y1, x1 + int(rng.integers(1, side)), y1 + int(rng.integers(1, side))))
        return out

    band = [(3 * i, 20, 3 * i + 30, 29) for i in range(NV12_BAND_BOXES + 4)]        # all meet rows 16..31
    nested = [(i, 0, w - i, h) for i in range(9)]                                   # level 2: (64 - i) x 8 luma cells per band
    cells = lambda k: sum((64 - i) * (NV12_ROWS // 2) for i in range(k))
    assert cells(8) <= NV12_CELLS < cells(9)
    cases = [(band[:NV12_BAND_BOXES], 2), (band, 2), (nested[:8], 2), (nested, 2), (rand(NV12_LDS_BOXES, 30), 3),
             (rand(NV12_LDS_BOXES + 44, 30), 3)]
    nv = _noise(1, h, w, 21)
    pairs = PAIRS + [("nv21", "nv21")]
    for k, (boxes, level) in enumerate(cases):
        xy, cnt = _arrays([boxes])
        want = _mosaic_ref(nv, [boxes], level, 0)
        for li, lo in (pairs if len(boxes) in (len(band), len(nested), NV12_LDS_BOXES + 44) else pairs[k % 4:k % 4 + 1]):
            got = plain.mosaic_yuv420(_cuda(yr.from_nv12(nv, li)), xy, cnt, level=level, layout=li, out_layout=lo)
            np.testing.assert_array_equal(got.cpu().numpy(), yr.from_nv12(want, lo), err_msg=f"{len(boxes)} boxes {li}->{lo}")


# ---- smooth blur and masks ---------------------------------------------------------------------------

def _all_flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _clip(seed=5):
    a, b, c = (nr.from_rgb(_scene(3, 360, 640, seed))[i] for i in range(3))
    return [a, a, b, b, c, a]


def test_smooth_and_mosaic_yuv420_in_an_ellipse_context_equal_the_nv12_calls(nets):
    h, w = 96, 128
    ctx = nets(**GAUSS)
    sets = _box_sets(h, w)
    lists = [sets["chain"] + sets["odd"], sets["off_and_empty"], sets["frame"][1:] + sets["one_px"]]
    xy, cnt = _arrays(lists)
    nv = _noise(3, h, w, 41)
    for level, cells in ((8, 8), (3, 2), (9, 5)):
        want_s = ctx.smooth_nv12(nv, xy, cnt, level=level, cells=cells)
        ctx.set_cells(cells)
        want_m = ctx.mosaic_nv12(nv, xy, cnt, level=level)           # the Gaussian context: the smooth blur too
        assert not np.array_equal(want_s, nv) and not np.array_equal(want_m, nv)
        for li, lo in (("i420", "i420"), ("nv12", "i420"), ("yv12", "nv21")):
            s = _cuda(yr.from_nv12(nv, li))
            got = ctx.smooth_yuv420(s, xy, cnt, level=level, cells=cells, layout=li, out_layout=lo)
            np.testing.assert_array_equal(got.cpu().numpy(), yr.from_nv12(want_s, lo), err_msg=f"smooth {li}->{lo}")
            got = ctx.mosaic_yuv420(s, xy, cnt, level=level, layout=li, out_layout=lo)
            np.testing.assert_array_equal(got.cpu().numpy(), yr.from_nv12(want_m, lo), err_msg=f"mosaic {li}->{lo}")
        got = ctx.smooth_yuv420(yr.from_nv12(nv, "i420"), xy, cnt, level=level, cells=cells)      # host frames
        np.testing.assert_array_equal(got, yr.from_nv12(want_s, "i420"))
    ctx.set_cells(8)


def test_process_yuv420_in_an_ellipse_context_equals_process_nv12(nets):
    ctx = nets(**GAUSS)
    nv = np.stack(_clip()[1:4])
    want, faces0, plates0 = ctx.process_nv12(nv, flags=_all_flags())
    assert not np.array_equal(want, nv) and int(faces0.count.sum()) > 0
    for li, lo in (("i420", "i420"), ("nv12", "i420")):
        out, faces, plates = ctx.process_yuv420(_cuda(yr.from_nv12(nv, li)), flags=_all_flags(), layout=li, out_layout=lo)
        _fields_equal(faces, faces0, 3)
        _fields_equal(plates, plates0, 3)
        np.testing.assert_array_equal(out.cpu().numpy(), yr.from_nv12(want, lo), err_msg=f"{li}->{lo}")
    # pixelation with rectangular masks, the same way
    ctx = nets("fp32")
    want, faces0, _ = ctx.process_nv12(nv, flags=_all_flags())
    out, faces, _ = ctx.process_yuv420(yr.from_nv12(nv, "yv12"), flags=_all_flags(), layout="yv12", out_layout="nv21")
    _fields_equal(faces, faces0, 3)
    np.testing.assert_array_equal(out, yr.from_nv12(want, "nv21"))
    assert not np.array_equal(want, nv)


# ---- hold and rescue -----------------------------------------------------------------------------------

def test_hold_and_rescue_over_calls_that_alternate_layouts(nets):
    frames = _clip()
    ctx = nets("fp32", hold=2, rescue=0.3)
    want = []
    for lo, n in ((0, 4), (4, 2)):
        out, faces, plates = ctx.process_nv12(np.stack(frames[lo:lo + n]), flags=_all_flags())
        held = ctx.read_held(n)
        resc = [ctx.read_rescue(net, n, "rescued") for net in (0, 1)]
        want.append((out, [(_lists(faces, i), _lists(plates, i), _lists(held, i), _lists(resc[0], i), _lists(resc[1], i))
                           for i in range(n)]))
    assert sum(len(r[2]) for _, rows in want for r in rows) > 0           # a non-zero held count
    ctx.hold_reset()
    for (lo, n), lay, (out_w, rows_w) in zip(((0, 4), (4, 2)), ("i420", "nv12"), want):
        batch = yr.from_nv12(np.stack(frames[lo:lo + n]), lay)
        out, faces, plates = ctx.process_yuv420(_cuda(batch), flags=_all_flags(), layout=lay)
        held = ctx.read_held(n)
        resc = [ctx.read_rescue(net, n, "rescued") for net in (0, 1)]
        rows = [(_lists(faces, i), _lists(plates, i), _lists(held, i), _lists(resc[0], i), _lists(resc[1], i))
                for i in range(n)]
        assert rows == rows_w, lay
        np.testing.assert_array_equal(out.cpu().numpy(), yr.from_nv12(out_w, lay), err_msg=lay)


# ---- equivalence with the NV12 entry ----------------------------------------------------------------

def test_the_nv12_layout_through_the_new_entry_is_the_old_entry(nets):
    import torch
    ctx = nets("fp32", hold=2)
    nv = np.stack(_clip()[:3])
    dev = torch.from_numpy(nv).cuda()
    ctx.hold_reset()
    want, faces0, plates0 = ctx.process_nv12(dev, flags=_all_flags())
    held0 = [_lists(ctx.read_held(3), i) for i in range(3)]
    ctx.hold_reset()
    out, faces, plates = ctx.process_yuv420(dev, flags=_all_flags(), layout="nv12")
    assert [_lists(ctx.read_held(3), i) for i in range(3)] == held0
    assert _fields_equal(faces, faces0, 3) > 0
    _fields_equal(plates, plates0, 3)
    assert torch.equal(out, want) and not torch.equal(out, dev)           # both planes, byte for byte


def test_rgb_nv12_and_i420_calls_interleaved_on_one_context(nets):
    """Calls of the three kinds on one context and stream: each gives what it gives alone."""
    ctx = nets("fp32")
    nv = np.stack(_clip()[2:5])
    rgb = nr.to_rgb(nv)
    i420 = yr.from_nv12(nv, "i420")
    alone = []
    for call in (lambda: ctx.process(rgb, flags=_all_flags()), lambda: ctx.process_nv12(nv, flags=_all_flags()),
                 lambda: ctx.process_yuv420(i420, flags=_all_flags())):
        ctx.hold_reset()
        out, faces, plates = call()
        alone.append((np.array(out), [_lists(faces, i) + _lists(plates, i) for i in range(3)]))
    ctx.hold_reset()
    for order in ((2, 0, 1), (1, 2, 0), (2, 2, 1)):
        for k in order:
            out, faces, plates = (ctx.process(rgb, flags=_all_flags()) if k == 0 else
                                  ctx.process_nv12(nv, flags=_all_flags()) if k == 1 else
                                  ctx.process_yuv420(i420, flags=_all_flags()))
            assert [_lists(faces, i) + _lists(plates, i) for i in range(3)] == alone[k][1]
            np.testing.assert_array_equal(out, alone[k][0])
    np.testing.assert_array_equal(alone[2][0], yr.from_nv12(alone[1][0], "i420"))
    assert sum(len(x) for x in alone[2][1]) > 0


# ---- refusals ---------------------------------------------------------------------------------------

def test_state_refusals_leave_the_next_call_unchanged(nets):
    import vdmi
    from vdmi import _lib, weights
    nv = np.stack(_clip()[:2])
    i420 = yr.from_nv12(nv, "i420")
    xy, cnt = _arrays([[(10, 10, 60, 50)]] * 2)
    ctx = nets(blur="gaussian", cells=8)
    want, faces_w, _ = ctx.process_yuv420(i420, flags=_all_flags())
    # the fixed-kernel Gaussian: cells off in a Gaussian context
    ctx.set_cells(0)
    for call in (lambda: ctx.process_yuv420(i420, flags=_all_flags()), lambda: ctx.mosaic_yuv420(i420, xy, cnt, level=8)):
        with pytest.raises(_lib.VdError, match="cells") as e:
            call()
        assert e.value.code == _lib.VD_ERR_STATE
    ctx.set_cells(8)
    # a call that would run a tiled net
    ctx.set_tiles((2, 2), 20)
    try:
        with pytest.raises(_lib.VdError, match="tile") as e:
            ctx.process_yuv420(i420[:1], flags=_all_flags())
        assert e.value.code == _lib.VD_ERR_STATE
    finally:
        ctx.set_tiles((1, 1), 20)
    ctx.hold_reset()
    out, faces, _ = ctx.process_yuv420(i420, flags=_all_flags())
    np.testing.assert_array_equal(out, want)
    assert _fields_equal(faces, faces_w, 2) > 0 and not np.array_equal(out, i420)
    # VD_PROC_MOSAIC in a look-ahead context
    lead = nets(lead=2)
    with pytest.raises(_lib.VdError, match="look-ahead") as e:
        lead.process_yuv420(i420, flags=_all_flags())
    assert e.value.code == _lib.VD_ERR_STATE
    _, faces, _ = lead.process_yuv420(i420, flags=_lib.VD_PROC_FACES)        # detection alone is vd_process's
    _fields_equal(faces, faces_w, 2)


def test_err_arg_cases_on_device_descriptors(nets):
    """The overlap rule and the descriptor rules through vd_process_yuv420, between two calls of a
    holding stream: the second call gives what it gives in a stream that never saw the refusals."""
    import torch
    from vdmi import _lib
    frames = _clip()
    first, second = (yr.from_nv12(np.stack(x), "i420") for x in (frames[:2], frames[2:5]))
    ctx = nets("fp32", hold=2)
    ctx.process_yuv420(first, flags=_all_flags())
    out_w, faces_w, _ = ctx.process_yuv420(second, flags=_all_flags())
    held_w = [_lists(ctx.read_held(3), i) for i in range(3)]
    ctx.hold_reset()
    ctx.process_yuv420(first, flags=_all_flags())

    h, w = 360, 640
    dev = torch.from_numpy(second).cuda()
    dout = torch.empty_like(dev)
    fb = h * w * 3 // 2
    good = dict(pitch=w, u=h * w, v=h * w * 5 // 4, cp=w // 2, st=fb, step=1, matrix=1, range=0)

    def call(n=3, hh=h, ww=w, out=True, obase=dout.data_ptr(), **kw):
        d = dict(good, **kw)
        i = _lib.vd_yuv420(dev.data_ptr(), d["pitch"], d["u"], d["v"], d["cp"], d["st"], d["step"], d["matrix"], d["range"])
        o = _lib.vd_yuv420(obase, w, h * w, h * w + 1, w, fb, 2, 0, 0)
        return ctx._lib.vd_process_yuv420(ctx._h, ctypes.byref(i), ctypes.byref(o) if out else None, n, hh, ww,
                                          _lib.VD_DEVICE, _all_flags(), None, None)

    bad = [dict(hh=359), dict(ww=639), dict(hh=0), dict(n=0), dict(n=5), dict(pitch=w - 2), dict(cp=w // 2 - 1),
           dict(step=3), dict(step=2, cp=w), dict(u=h * w - 1), dict(v=h * w * 5 // 4 - 1), dict(st=fb - 1),
           dict(matrix=2), dict(range=7), dict(out=False), dict(obase=dev.data_ptr()),
           dict(obase=dev.data_ptr() + 3 * fb - 16), dict(obase=dev.data_ptr() - 3 * fb + 16)]
    for kw in bad:
        assert call(**kw) == _lib.VD_ERR_ARG, kw
    out, faces, _ = ctx.process_yuv420(second, flags=_all_flags())
    assert [_lists(ctx.read_held(3), i) for i in range(3)] == held_w and sum(len(x) for x in held_w) > 0
    _fields_equal(faces, faces_w, 3)
    np.testing.assert_array_equal(out, out_w)
