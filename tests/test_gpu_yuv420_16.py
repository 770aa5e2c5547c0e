"""10- and 12-bit 4:2:0 frames on the GPU (include/vdmi.h at vd_yuv420_16; csrc/pre.hip, nv12.hip,
smooth.hip, mask.hip). Detection is compared with the *_yuv420 call on D(S), the 8-bit picture of the
surface; pixelation with the lo / hi definition; the smooth blur and the ellipse with the numpy
reference on values (tests/yuv420_16_ref.py). Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import nv12_ref as nr
import yuv420_16_ref as y16
import yuv420_ref as yr

pytestmark = pytest.mark.gpu

# csrc/nv12.hip
NV12_ROWS, NV12_LDS_BOXES, NV12_BAND_BOXES, NV12_CELLS = 16, 256, 32, 4096
GAUSS = dict(blur="gaussian", cells=8, mask="ellipse", mask_grow=42)
P010 = ("nv12", 10, 6)                 # layout, depth, shift
P12 = ("i420", 12, 0)                  # yuv420p12le
SIZES = [(1080, 1920), (720, 1280), (480, 640), (334, 518), (48, 64), (2, 2)]   # tests/test_gpu_yuv420.py

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


def _noise8(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cuda16(a):
    """uint16 words on the device (as int16: the one 16-bit integer type every torch moves)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda()


def _np16(x):
    return x.cpu().numpy().view(np.uint16) if hasattr(x, "cpu") else np.asarray(x).view(np.uint16)


def _y16(buf, fd, h, w, depth, shift):
    """vdmi.Yuv420_16 over a padded buffer of yuv420_16_ref.padded (numpy uint16, or a torch int16 tensor)."""
    import vdmi
    return vdmi.Yuv420_16(buf[fd["base"] // 2:], h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"],
                          fd["chroma_step"], fd["frame_stride"], depth=depth, shift=shift)


# ---- 1. letterbox -------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("h,w", SIZES)
def test_letterbox_equals_the_8_bit_letterbox_on_D(nets, h, w, precision):
    """P010 and planar depth 12, packed and (one of the two, alternating) padded and misaligned: the word
    path. The unused bits and the value bits below the top eight are noise."""
    i = SIZES.index((h, w))
    m, r = (("bt709", "limited"), ("bt601", "limited"), ("bt709", "full"), ("bt601", "full"))[i % 4]
    ctx = nets(precision)
    for k, (lay, depth, shift) in enumerate((P010, P12)):
        s8 = yr.from_nv12(_noise8(2, h, w, h + w + k), lay)
        want = ctx.letterbox_yuv420(_cuda(s8), layout=lay, matrix=m, range=r)
        assert np.abs(want).max() > 0
        s = y16.widen(s8, depth, shift, i)
        assert np.array_equal(y16.D(s, depth, shift), s8) and (s != y16.values(s, depth, shift) << shift).any()
        got = ctx.letterbox_yuv420_16(_cuda16(s), layout=lay, depth=depth, shift=shift, matrix=m, range=r)
        np.testing.assert_array_equal(got, want, err_msg=f"{lay} packed")
        if (i + k) % 2 == 0:
            step = 2 if lay in y16.INTERLEAVED else 1
            buf, fd = y16.padded(s, lay, w + 21, (w // 2 + 9) * step, h + 6, k == 1, 13, base_pad_w=3)
            got = ctx.letterbox_yuv420_16(_y16(_cuda16(buf), fd, h, w, depth, shift), matrix=m, range=r)
            np.testing.assert_array_equal(got, want, err_msg=f"{lay} padded, device")
            if h <= 480:
                got = ctx.letterbox_yuv420_16(_y16(buf, fd, h, w, depth, shift), matrix=m, range=r)
                np.testing.assert_array_equal(got, want, err_msg=f"{lay} padded, host")


def test_letterbox_f32_canvas_kernel(gpu):
    """The fp32 plan without the fused stem keeps an f32 NHWC canvas: the per-pixel kernel."""
    import vdmi
    from vdmi import weights
    c32 = vdmi.Context(precision="fp32", max_batch=2, options={"stem_pool": 0})
    try:
        c32.load_weights(0, weights.retinaface_state_dict(0))
        for (hh, ww), (lay, depth, shift) in (((480, 640), P12), ((640, 1280), ("nv21", 10, 6))):   # linear, exact 2x area
            s8 = yr.from_nv12(_noise8(2, hh, ww, hh), lay)
            s = y16.widen(s8, depth, shift, 3)
            np.testing.assert_array_equal(c32.letterbox_yuv420_16(s, layout=lay, depth=depth, shift=shift),
                                          c32.letterbox_yuv420(s8, layout=lay))
    finally:
        c32.close()


# ---- 2. process -------------------------------------------------------------------------------------

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


def _all_flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _arrays(lists):
    cap = max(1, max(len(b) for b in lists))
    xy = np.zeros((len(lists), cap, 4), np.int32)
    for i, b in enumerate(lists):
        if b:
            xy[i, :len(b)] = np.asarray(b, np.int32)
    return xy, np.asarray([len(b) for b in lists], np.int32)


_CLIP = []


def _clip(seed=5):
    if not _CLIP:
        a, b, c = (nr.from_rgb(_scene(3, 360, 640, seed))[i] for i in range(3))
        _CLIP.extend([a, a, b, b, c, a])
    return _CLIP


def test_process_pixelation_lists_and_pixels(nets):
    from vdmi import _lib
    ctx = nets("fp32")
    F, P = _lib.VD_PROC_FACES, _lib.VD_PROC_PLATES
    nv8 = np.stack(_clip()[1:4])
    n = len(nv8)
    total = 0
    for (lay, depth, shift), lo in ((P010, "nv12"), (P12, "nv21")):
        s8 = yr.from_nv12(nv8, lay)
        s = y16.widen(s8, depth, shift, depth)
        out8, faces0, plates0 = ctx.process_yuv420(_cuda(s8), flags=_all_flags(), layout=lay, out_layout=lo)
        rb0 = [ctx.read_boxes(net, n) for net in (0, 1)]
        out, faces, plates = ctx.process_yuv420_16(_cuda16(s), flags=_all_flags(), layout=lay, out_layout=lo, depth=depth,
                                                   shift=shift)
        rb = [ctx.read_boxes(net, n) for net in (0, 1)]
        total += _fields_equal(faces, faces0, n) + _fields_equal(plates, plates0, n)
        for x, y in zip(rb, rb0):
            _fields_equal(x, y, n)
        out = _np16(out)
        # the definition: the low and the high bytes as vd_mosaic_yuv420 pixelates them with the blurred list
        xy, cnt = _arrays([_lists(faces, i) + _lists(plates, i) for i in range(n)])
        want = y16.join(*(ctx.mosaic_yuv420(_cuda(half(s)), xy, cnt, layout=lay, out_layout=lo).cpu().numpy()
                          for half in (y16.lo, y16.hi)))
        np.testing.assert_array_equal(out, want, err_msg=lay)
        np.testing.assert_array_equal(y16.D(out, depth, shift), out8.cpu().numpy())
        assert not np.array_equal(out, y16.relayout(s, lay, lo))
        # detection alone, and one net at a time (the unpaired letterbox launches)
        for flags in (F, P):
            _, f0, p0 = ctx.process_yuv420(_cuda(s8), flags=flags, layout=lay)
            _, f1, p1 = ctx.process_yuv420_16(_cuda16(s), flags=flags, layout=lay, depth=depth, shift=shift)
            _fields_equal(f1, f0, n) if flags == F else _fields_equal(p1, p0, n)
    assert total > 0


def test_process_in_the_gaussian_cells_ellipse_context(nets):
    ctx = nets(**GAUSS)
    nv8 = np.stack(_clip()[1:4])
    n = len(nv8)
    level = ctx.cfg.mosaic_level
    for (lay, depth, shift), lo, host in ((P010, "i420", False), (P12, "nv12", True)):
        s8 = yr.from_nv12(nv8, lay)
        s = y16.widen(s8, depth, shift, 7)
        _, faces0, plates0 = ctx.process_yuv420(s8, flags=_all_flags(), layout=lay)
        out, faces, plates = ctx.process_yuv420_16(s if host else _cuda16(s), flags=_all_flags(), layout=lay, out_layout=lo,
                                                   depth=depth, shift=shift)
        assert _fields_equal(faces, faces0, n) > 0
        _fields_equal(plates, plates0, n)
        src = y16.relayout(s, lay, "nv12")
        want = np.stack([y16.shaped(src[i], _lists(faces, i) + _lists(plates, i), "ellipse", 42,
                                    lambda f, g: y16.smooth(f, g, level, 8, depth, shift)) for i in range(n)])
        assert not np.array_equal(want, src)
        np.testing.assert_array_equal(y16.relayout(_np16(out), lo, "nv12"), want, err_msg=lay)


def test_hold_and_rescue_over_calls_that_alternate_8_and_16_bit_surfaces(nets):
    frames = _clip()
    ctx = nets("fp32", hold=2, rescue=0.3)
    calls = ((0, 4), (4, 2))

    def rows_of(faces, plates, n):
        held = ctx.read_held(n)
        resc = [ctx.read_rescue(net, n, "rescued") for net in (0, 1)]
        return [(_lists(faces, i), _lists(plates, i), _lists(held, i), _lists(resc[0], i), _lists(resc[1], i)) for i in range(n)]

    want = []
    for lo, n in calls:
        out, faces, plates = ctx.process_yuv420(yr.from_nv12(np.stack(frames[lo:lo + n]), "i420"), flags=_all_flags())
        want.append((yr.to_nv12(out, "i420"), rows_of(faces, plates, n)))
    assert sum(len(r[2]) for _, rows in want for r in rows) > 0           # a non-zero held count
    assert sum(len(r[0]) for _, rows in want for r in rows) > 0
    for wide_first in (True, False):
        ctx.hold_reset()
        for k, ((lo, n), (out_w, rows_w)) in enumerate(zip(calls, want)):
            nv8 = np.stack(frames[lo:lo + n])
            if (k == 0) == wide_first:
                lay, depth, shift = P010 if wide_first else P12
                s = y16.widen(yr.from_nv12(nv8, lay), depth, shift, k)
                out, faces, plates = ctx.process_yuv420_16(_cuda16(s), flags=_all_flags(), layout=lay, depth=depth, shift=shift)
                out8 = yr.to_nv12(y16.D(_np16(out), depth, shift), lay)
            else:
                out, faces, plates = ctx.process_yuv420(_cuda(yr.from_nv12(nv8, "yv12")), flags=_all_flags(), layout="yv12")
                out8 = yr.to_nv12(out.cpu().numpy(), "yv12")
            assert rows_of(faces, plates, n) == rows_w, (wide_first, k)
            np.testing.assert_array_equal(out8, out_w, err_msg=f"{wide_first} {k}")


# ---- 3. mosaic and smooth with caller lists ---------------------------------------------------------------

def _box_sets(h, w):
    return {
        "odd": [(3, 5, 41, 37), (w - 31, h - 23, w - 2, h - 1)],
        "chain": [(10, 10, 60, 50), (40, 30, 90, 70), (55, 5, 75, 64)],                  # unequal levels under cells
        "equal": [(10, 10, 50, 50), (30, 30, 70, 70), (20, 40, 60, 80)],                 # equal levels, overlapping
        "borders": [(-20, -9, 17, 13), (w - 9, h - 7, w + 30, h + 30), (w + 5, 5, w + 40, 40), (30, 20, 30, 50),
                    (50, 40, 45, 60), (-50, -50, -10, -10), (20, -5, 44, 11), (-7, 30, 9, 52), (60, h - 9, 90, h + 4),
                    (w - 6, 33, w + 8, 61)],
        "small": [(7, 9, 8, 10), (w - 1, h - 1, w, h), (0, 0, 1, 1), (12, 3, 13, 30), (2, 40, 70, 41), (5, 5, 7, 7),
                  (w - 2, h - 2, w, h), (21, 9, 23, 40), (33, 60, 80, 62)],
        "frame": [(0, 0, w, h), (11, 13, 50, 47)],
    }


def _four_lists(h, w):
    s = _box_sets(h, w)
    return [s["odd"] + s["small"], s["borders"] + s["frame"][1:], s["chain"] + s["equal"], []]


FORMATS = [("nv12", "nv12", 10, 6), ("i420", "nv12", 10, 0), ("nv12", "yv12", 12, 4), ("yv12", "nv21", 12, 0),
           ("nv21", "i420", 10, 3)]
_REF = {}


def _reference(kind, h, w, depth, shift, level, cells, seed=31):
    """(NV12-layout uint16 input frames, expected frames) of the four lists, computed once per case."""
    key = (kind, h, w, depth, shift, level, cells, seed)
    if key not in _REF:
        src = y16.noise(4, h, w, depth, shift, seed)
        lists = _four_lists(h, w)
        if kind == "mosaic":
            want = y16.mosaic(src, lists, level, cells)
        else:
            want = np.stack([y16.smooth(src[i], lists[i], level, cells, depth, shift) for i in range(4)])
        assert (not np.array_equal(want[:3], src[:3]) or (kind, level, cells) == ("mosaic", 1, 0)) and np.array_equal(want[3], src[3])
        _REF[key] = (src, want)
    return _REF[key]


@pytest.mark.parametrize("level,cells", [(1, 0), (8, 0), (9, 0), (8, 4)])
def test_mosaic_matches_the_lo_hi_definition(plain, level, cells):
    h, w = 96, 128
    xy, cnt = _arrays(_four_lists(h, w))
    plain.set_cells(cells)
    try:
        for li, lo, depth, shift in FORMATS:
            src, want = _reference("mosaic", h, w, depth, shift, level, cells)
            got = plain.mosaic_yuv420_16(_cuda16(y16.relayout(src, "nv12", li)), xy, cnt, level=level, layout=li, out_layout=lo,
                                         depth=depth, shift=shift)
            np.testing.assert_array_equal(_np16(got), y16.relayout(want, "nv12", lo), err_msg=f"{li}->{lo} device")
        li, lo, depth, shift = FORMATS[3]
        src, want = _reference("mosaic", h, w, depth, shift, level, cells)
        got = plain.mosaic_yuv420_16(y16.relayout(src, "nv12", li), xy, cnt, level=level, layout=li, out_layout=lo,
                                     depth=depth, shift=shift)
        np.testing.assert_array_equal(got, y16.relayout(want, "nv12", lo), err_msg="host frames")
    finally:
        plain.set_cells(0)


@pytest.mark.parametrize("level,cells", [(8, 8), (3, 2), (9, 5), (1, 64)])
def test_smooth_matches_the_reference_on_values(plain, level, cells):
    h, w = 96, 128
    xy, cnt = _arrays(_four_lists(h, w))
    for li, lo, depth, shift in FORMATS:
        src, want = _reference("smooth", h, w, depth, shift, level, cells)
        got = plain.smooth_yuv420_16(_cuda16(y16.relayout(src, "nv12", li)), xy, cnt, level=level, cells=cells, layout=li,
                                     out_layout=lo, depth=depth, shift=shift)
        np.testing.assert_array_equal(_np16(got), y16.relayout(want, "nv12", lo), err_msg=f"{li}->{lo} device")
    li, lo, depth, shift = FORMATS[1]
    src, want = _reference("smooth", h, w, depth, shift, level, cells)
    got = plain.smooth_yuv420_16(y16.relayout(src, "nv12", li), xy, cnt, level=level, cells=cells, layout=li, out_layout=lo,
                                 depth=depth, shift=shift)
    np.testing.assert_array_equal(got, y16.relayout(want, "nv12", lo), err_msg="host frames")


@pytest.mark.parametrize("kind", ["mosaic", "smooth"])
@pytest.mark.parametrize("li,lo,depth,shift", FORMATS + [("i420", "i420", 12, 4)])
def test_padded_pairs_word_and_vector_paths(plain, kind, li, lo, depth, shift):
    """A padded, misaligned pair (odd word pitches, a base 6 bytes off the 16-B grid: the word path) and a
    padded, fully 16-B aligned pair (the vector path with its tails: w / 2 = 61). Both match the reference,
    on the device and from host memory, and every pad word of the output keeps its 0xA5A5."""
    h, w = 96, 122
    level, cells = (8, 0) if kind == "mosaic" else (5, 6)
    xy, cnt = _arrays(_four_lists(h, w))
    src, want = _reference(kind, h, w, depth, shift, level, cells, seed=77)
    step = lambda lay: 2 if lay in y16.INTERLEAVED else 1
    call = plain.mosaic_yuv420_16 if kind == "mosaic" else plain.smooth_yuv420_16
    kw = dict(level=level) if kind == "mosaic" else dict(level=level, cells=cells)
    for pitch, cpi, cpo, extra, base_pad in ((131, 67, 71, 5, 3), (144, 80, 96, 48, 0)):
        ibuf, ifd = y16.padded(y16.relayout(src, "nv12", li), li, pitch, cpi * step(li), h + 8, li in ("yv12", "nv21"), extra,
                               base_pad_w=base_pad)
        obuf, ofd = y16.padded(np.full_like(src, 0xA5A5), lo, pitch + 16, cpo * step(lo), h + 2, lo in ("yv12", "nv21"),
                               extra + 16, base_pad_w=base_pad)
        for host in (False, True):
            if host and (pitch, li) not in ((131, "nv12"), (144, "yv12")):
                continue
            din, dout = (ibuf.copy(), obuf.copy()) if host else (_cuda16(ibuf), _cuda16(obuf))
            call(_y16(din, ifd, h, w, depth, shift), xy, cnt, out=_y16(dout, ofd, h, w, depth, shift), **kw)
            plain.sync()
            o = _np16(dout)
            np.testing.assert_array_equal(y16.unpadded(o, ofd, 4, h, w, "nv12"), want, err_msg=f"pitch {pitch} host {host}")
            assert (o[~y16.picture_mask(ofd, 4, h, w, o.size)] == 0xA5A5).all(), f"pad words written, pitch {pitch}"
            np.testing.assert_array_equal(_np16(din), ibuf)


def test_ellipse_mask_on_caller_lists(nets):
    """The Gaussian + cells + ellipse context on caller lists: the restore copies words."""
    h, w = 96, 128
    ctx = nets(**GAUSS)
    lists = _four_lists(h, w)
    xy, cnt = _arrays(lists)
    for li, lo, depth, shift in FORMATS[:3]:
        src = y16.noise(4, h, w, depth, shift, 41)
        for level, cells in ((8, 8), (3, 2)):
            ctx.set_cells(cells)
            want = np.stack([y16.shaped(src[i], lists[i], "ellipse", 42, lambda f, g: y16.smooth(f, g, level, cells, depth, shift))
                             for i in range(4)])
            got = ctx.mosaic_yuv420_16(_cuda16(y16.relayout(src, "nv12", li)), xy, cnt, level=level, layout=li, out_layout=lo,
                                       depth=depth, shift=shift)          # the Gaussian context: the smooth blur
            np.testing.assert_array_equal(_np16(got), y16.relayout(want, "nv12", lo), err_msg=f"{li}->{lo}")
    # pixelation under the ellipse, in a context of its own mask setting
    pix = nets("fp32", mask="ellipse", mask_grow=42)
    li, lo, depth, shift = FORMATS[2]
    src = y16.noise(4, h, w, depth, shift, 43)
    want = np.stack([y16.shaped(src[i], lists[i], "ellipse", 42, lambda f, g: y16.mosaic(f[None], [g], 8, 0)[0]) for i in range(4)])
    got = pix.mosaic_yuv420_16(_cuda16(y16.relayout(src, "nv12", li)), xy, cnt, level=8, layout=li, out_layout=lo, depth=depth,
                               shift=shift)
    np.testing.assert_array_equal(_np16(got), y16.relayout(want, "nv12", lo))
    ctx.set_cells(8)


# ---- 4. the arithmetic extreme ----------------------------------------------------------------------------

def test_largest_T_the_format_allows(plain):
    """A 4 x 4 frame of all-4095 samples at depth 12, level 32768, cells 2, one box over the frame: t = 65520
    and T + 16f = 65536 * 65520 + 16 * 32768, the largest the format allows. Every output value is 4095."""
    for lay, shift in (("i420", 0), ("nv12", 4)):
        s = np.full((1, 6, 4), 4095 << shift, np.uint16)
        s |= np.uint16(0 if shift == 0 else 0xF)                       # unused bits set: they must come back zero
        got = _np16(plain.smooth_yuv420_16(_cuda16(s), [[(0, 0, 4, 4)]], level=32768, cells=2, layout=lay, depth=12, shift=shift))
        assert (y16.values(got, 12, shift) == 4095).all() and (got == 4095 << shift).all(), lay
    # the sums' widths either side of the 64-bit threshold, all-4095 frames of 96 x 128
    h, w = 96, 128
    s = np.full((1, h * 3 // 2, w), 4095 << 4, np.uint16)
    for level in (1024, 1025, 700):
        got = _np16(plain.smooth_yuv420_16(_cuda16(s), [[(0, 0, w, h), (-500, -500, 700, 600)]], level=level, cells=2,
                                           layout="nv12", depth=12, shift=4))
        assert (got == 4095 << 4).all(), level


# ---- 5. capacities -----------------------------------------------------------------------------------------

def test_mosaic_past_every_capacity(plain):
    """The lists of test_mosaic_yuv420_past_every_capacity -- past NV12_BAND_BOXES, NV12_CELLS and
    NV12_LDS_BOXES, next to lists just below -- on 16-bit surfaces: the generic path for every step pair."""
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
    pairs = [f[:2] for f in FORMATS]
    src = y16.noise(1, h, w, 10, 6, 21)
    for k, (boxes, level) in enumerate(cases):
        xy, cnt = _arrays([boxes])
        want = y16.mosaic(src, [boxes], level, 0)
        for li, lo in (pairs if len(boxes) in (len(band), len(nested), NV12_LDS_BOXES + 44) else pairs[k % 4:k % 4 + 1]):
            got = plain.mosaic_yuv420_16(_cuda16(y16.relayout(src, "nv12", li)), xy, cnt, level=level, layout=li, out_layout=lo,
                                         depth=10, shift=6)
            np.testing.assert_array_equal(_np16(got), y16.relayout(want, "nv12", lo), err_msg=f"{len(boxes)} boxes {li}->{lo}")


# ---- 6. refusals -------------------------------------------------------------------------------------------

def test_refusals_leave_the_next_call_unchanged(nets):
    import vdmi
    from vdmi import _lib
    lay, depth, shift = P010
    nv8 = np.stack(_clip()[:2])
    s = y16.widen(yr.from_nv12(nv8, lay), depth, shift, 1)
    xy, cnt = _arrays([[(10, 10, 60, 50)]] * 2)
    kw = dict(layout=lay, depth=depth, shift=shift)
    ctx = nets(blur="gaussian", cells=8)
    want, faces_w, _ = ctx.process_yuv420_16(s, flags=_all_flags(), **kw)

    def unchanged():
        ctx.hold_reset()
        out, faces, _ = ctx.process_yuv420_16(s, flags=_all_flags(), **kw)
        np.testing.assert_array_equal(out, want)
        assert _fields_equal(faces, faces_w, 2) > 0 and not np.array_equal(out, s)

    # the fixed-kernel Gaussian: cells off in a Gaussian context
    ctx.set_cells(0)
    for call in (lambda: ctx.process_yuv420_16(s, flags=_all_flags(), **kw), lambda: ctx.mosaic_yuv420_16(s, xy, cnt, level=8, **kw)):
        with pytest.raises(_lib.VdError, match="cells") as e:
            call()
        assert e.value.code == _lib.VD_ERR_STATE
    ctx.set_cells(8)
    unchanged()
    # a call that would run a tiled net
    ctx.set_tiles((2, 2), 20)
    try:
        with pytest.raises(_lib.VdError, match="tile") as e:
            ctx.process_yuv420_16(s[:1], flags=_all_flags(), **kw)
        assert e.value.code == _lib.VD_ERR_STATE
    finally:
        ctx.set_tiles((1, 1), 20)
    unchanged()
    # out.depth != in.depth, out.shift != in.shift
    h, w = 360, 640
    for od, osh in ((12, 4), (10, 0)):
        o = vdmi.Yuv420_16(np.zeros_like(s), h, w, 2 * w, 2 * h * w, 2 * h * w + 2, 2 * w, 2, 3 * h * w, depth=od, shift=osh)
        for call in (lambda: ctx.process_yuv420_16(s, out=o, flags=_all_flags(), **kw),
                     lambda: ctx.mosaic_yuv420_16(s, xy, cnt, level=8, out=o, **kw),
                     lambda: ctx.smooth_yuv420_16(s, xy, cnt, level=8, cells=4, out=o, **kw)):
            with pytest.raises(_lib.VdError, match="depth") as e:
                call()
            assert e.value.code == _lib.VD_ERR_ARG
        assert not o.buffer.any()
    unchanged()
    # VD_PROC_MOSAIC in a look-ahead context
    lead = nets(lead=2)
    with pytest.raises(_lib.VdError, match="look-ahead") as e:
        lead.process_yuv420_16(s, flags=_all_flags(), **kw)
    assert e.value.code == _lib.VD_ERR_STATE
    _, faces, _ = lead.process_yuv420_16(s, flags=_lib.VD_PROC_FACES, **kw)        # detection alone is vd_process's
    _fields_equal(faces, faces_w, 2)
    _, faces0, _ = lead.process_yuv420(yr.from_nv12(nv8, lay), flags=_lib.VD_PROC_FACES, layout=lay)
    _fields_equal(faces, faces0, 2)


def test_descriptor_rules_through_the_device_entry(nets):
    """The descriptor rules and the overlap rule through vd_process_yuv420_16 between two calls of a holding
    stream: the second call gives what it gives in a stream that never saw the refusals."""
    import torch
    from vdmi import _lib
    frames = _clip()
    lay, depth, shift = P12
    first, second = (y16.widen(yr.from_nv12(np.stack(x), lay), depth, shift, 2) for x in (frames[:2], frames[2:5]))
    kw = dict(layout=lay, depth=depth, shift=shift)
    ctx = nets("fp32", hold=2)
    ctx.process_yuv420_16(first, flags=_all_flags(), **kw)
    out_w, faces_w, _ = ctx.process_yuv420_16(second, flags=_all_flags(), **kw)
    held_w = [_lists(ctx.read_held(3), i) for i in range(3)]
    ctx.hold_reset()
    ctx.process_yuv420_16(first, flags=_all_flags(), **kw)

    h, w = 360, 640
    dev = _cuda16(second)
    dout = torch.empty_like(dev)
    yb = 2 * h * w
    fb = yb * 3 // 2
    good = dict(pitch=2 * w, u=yb, v=yb + yb // 4, cp=w, st=fb, step=1, matrix=1, range=0, depth=12, shift=0)

    def call(n=3, hh=h, ww=w, out=True, obase=dout.data_ptr(), odepth=12, oshift=0, base=dev.data_ptr(), **k2):
        d = dict(good, **k2)
        i = _lib.vd_yuv420_16(base, d["pitch"], d["u"], d["v"], d["cp"], d["st"], d["step"], d["matrix"], d["range"],
                              d["depth"], d["shift"])
        o = _lib.vd_yuv420_16(obase, 2 * w, yb, yb + 2, 2 * w, fb, 2, 0, 0, odepth, oshift)
        return ctx._lib.vd_process_yuv420_16(ctx._h, ctypes.byref(i), ctypes.byref(o) if out else None, n, hh, ww,
                                             _lib.VD_DEVICE, _all_flags(), None, None)

    bad = [dict(hh=359), dict(ww=639), dict(hh=0), dict(n=0), dict(n=5), dict(pitch=2 * w - 2), dict(pitch=2 * w + 1),
           dict(cp=w - 2), dict(cp=w + 1), dict(step=3), dict(step=2, cp=2 * w), dict(u=yb - 2), dict(u=yb + 1),
           dict(v=yb + yb // 4 - 2), dict(st=fb - 2), dict(st=fb + 1), dict(matrix=2), dict(range=7), dict(depth=8),
           dict(depth=16), dict(shift=5), dict(shift=-1), dict(base=dev.data_ptr() + 1), dict(out=False), dict(odepth=10),
           dict(oshift=2), dict(obase=dev.data_ptr()), dict(obase=dev.data_ptr() + 3 * fb - 16),
           dict(obase=dev.data_ptr() - 3 * fb + 16)]
    for k2 in bad:
        assert call(**k2) == _lib.VD_ERR_ARG, k2
    out, faces, _ = ctx.process_yuv420_16(second, flags=_all_flags(), **kw)
    assert [_lists(ctx.read_held(3), i) for i in range(3)] == held_w and sum(len(x) for x in held_w) > 0
    _fields_equal(faces, faces_w, 3)
    np.testing.assert_array_equal(out, out_w)


def test_rgb_nv12_and_p010_calls_interleaved_on_one_context(nets):
    """Calls of the three kinds on one context and stream: each gives what it gives alone."""
    ctx = nets("fp32")
    lay, depth, shift = P010
    nv = np.stack(_clip()[2:5])
    rgb = nr.to_rgb(nv)
    p010 = y16.widen(nv, depth, shift, 4)
    kinds = (lambda: ctx.process(rgb, flags=_all_flags()), lambda: ctx.process_nv12(nv, flags=_all_flags()),
             lambda: ctx.process_yuv420_16(p010, flags=_all_flags(), layout=lay, depth=depth, shift=shift))
    alone = []
    for call in kinds:
        ctx.hold_reset()
        out, faces, plates = call()
        alone.append((np.array(out), [_lists(faces, i) + _lists(plates, i) for i in range(3)]))
    ctx.hold_reset()
    for order in ((2, 0, 1), (1, 2, 0), (2, 2, 1)):
        for k in order:
            out, faces, plates = kinds[k]()
            assert [_lists(faces, i) + _lists(plates, i) for i in range(3)] == alone[k][1]
            np.testing.assert_array_equal(out, alone[k][0])
    np.testing.assert_array_equal(y16.D(alone[2][0], depth, shift), alone[1][0])
    assert alone[2][1] == alone[1][1] and sum(len(x) for x in alone[2][1]) > 0


# ---- 7. launch counts --------------------------------------------------------------------------------------

@pytest.mark.parametrize("gauss", [False, True])
def test_launch_counts_by_family_equal_the_8_bit_call(nets, gauss):
    """No extra pass: per timing family a *_yuv420_16 call launches what the *_yuv420 call on D(S) launches."""
    ctx = nets(**GAUSS) if gauss else nets("fp32")
    nv8 = np.stack(_clip()[1:4])
    xy, cnt = _arrays([[(10, 10, 60, 50), (40, 30, 200, 170)]] * 3)

    def counts(call):
        ctx.hold_reset()
        ctx.timing(True)
        ctx.timing_reset()
        call()
        ctx.sync()
        n = tuple(ctx.timing_read(f)[1] for f in range(7))
        ctx.timing(False)
        return n

    try:
        for lay, depth, shift in (P010, P12, ("nv21", 12, 4)):
            s8 = _cuda(yr.from_nv12(nv8, lay))
            s = _cuda16(y16.widen(yr.from_nv12(nv8, lay), depth, shift, 9))
            kw = dict(layout=lay, depth=depth, shift=shift)
            a = counts(lambda: ctx.process_yuv420(s8, flags=_all_flags(), layout=lay))
            b = counts(lambda: ctx.process_yuv420_16(s, flags=_all_flags(), **kw))
            assert a == b and a[1] > 0 and a[2] > 0, (lay, a, b)
            a = counts(lambda: ctx.mosaic_yuv420(s8, xy, cnt, level=8, layout=lay))
            b = counts(lambda: ctx.mosaic_yuv420_16(s, xy, cnt, level=8, **kw))
            assert a == b and a[1] > 0, (lay, a, b)
            a = counts(lambda: ctx.smooth_yuv420(s8, xy, cnt, level=8, cells=4, layout=lay))
            b = counts(lambda: ctx.smooth_yuv420_16(s, xy, cnt, level=8, cells=4, **kw))
            assert a == b and a[1] >= 2, (lay, a, b)
    finally:
        ctx.timing(False)
