"""The scaled smooth blur and the ellipse mask on NV12 frames on the GPU (include/vdmi.h at vd_nv12;
csrc/smooth.hip, csrc/mask.hip), bit-exact against tests/nv12_modes_ref.py: smooth_nv12 and
mosaic_nv12 with caller lists, and process_nv12 over the lists the context reports."""
import ctypes

import numpy as np
import pytest

import cells_ref as cr
import hold_ref as hr
import mask_ref as mr
import nv12_modes_ref as nm
import nv12_ref as nr
import rescue_ref as rr

pytestmark = pytest.mark.gpu

# csrc/smooth.hip
PART_PX = 16384         # a box of more pixels (per plane) is shared among workgroups
BEAT_CAP = 128          # beating boxes listed in LDS; more: the frame's list is walked per sample
F32_MAX = 4096          # larger cell sizes sum in 64 bits
# csrc/mask.hip
BR, BCAP = 16, 64       # luma rows per band; boxes a band lists in LDS

_NETS = {}


@pytest.fixture(scope="module")
def nets(gpu):
    """Contexts with seeded RetinaFace + YOLO weights by keyword arguments."""
    import vdmi
    from vdmi import weights

    def make(**kw):
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in _NETS:
            c = vdmi.Context(precision="fp32", max_batch=4, **kw)
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


@pytest.fixture
def masked(plain):
    """plain with a mask setting for the length of a test."""
    def set_mask(shape, g):
        plain.set_mask(shape, g)
        return plain
    yield set_mask
    plain.set_mask("rect", 0)
    plain.set_cells(0)


def _noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def _arrays(lists):
    cap = max(1, max(len(b) for b in lists))
    xy = np.zeros((len(lists), cap, 4), np.int32)
    for i, b in enumerate(lists):
        if b:
            xy[i, :len(b)] = np.asarray(b, np.int32)
    return xy, np.asarray([len(b) for b in lists], np.int32)


def _smooth_ref(f, lists, level, cells, height=None):
    return np.stack([nm.smooth(f[i], lists[i], level, cells, height) for i in range(len(f))])


def _dev(a):
    import torch
    return torch.from_numpy(a).cuda()


# ---- 1: smooth_nv12 against the reference ---------------------------------------------------------

def _box_sets(h, w):
    return {
        # odd-aligned corners, and a box clipped by two edges at each of two corners
        "odd": [(3, 5, 41, 37), (w - 31, h - 23, w - 2, h - 1), (-20, -9, 17, 13), (w - 9, h - 7, w + 30, h + 30)],
        # one edge each: left, right, top, bottom
        "edges": [(-10, 30, 21, 51), (w - 15, 31, w + 9, 55), (41, -12, 70, 9), (45, h - 11, 80, h + 30)],
        # 1 px wide, 1 px high, empty, inverted, fully outside (twice), and the N + 1 chroma grid of N = 2, level 1
        "thin": [(7, 9, 8, 40), (12, 51, 71, 52), (30, 20, 30, 50), (50, 40, 45, 60), (w + 5, 5, w + 40, 40),
                 (-50, -50, -10, -10), (1, 0, 5, 4)],
        # a small box inside a large one (strongest wins from either position), the frame itself
        "frame": [(11, 13, 50, 47), (0, 0, w, h)],
        # equal L, crossing: the overlap is the first one's; and a small box listed before the large one around it
        "tie": [(10, 10, 58, 40), (40, 20, 88, 50), (31, 65, 51, 81), (20, 60, 100, 90)],
    }


@pytest.mark.parametrize("level,cells", [(1, 2), (8, 4), (8, 16), (2, 64)])
@pytest.mark.parametrize("h,w", [(96, 128), (270, 480)])
def test_smooth_nv12_matches_the_reference(plain, h, w, level, cells):
    sets = _box_sets(h, w)
    names = sorted(sets)
    p, q = sets["tie"][:2]
    assert cr.box_level(p, level, cells) == cr.box_level(q, level, cells)
    if (level, cells) == (1, 2):
        assert nm.chroma_grid((1, 0, 5, 4), h, w, level, cells)[1][0] == cells + 1
    f = _noise(len(names), h, w, 3 * h + level)
    lists = [sets[k] for k in names]
    xy, cnt = _arrays(lists)
    want = _smooth_ref(f, lists, level, cells)
    assert all(not np.array_equal(want[i], f[i]) for i in range(len(names)))
    got = plain.smooth_nv12(_dev(f), xy, cnt, level=level, cells=cells)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---- 2: the parts split in both planes ------------------------------------------------------------

def test_smooth_nv12_large_box_is_split_in_both_planes(plain):
    h, w = 360, 640
    boxes = [(21, 31, 621, 331)]                       # 300 x 600: 180000 luma px, 45000 chroma samples
    (c, cc) = nm.rects(boxes[0], h, w)
    assert (c[2] - c[0]) * (c[3] - c[1]) > 2 * PART_PX and (cc[2] - cc[0]) * (cc[3] - cc[1]) > 2 * PART_PX
    f = _noise(1, h, w, 12)
    xy, cnt = _arrays([boxes])
    for level, cells in [(8, 16), (8, 64)]:            # 8 x 16 cells of 38 px; 32 x 63 cells of 10 px (5 in chroma)
        assert min(nm.chroma_grid(boxes[0], h, w, level, cells)[1]) >= 8
        got = plain.smooth_nv12(_dev(f), xy, cnt, level=level, cells=cells)
        np.testing.assert_array_equal(got.cpu().numpy(), _smooth_ref(f, [boxes], level, cells))


# ---- 3: more beating boxes than the LDS list holds ------------------------------------------------

def test_smooth_nv12_more_beating_boxes_than_the_lds_list(plain):
    """140 boxes from one corner with sides 2, 4, ..., 280 under (level 1, cells 2): L = 1 ... 140, all
    distinct, and the smallest is beaten by 139 others in both planes."""
    h, w = 96, 128
    boxes = [(9, 11, 9 + 2 * i, 11 + min(2 * i, 70)) for i in range(1, 141)]
    assert sorted(cr.box_level(b, 1, 2) for b in boxes) == list(range(1, 141)) and len(boxes) - 1 > BEAT_CAP
    order = np.random.default_rng(4).permutation(len(boxes))
    boxes = [boxes[i] for i in order]
    f = _noise(1, h, w, 13)
    xy, cnt = _arrays([boxes])
    got = plain.smooth_nv12(_dev(f), xy, cnt, level=1, cells=2)
    np.testing.assert_array_equal(got.cpu().numpy(), _smooth_ref(f, [boxes], 1, 2))


# ---- 4: wide sums ---------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [5000, 32768])
def test_smooth_nv12_levels_past_4096_give_the_rounded_mean(plain, level):
    """One cell per box: fc = 2500 (32-bit sums beside 64-bit luma sums) and fc = 16384 (64-bit in both)."""
    h, w = 96, 128
    assert level > F32_MAX and nm.chroma_level(32768) > F32_MAX > nm.chroma_level(5000)
    f = _noise(2, h, w, level)
    lists = [[(3, 5, 100, 90)], [(0, 0, w, h)]]
    xy, cnt = _arrays(lists)
    got = plain.smooth_nv12(_dev(f), xy, cnt, level=level, cells=4).cpu().numpy()
    np.testing.assert_array_equal(got, _smooth_ref(f, lists, level, 4))
    for i, boxes in enumerate(lists):
        c, cc = nm.rects(boxes[0], h, w)
        (Yi, UVi), (Yo, UVo) = nr.planes(f[i]), nr.planes(got[i])
        for src, dst, q in ((Yi[..., None], Yo[..., None], c), (UVi, UVo, cc)):
            reg = src[q[1]:q[3], q[0]:q[2]].astype(np.int64)
            n = reg.shape[0] * reg.shape[1]
            mean = ((16 * reg.reshape(n, -1).sum(0) + n // 2) // n + 8) >> 4
            assert (dst[q[1]:q[3], q[0]:q[2]] == mean).all()


# ---- 5: the byte path and a padded layout ---------------------------------------------------------

def _strided(packed, h, H, pitch, extra, offset, fill):
    """The packed frames [n, 3h/2, w] in a flat device buffer filled with `fill`: row pitch `pitch`, a
    luma plane padded to H rows, `extra` rows between frames, the first byte `offset` bytes into the
    buffer. -> (view [n, 3H/2, w], the buffer, a host array [n, rows + extra, pitch] of the buffer's frames)."""
    import torch
    n, _, w = packed.shape
    rows = H * 3 // 2
    fstride = (rows + extra) * pitch
    host = np.full((n, rows + extra, pitch), fill, np.uint8)
    host[:, :h, :w] = packed[:, :h]
    host[:, H:H + h // 2, :w] = packed[:, h:]
    buf = torch.full((offset + n * fstride,), fill, dtype=torch.uint8)
    buf[offset:] = torch.from_numpy(host.reshape(-1))
    buf = buf.cuda()
    return buf.as_strided((n, rows, w), (fstride, pitch, 1), offset), buf, host


@pytest.mark.parametrize("shape,g", [("rect", 0), ("ellipse", 20)])
@pytest.mark.parametrize("out_offset", [1, 2])           # rows congruent mod 16 (vectors behind a head) / not (bytes)
def test_smooth_nv12_byte_path_padded_layout_and_untouched_pad_bytes(masked, out_offset, shape, g):
    h, w, H = 96, 128, 104
    pitch = w + 6
    sets = _box_sets(h, w)
    lists = [sets["tie"] + sets["odd"], sets["thin"] + sets["edges"]]
    f = _noise(2, h, w, 77)
    xy, cnt = _arrays(lists)
    fn = lambda fr, bl: nm.smooth(fr, bl, 4, 6)
    want = np.stack([nm.shaped(f[i], lists[i], shape, g, fn) for i in range(2)])
    view, _, _ = _strided(f, h, H, pitch, 3, 1, 0xA5)
    out, obuf, _ = _strided(np.zeros_like(f), h, H, pitch, 3, out_offset, 0x5A)
    obuf[:] = 0x5A
    masked(shape, g).smooth_nv12(view, xy, cnt, level=4, cells=6, out=out, height=h)
    o = obuf.cpu().numpy()
    assert (o[:out_offset] == 0x5A).all()
    o = o[out_offset:].reshape(2, H * 3 // 2 + 3, pitch)
    np.testing.assert_array_equal(o[:, :h, :w], want[:, :h])
    np.testing.assert_array_equal(o[:, H:H + h // 2, :w], want[:, h:])
    o[:, :h, :w] = 0x5A
    o[:, H:H + h // 2, :w] = 0x5A
    assert (o == 0x5A).all()                             # pad bytes and the rows between the planes


# ---- 6: the ellipse -------------------------------------------------------------------------------

def _ellipse_lists(h, w):
    many = [(2 * i - 4, 17 + i % 7, 2 * i + 21, 24 + i % 9) for i in range(BCAP + 6)]     # all meet luma rows 16 .. 31
    assert all(b[1] < 2 * BR and b[3] > BR for b in many)
    return [
        # 4 x 4, 3 x 3, edge-clipped on all four sides, and b's corner inside a's ellipse
        [(40, 30, 44, 34), (51, 3, 54, 6), (-12, 40, 19, 71), (w - 17, 20, w + 11, 49), (60, -9, 91, 13),
         (70, h - 15, 99, h + 20), (20, 50, 70, 90), (45, 70, 90, 95)],
        [(-20000, 21, 20000, 51), (5, 60, 64, 93)],                                           # W > 32768: inside everywhere
        many,
    ]


@pytest.mark.parametrize("g", [0, 42])
@pytest.mark.parametrize("h,w", [(96, 128), (270, 480)])
@pytest.mark.parametrize("mode", ["mosaic", "smooth"])
def test_ellipse_on_both_planes(masked, mode, h, w, g):
    lists = _ellipse_lists(h, w)
    f = _noise(len(lists), h, w, h + g)
    xy, cnt = _arrays(lists)
    ctx = masked("ellipse", g)
    if mode == "mosaic":
        fn = lambda fr, bl: nr.mosaic(fr, bl, 4, 0)
        got = ctx.mosaic_nv12(_dev(f), xy, cnt, level=4)
    else:
        fn = lambda fr, bl: nm.smooth(fr, bl, 2, 4)
        got = ctx.smooth_nv12(_dev(f), xy, cnt, level=2, cells=4)
    got = got.cpu().numpy()
    for i in range(len(lists)):
        want = nm.shaped(f[i], lists[i], "ellipse", g, fn)
        np.testing.assert_array_equal(got[i], want, err_msg=f"frame {i}")
        assert not np.array_equal(want, fn(f[i], mr.grow_list(lists[i], g))) and not np.array_equal(want, f[i])


# ---- 8: host frames -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["mosaic", "smooth"])
def test_host_frames_equal_device_frames(masked, mode):
    h, w = 96, 128
    lists = _ellipse_lists(h, w)[:2] + [_box_sets(h, w)["tie"]]
    f = _noise(len(lists), h, w, 8)
    xy, cnt = _arrays(lists)
    ctx = masked("ellipse", 42)
    if mode == "mosaic":
        fn = lambda fr, bl: nr.mosaic(fr, bl, 4, 0)
        dev, host = ctx.mosaic_nv12(_dev(f), xy, cnt, level=4), ctx.mosaic_nv12(f, xy, cnt, level=4)
    else:
        fn = lambda fr, bl: nm.smooth(fr, bl, 2, 4)
        dev, host = ctx.smooth_nv12(_dev(f), xy, cnt, level=2, cells=4), ctx.smooth_nv12(f, xy, cnt, level=2, cells=4)
    np.testing.assert_array_equal(host, dev.cpu().numpy())
    np.testing.assert_array_equal(host, np.stack([nm.shaped(f[i], lists[i], "ellipse", 42, fn) for i in range(len(lists))]))
    # padded host surfaces: only [0, w) of the planes' rows comes back
    H = 104
    big = np.full((len(lists), H * 3 // 2, w), 0xA5, np.uint8)
    big[:, :h] = f[:, :h]
    big[:, H:H + h // 2] = f[:, h:]
    obig = np.full_like(big, 0x5A)
    call = ctx.mosaic_nv12 if mode == "mosaic" else ctx.smooth_nv12
    kw = dict(level=4) if mode == "mosaic" else dict(level=2, cells=4)
    call(big, xy, cnt, out=obig, height=h, **kw)
    np.testing.assert_array_equal(obig[:, :h], host[:, :h])
    np.testing.assert_array_equal(obig[:, H:H + h // 2], host[:, h:])
    assert (obig[:, h:H] == 0x5A).all() and (obig[:, H + h // 2:] == 0x5A).all()


# ---- 7: process_nv12 end to end -------------------------------------------------------------------

GAUSS = dict(blur="gaussian", cells=8, mask="ellipse", mask_grow=42, hold=2)


def _scene(n, h, w, seed):
    from vdmi import synth
    return np.stack([np.repeat(np.repeat(synth.frame(h // 2, w // 2, i, seed=seed), 2, 0), 2, 1) for i in range(n)])


def _clip(seed=5):
    a, b, c = (nr.from_rgb(_scene(3, 360, 640, seed))[i] for i in range(3))
    return [a, a, b, b, c, a]


def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _all_flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _modes_ref(frame, bl, level=8, cells=8, g=42):
    return nm.shaped(frame, bl, "ellipse", g, lambda fr, b: nm.smooth(fr, b, level, cells))


def test_process_nv12_smooth_ellipse_over_the_reported_lists(nets):
    """hold=2 over [A, A, B, B, C, A] in calls of 4 + 2, device frames: every output frame is the
    reference over faces ++ plates ++ held, and the detections are a pixelate / rect context's."""
    frames = _clip()
    ctx, base = nets(**GAUSS), nets(hold=2)
    lo, held_total, own_total = 0, 0, 0
    for n in (4, 2):
        batch = np.stack(frames[lo:lo + n])
        out, faces, plates = ctx.process_nv12(_dev(batch), flags=_all_flags())
        ff, pp, held = ctx.read_boxes(0, n), ctx.read_boxes(1, n), ctx.read_held(n)
        _, faces0, plates0 = base.process_nv12(_dev(batch), flags=_all_flags())
        held0 = base.read_held(n)
        out = out.cpu().numpy()
        for i in range(n):
            assert _lists(faces, i) == _lists(ff, i) == _lists(faces0, i)
            assert _lists(plates, i) == _lists(pp, i) == _lists(plates0, i)
            assert _lists(held, i) == _lists(held0, i)
            bl = _lists(ff, i) + _lists(pp, i) + _lists(held, i)
            own_total += len(bl) - int(held.count[i])
            held_total += int(held.count[i])
            np.testing.assert_array_equal(out[i], _modes_ref(batch[i], bl), err_msg=f"frame {lo + i}")
            assert not np.array_equal(out[i], batch[i])
        lo += n
    assert held_total > 0 and own_total > 0


def test_process_nv12_smooth_ellipse_with_rescue(nets):
    """The same with rescue on (host frames): every output frame is the reference over B_t = E_t ++ H_t."""
    K, S, H, W = 2, 3, 360, 640
    frames = _clip()
    ctx = nets(rescue=0.2, rescue_span=S, **GAUSS)
    base = nets(hold=K, rescue=0.2, rescue_span=S)
    outs, D, Wk, R = [], [], [], []
    lo = 0
    for n in (4, 2):
        batch = np.stack(frames[lo:lo + n])
        out, faces, plates = ctx.process_nv12(batch, flags=_all_flags())
        weak = [ctx.read_rescue(net, n, "weak") for net in (0, 1)]
        resc = [ctx.read_rescue(net, n, "rescued") for net in (0, 1)]
        _, faces0, plates0 = base.process_nv12(batch, flags=_all_flags())
        resc0 = [base.read_rescue(net, n, "rescued") for net in (0, 1)]
        for i in range(n):
            assert _lists(faces, i) == _lists(faces0, i) and _lists(plates, i) == _lists(plates0, i)
            assert [_lists(r, i) for r in resc] == [_lists(r, i) for r in resc0]
            outs.append(out[i])
            D.append(_lists(faces, i) + _lists(plates, i))
            Wk.append(_lists(weak[0], i) + _lists(weak[1], i))
            R.append(_lists(resc[0], i) + _lists(resc[1], i))
        lo += n
    E, _, Rr, _, _ = rr.rescue_lists(D, Wk, H, W, K, S, 30)
    assert R == Rr and sum(len(r) for r in R) > 0
    B, _, _, _ = hr.hold_lists(E, H, W, K, 30)
    for t, fr in enumerate(frames):
        np.testing.assert_array_equal(outs[t], _modes_ref(fr, B[t]), err_msg=f"frame {t}")


# ---- 9: RGB and NV12 calls interleaved ------------------------------------------------------------

def test_rgb_and_nv12_calls_advance_one_history(nets):
    frames = _clip()
    ctx = nets(**GAUSS)
    first, second = np.stack(frames[:3]), np.stack(frames[3:])
    ctx.process_nv12(first, flags=_all_flags())
    out_w, _, _ = ctx.process_nv12(second, flags=_all_flags())
    want = ctx.read_held(3)
    want_lists = [_lists(want, i) for i in range(3)]
    ctx.hold_reset()
    ctx.process(nr.to_rgb(first), flags=_all_flags())
    out, faces, plates = ctx.process_nv12(second, flags=_all_flags())
    held = ctx.read_held(3)
    assert [_lists(held, i) for i in range(3)] == want_lists and sum(len(x) for x in want_lists) > 0
    np.testing.assert_array_equal(out, out_w)
    for i in range(3):
        bl = _lists(faces, i) + _lists(plates, i) + want_lists[i]
        np.testing.assert_array_equal(out[i], _modes_ref(second[i], bl))


# ---- 10: refusals ---------------------------------------------------------------------------------

def test_refusals_leave_the_stream_untouched(nets):
    """The two settings still without an NV12 pass answer VD_ERR_STATE, the smooth blur's limits
    VD_ERR_ARG; between two calls of a holding stream none of them changes what the second call gives."""
    from vdmi import _lib
    frames = _clip()
    first, second = np.stack(frames[:2]), np.stack(frames[2:5])
    ctx = nets(**GAUSS)
    ctx.process_nv12(first, flags=_all_flags())
    out_w, faces_w, plates_w = ctx.process_nv12(second, flags=_all_flags())
    held_w = ctx.read_held(3)
    ctx.hold_reset()
    ctx.process_nv12(first, flags=_all_flags())

    # the fixed-kernel Gaussian: cells off in a Gaussian context
    ctx.set_cells(0)
    xy, cnt = _arrays([[(10, 10, 60, 50)]] * 3)
    for call in (lambda: ctx.process_nv12(second, flags=_all_flags()), lambda: ctx.mosaic_nv12(second, xy, cnt, level=8)):
        with pytest.raises(_lib.VdError, match="cells") as e:
            call()
        assert e.value.code == _lib.VD_ERR_STATE
    ctx.set_cells(8)

    # the smooth blur's limits, through the raw entry point (nothing is read before the refusal)
    buf, obuf = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    hb = _lib.HostBoxes(1, 1)
    s = hb.struct()

    def smooth(h, w, level, cells=8):
        d = [_lib.vd_nv12(b.ctypes.data, w, h * w, h * w * 3 // 2, 1, 0) for b in (buf, obuf)]
        return ctx._lib.vd_smooth_nv12(ctx._h, ctypes.byref(d[0]), ctypes.byref(d[1]), 1, h, w, _lib.VD_HOST,
                                       ctypes.byref(s), level, cells)

    for kw in (dict(h=32770, w=2, level=8), dict(h=2, w=32770, level=8), dict(h=4, w=4, level=32769),
               dict(h=4, w=4, level=0), dict(h=4, w=4, level=8, cells=1), dict(h=4, w=4, level=8, cells=65),
               dict(h=5, w=4, level=8), dict(h=4, w=5, level=8)):
        assert smooth(**kw) == _lib.VD_ERR_ARG, kw
    with pytest.raises(_lib.VdError):
        ctx.smooth_nv12(second, xy, cnt, level=32769)
    with pytest.raises(ValueError):
        ctx.smooth_nv12(second, xy, cnt, cells=1)

    out, faces, plates = ctx.process_nv12(second, flags=_all_flags())
    held = ctx.read_held(3)
    for i in range(3):
        assert _lists(faces, i) == _lists(faces_w, i) and _lists(plates, i) == _lists(plates_w, i)
        assert _lists(held, i) == _lists(held_w, i)
    np.testing.assert_array_equal(out, out_w)
    assert int(held_w.count.sum()) > 0 and not np.array_equal(out, second)


def test_tiling_is_still_refused_on_nv12_frames(nets):
    from vdmi import _lib
    f = np.stack(_clip()[:1])
    ctx = nets(blur="gaussian", cells=8)
    want, _, _ = ctx.process_nv12(f, flags=_all_flags())
    ctx.set_tiles((2, 2), 20)
    try:
        with pytest.raises(_lib.VdError, match="tile") as e:
            ctx.process_nv12(f, flags=_all_flags())
        assert e.value.code == _lib.VD_ERR_STATE
    finally:
        ctx.set_tiles((1, 1), 20)
    out, _, _ = ctx.process_nv12(f, flags=_all_flags())
    np.testing.assert_array_equal(out, want)
