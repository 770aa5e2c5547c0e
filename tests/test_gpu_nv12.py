"""NV12 frames on the GPU (include/vdmi.h at vd_nv12; csrc/pre.hip, csrc/nv12.hip), exact against
tests/nv12_ref.py: the NV12 letterbox equals the RGB letterbox of the converted frames, the detection
lists of process_nv12 equal those of process on the converted frames, and both planes of the output
equal the plane-wise reference mosaic of the lists the context reports."""
import numpy as np
import pytest

import hold_ref as hr
import mask_ref as mr
import nv12_ref as nr
import rescue_ref as rr

pytestmark = pytest.mark.gpu

# csrc/nv12.hip
NV12_ROWS = 16          # luma rows per band (8 chroma rows)
NV12_LDS_BOXES = 256    # boxes of a frame a workgroup clips into LDS; fuller frames walk the lists in global memory
NV12_BAND_BOXES = 32    # boxes in a band's list; fuller bands walk per sample
NV12_CELLS = 4096       # cell colours per band and plane in LDS; more: per-sample walk

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
    """A weight-less context: mosaic_nv12 needs no network."""
    import vdmi
    c = vdmi.Context(precision="fp32", max_batch=4)
    yield c
    c.close()


def _noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def _padded_view(packed, h, H, pitch, extra_rows, device="cuda:0"):
    """The packed frames [n, 3h/2, w] as a torch view with a row pitch > w, a luma plane padded to H
    rows and a padded frame stride; pad bytes are 0xA5. -> (view [n, 3H/2, w], the whole buffer)."""
    import torch
    n, _, w = packed.shape
    big = torch.full((n, H * 3 // 2 + extra_rows, pitch), 0xA5, dtype=torch.uint8)
    big[:, :h, :w] = torch.from_numpy(packed[:, :h])
    big[:, H:H + h // 2, :w] = torch.from_numpy(packed[:, h:])
    big = big.to(device)
    return big[:, :H * 3 // 2, :w], big


# ---- letterbox -------------------------------------------------------------------------------------

SIZES = [(1080, 1920), (720, 1280), (640, 640), (480, 640), (334, 518), (48, 64), (2, 2)]
COLOURS = [("bt709", "limited"), ("bt601", "limited"), ("bt709", "full"), ("bt601", "full")]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("h,w", SIZES)
def test_letterbox_equals_the_rgb_letterbox_of_the_converted_frames(nets, h, w, precision):
    import torch
    m, r = COLOURS[SIZES.index((h, w)) % 4]
    f = _noise(2, h, w, h + w)
    ctx = nets(precision)
    want = ctx.letterbox(nr.to_rgb(f, m, r))
    assert np.abs(want).max() > 0
    np.testing.assert_array_equal(ctx.letterbox_nv12(torch.from_numpy(f).cuda(), matrix=m, range=r), want)


def test_letterbox_fp16_f32_canvas_host_frames_and_a_padded_layout(nets, gpu):
    import vdmi
    from vdmi import weights
    h, w = 480, 640
    f = _noise(2, h, w, 11)
    want_rgb = nr.to_rgb(f, "bt601", "limited")
    ctx = nets("fp16")
    want = ctx.letterbox(want_rgb)
    np.testing.assert_array_equal(ctx.letterbox_nv12(f, matrix="bt601"), want)            # host frames, staged as NV12
    # pitch > w, a luma plane padded to 496 rows, a padded frame stride; device and host
    view, big = _padded_view(f, h, 496, 704, 5)
    np.testing.assert_array_equal(ctx.letterbox_nv12(view, matrix="bt601", height=h), want)
    np.testing.assert_array_equal(ctx.letterbox_nv12(view.cpu(), matrix="bt601", height=h), want)
    # the fp32 plan without the fused stem keeps an f32 NHWC canvas: the per-pixel NV12 kernel
    c32 = vdmi.Context(precision="fp32", max_batch=2, options={"stem_pool": 0})
    try:
        c32.load_weights(0, weights.retinaface_state_dict(0))
        for hh, ww in ((480, 640), (334, 518), (640, 1280)):     # linear, linear, exact 2x area
            g = _noise(2, hh, ww, hh)
            np.testing.assert_array_equal(c32.letterbox_nv12(g), c32.letterbox(nr.to_rgb(g)))
    finally:
        c32.close()


# ---- detection -------------------------------------------------------------------------------------

def _scene(n, h, w, seed):
    """n RGB frames of synthetic scenes on which the seeded weights fire, pixels doubled (so the 2 x 2
    chroma pooling of the test-only inverse loses little)."""
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
def test_process_nv12_lists_equal_process_on_the_converted_frames(nets, h, w, seed, precision):
    from vdmi import _lib
    ctx = nets(precision)
    F, P = _lib.VD_PROC_FACES, _lib.VD_PROC_PLATES
    seen = {F: 0, P: 0}
    for m in ("bt709", "bt601"):
        f = nr.from_rgb(_scene(2, h, w, seed), m, "limited")
        rgb = nr.to_rgb(f, m, "limited")
        for flags in (F, P, F | P):                      # F | P: the paired letterbox launch
            _, faces, plates = ctx.process_nv12(f, flags=flags, matrix=m)
            rb = [ctx.read_boxes(net, 2) for net, bit in ((0, F), (1, P)) if flags & bit]
            _, faces0, plates0 = ctx.process(rgb, flags=flags)
            rb0 = [ctx.read_boxes(net, 2) for net, bit in ((0, F), (1, P)) if flags & bit]
            if flags & F:
                seen[F] += _fields_equal(faces, faces0, 2)
            if flags & P:
                seen[P] += _fields_equal(plates, plates0, 2)
            for x, y in zip(rb, rb0):
                _fields_equal(x, y, 2)
    assert seen[F] > 0 and seen[P] > 0, seen              # the compared lists are not empty


# ---- mosaic of caller lists --------------------------------------------------------------------------

def _box_sets(h, w):
    return {
        "odd": [(3, 5, 41, 37), (w - 31, h - 23, w - 2, h - 1)],
        "chain": [(10, 10, 60, 50), (40, 30, 90, 70), (55, 5, 75, 64)],
        "off_and_empty": [(-20, -9, 17, 13), (w - 9, h - 7, w + 30, h + 30), (w + 5, 5, w + 40, 40), (30, 20, 30, 50),
                          (50, 40, 45, 60), (-50, -50, -10, -10), (20, 20, 44, 41)],
        "one_px": [(7, 9, 8, 10), (w - 1, h - 1, w, h), (0, 0, 1, 1), (12, 3, 13, 30), (2, 40, 70, 41)],
        "frame": [(0, 0, w, h), (11, 13, 50, 47)],
    }


def _mosaic_ref(f, lists, level, cells, height=None):
    return np.stack([nr.mosaic(f[i], lists[i], level, cells, height) for i in range(len(f))])


def _arrays(lists):
    cap = max(1, max(len(b) for b in lists))
    xy = np.zeros((len(lists), cap, 4), np.int32)
    for i, b in enumerate(lists):
        if b:
            xy[i, :len(b)] = np.asarray(b, np.int32)
    return xy, np.asarray([len(b) for b in lists], np.int32)


@pytest.mark.parametrize("level,cells", [(1, 0), (2, 0), (8, 0), (9, 0), (8, 4)])
@pytest.mark.parametrize("h,w", [(96, 128), (270, 480)])
def test_mosaic_nv12_matches_the_plane_wise_reference(plain, h, w, level, cells):
    import torch
    sets = _box_sets(h, w)
    names = sorted(sets)
    f = _noise(len(names), h, w, 3 * h + level)
    lists = [sets[k] for k in names]
    xy, cnt = _arrays(lists)
    plain.set_cells(cells)
    try:
        want = _mosaic_ref(f, lists, level, cells)
        got = plain.mosaic_nv12(torch.from_numpy(f).cuda(), xy, cnt, level=level)            # device, 16-B vectors
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(plain.mosaic_nv12(f, xy, cnt, level=level), want)       # host frames
    finally:
        plain.set_cells(0)


def test_mosaic_nv12_byte_path_padded_layout_and_untouched_pad_bytes(plain):
    """An unaligned pitch (the byte path) with a padded luma height and frame stride: both planes match
    the reference, and no byte outside [0, w) of the planes' rows is written (the output buffer keeps its
    fill there). Then a width that is no multiple of 16 on aligned rows: vectors plus a byte tail."""
    import torch
    h, w, H = 96, 128, 104
    sets = _box_sets(h, w)
    lists = [sets["chain"] + sets["odd"], sets["off_and_empty"]]
    f = _noise(2, h, w, 77)
    xy, cnt = _arrays(lists)
    want = _mosaic_ref(f, lists, 8, 0)
    for pitch in (131, 144):
        view, _ = _padded_view(f, h, H, pitch, 3)
        obig = torch.full((2, H * 3 // 2 + 3, pitch), 0x5A, dtype=torch.uint8, device="cuda:0")
        out = obig[:, :H * 3 // 2, :w]
        plain.mosaic_nv12(view, xy, cnt, level=8, out=out, height=h)
        o = obig.cpu().numpy()
        np.testing.assert_array_equal(o[:, :h, :w], want[:, :h])
        np.testing.assert_array_equal(o[:, H:H + h // 2, :w], want[:, h:])
        o[:, :h, :w] = 0x5A
        o[:, H:H + h // 2, :w] = 0x5A
        assert (o == 0x5A).all()
    g = _noise(2, 50, 90, 5)
    lists = [[(3, 3, 88, 47), (60, 10, 90, 50)], [(-4, 20, 33, 49)]]
    xy, cnt = _arrays(lists)
    got = plain.mosaic_nv12(torch.from_numpy(g).cuda(), xy, cnt, level=4)
    np.testing.assert_array_equal(got.cpu().numpy(), _mosaic_ref(g, lists, 4, 0))


def test_mosaic_nv12_past_every_capacity(plain):
    """Lists that cross NV12_BAND_BOXES (a band more than 32 boxes meet), NV12_CELLS (level 1: a band's
    slices hold more than 4096 cells) and NV12_LDS_BOXES (300 boxes in a frame), next to frames below
    each; device lists."""
    import torch
    from vdmi.context import DeviceBoxes
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
    cases = [(rand(NV12_BAND_BOXES - 2, 40), 8), (band[:NV12_BAND_BOXES], 2), (band, 2), (nested[:8], 2), (nested, 2),
             (rand(NV12_LDS_BOXES, 30), 3), (rand(NV12_LDS_BOXES + 44, 30), 3)]
    f = _noise(1, h, w, 21)
    for boxes, level in cases:
        xy, cnt = _arrays([boxes])
        db = DeviceBoxes(1, xy.shape[1], "cuda:0")
        db.count.copy_(torch.from_numpy(cnt))
        db.xyxy.copy_(torch.from_numpy(xy))
        torch.cuda.synchronize()
        dev = torch.from_numpy(f).cuda()
        got = plain.mosaic_nv12(dev, db, level=level)
        plain.sync()                                     # every pointer on the device: the call is asynchronous
        np.testing.assert_array_equal(got.cpu().numpy(), _mosaic_ref(f, [boxes], level, 0), err_msg=f"{len(boxes)} boxes")


def test_mosaic_nv12_mask_growth_and_host_capacity(plain):
    from vdmi import VdCapacityError
    h, w = 96, 128
    f = _noise(1, h, w, 31)
    boxes = [(20, 20, 50, 60), (70, 10, 120, 40), (100, 80, 140, 120)]
    xy, cnt = _arrays([boxes])
    plain.set_mask("rect", 20)
    plain.set_cells(8)
    try:
        got = plain.mosaic_nv12(f, xy, cnt, level=4)
        np.testing.assert_array_equal(got, _mosaic_ref(f, [mr.grow_list(boxes, 20)], 4, 8))
    finally:
        plain.set_mask("rect", 0)
        plain.set_cells(0)
    with pytest.raises(VdCapacityError):
        plain.mosaic_nv12(f, xy, np.asarray([9], np.int32), level=4)


# ---- process with the output pass ---------------------------------------------------------------------

def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _all_flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _clip(seed=5):
    a, b, c = (nr.from_rgb(_scene(3, 360, 640, seed))[i] for i in range(3))
    return [a, a, b, b, c, a]


def test_process_nv12_output_is_the_reference_over_the_reported_lists(nets):
    """hold=2 over [A, A, B, B, C, A] in calls of 4 + 2, device frames: every output frame is the
    reference over D_t ++ read_held."""
    import torch
    frames = _clip()
    ctx = nets("fp32", hold=2)
    lo, held_total, own_total = 0, 0, 0
    for n in (4, 2):
        batch = np.stack(frames[lo:lo + n])
        out, faces, plates = ctx.process_nv12(torch.from_numpy(batch).cuda(), flags=_all_flags())
        ff, pp, held = ctx.read_boxes(0, n), ctx.read_boxes(1, n), ctx.read_held(n)
        out = out.cpu().numpy()
        for i in range(n):
            assert _lists(faces, i) == _lists(ff, i) and _lists(plates, i) == _lists(pp, i)
            bl = _lists(ff, i) + _lists(pp, i) + _lists(held, i)
            own_total += len(bl) - int(held.count[i])
            held_total += int(held.count[i])
            np.testing.assert_array_equal(out[i], nr.mosaic(batch[i], bl, 8), err_msg=f"frame {lo + i}")
        lo += n
    assert held_total > 0 and own_total > 0


def test_process_nv12_mask_growth_and_cells(nets):
    frames = np.stack(_clip()[1:4])
    ctx = nets("fp32", mask_grow=20, cells=8)
    out, faces, plates = ctx.process_nv12(frames, flags=_all_flags())                    # host frames
    total = 0
    for i in range(3):
        bl = mr.grow_list(_lists(faces, i) + _lists(plates, i), 20)
        total += len(bl)
        np.testing.assert_array_equal(out[i], nr.mosaic(frames[i], bl, 8, 8), err_msg=f"frame {i}")
    assert total > 0 and not np.array_equal(out, frames)


def test_process_nv12_with_rescue(nets):
    """hold=2, rescue=0.2, span=3 over the clip in calls of 4 + 2: read_rescue equals the reference over
    the GPU's D and W lists, and every output frame is the reference over B_t = E_t ++ H_t."""
    K, S, H, W = 2, 3, 360, 640
    frames = _clip()
    ctx = nets("fp32", hold=K, rescue=0.2, rescue_span=S)
    outs, D, Wk, R = [], [], [], []
    lo = 0
    for n in (4, 2):
        batch = np.stack(frames[lo:lo + n])
        out, faces, plates = ctx.process_nv12(batch, flags=_all_flags())
        weak = [ctx.read_rescue(net, n, "weak") for net in (0, 1)]
        resc = [ctx.read_rescue(net, n, "rescued") for net in (0, 1)]
        for i in range(n):
            outs.append(out[i])
            D.append(_lists(faces, i) + _lists(plates, i))
            Wk.append(_lists(weak[0], i) + _lists(weak[1], i))
            R.append(_lists(resc[0], i) + _lists(resc[1], i))
        lo += n
    E, _, Rr, _, _ = rr.rescue_lists(D, Wk, H, W, K, S, 30)
    assert R == Rr and sum(len(r) for r in R) > 0
    B, _, _, _ = hr.hold_lists(E, H, W, K, 30)
    for t, fr in enumerate(frames):
        np.testing.assert_array_equal(outs[t], nr.mosaic(fr, B[t], 8), err_msg=f"frame {t}")


def test_rgb_and_nv12_calls_share_one_stream(nets):
    """An RGB call followed by an NV12 call of the same (h, w): the held boxes are those of the
    uninterrupted stream."""
    frames = _clip()
    ctx = nets("fp32", hold=2)
    first, second = np.stack(frames[:3]), np.stack(frames[3:])
    ctx.process_nv12(first, flags=_all_flags())
    ctx.process_nv12(second, flags=_all_flags())
    want = ctx.read_held(3)
    want_lists = [_lists(want, i) for i in range(3)]
    ctx.hold_reset()
    ctx.process(nr.to_rgb(first), flags=_all_flags())
    out, faces, plates = ctx.process_nv12(second, flags=_all_flags())
    held = ctx.read_held(3)
    assert [_lists(held, i) for i in range(3)] == want_lists and sum(len(x) for x in want_lists) > 0
    for i in range(3):
        bl = _lists(faces, i) + _lists(plates, i) + want_lists[i]
        np.testing.assert_array_equal(out[i], nr.mosaic(second[i], bl, 8))


# ---- refused calls -------------------------------------------------------------------------------------

def test_err_arg_cases_leave_the_stream_untouched(nets):
    """Every VD_ERR_ARG case of vd_process_nv12, between two calls of a holding stream: the second call's
    lists, held boxes and pixels equal those of a stream that never saw the refusals."""
    import ctypes
    import torch
    from vdmi import _lib
    frames = _clip()
    first, second = np.stack(frames[:2]), np.stack(frames[2:5])
    ctx = nets("fp32", hold=2)
    ctx.process_nv12(first, flags=_all_flags())
    out_w, faces_w, plates_w = ctx.process_nv12(second, flags=_all_flags())
    held_w = ctx.read_held(3)
    ctx.hold_reset()
    ctx.process_nv12(first, flags=_all_flags())

    h, w = 360, 640
    dev = torch.from_numpy(second).cuda()
    dout = torch.empty_like(dev)
    base, obase = dev.data_ptr(), dout.data_ptr()
    good = dict(pitch=w, uv_offset=h * w, frame_stride=h * w * 3 // 2, matrix=1, range=0)

    def call(n=3, hh=h, ww=w, out=True, obase=obase, **kw):
        d = dict(good, **kw)
        i = _lib.vd_nv12(base, d["pitch"], d["uv_offset"], d["frame_stride"], d["matrix"], d["range"])
        o = _lib.vd_nv12(obase, w, h * w, h * w * 3 // 2, 0, 0)
        return ctx._lib.vd_process_nv12(ctx._h, ctypes.byref(i), ctypes.byref(o) if out else None, n, hh, ww,
                                        _lib.VD_DEVICE, _all_flags(), None, None)

    bad = [dict(hh=359), dict(ww=639), dict(hh=0), dict(ww=-640), dict(n=0), dict(n=5), dict(pitch=w - 2),
           dict(uv_offset=h * w - 1), dict(frame_stride=h * w * 3 // 2 - 1), dict(matrix=2), dict(range=7),
           dict(out=False), dict(obase=base), dict(obase=base + 3 * h * w * 3 // 2 - 16),
           dict(obase=base - 3 * h * w * 3 // 2 + 16)]
    for kw in bad:
        assert call(**kw) == _lib.VD_ERR_ARG, kw
    with pytest.raises(ValueError):
        ctx.process_nv12(second, matrix="bt2020")
    with pytest.raises(ValueError):
        ctx.process_nv12(second[:, :-1])

    out, faces, plates = ctx.process_nv12(second, flags=_all_flags())
    held = ctx.read_held(3)
    for i in range(3):
        assert _lists(faces, i) == _lists(faces_w, i) and _lists(plates, i) == _lists(plates_w, i)
        assert _lists(held, i) == _lists(held_w, i)
    np.testing.assert_array_equal(out, out_w)
    assert int(held_w.count.sum()) > 0
