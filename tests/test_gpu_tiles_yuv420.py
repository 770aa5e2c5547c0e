"""Tiled detection on 4:2:0 surfaces on the GPU (include/vdmi.h at vd_tiles_surfaces; csrc/pre.hip's
rectangle sources). Nothing new is computed, so everything is checked against what exists: the tile
canvases against the RGB tile letterbox of the converted frames, the lists against the RGB tiled call's
in the same context, the output surfaces against the stand-alone surface blur of those lists. Every
comparison is bit equality."""
import ctypes

import numpy as np
import pytest

import nv12_ref as nr
import yuv420_16_ref as y16
import yuv420_ref as yr

pytestmark = pytest.mark.gpu

H, W = 360, 640
# tests/test_gpu_plate_tiles.py's contexts (dense face weights, plate weights loaded on first use)
NET = dict(precision="fp32", max_batch=10, wkind="dense", plate_conf=0.5)
T22 = dict(tiles=(2, 2), tile_overlap=20)
SURF = dict(tile_nets="both", tile_surfaces=True)
COLOURS = [("bt709", "limited"), ("bt601", "full")]
# (layout, depth, shift): P010, yuv420p10le, and a 12-bit layout with V first and the samples in the middle of the word
WORDS = [("nv12", 10, 6), ("i420", 10, 0), ("yv12", 12, 2)]
# every parity of a tile origin and odd and even extents occur (tests/test_tiles_surfaces_abi.py); 38 x 54: iw < 46
LB_SHAPES = [(174, 212, (2, 2), 20), (174, 212, (1, 3), 0), (174, 212, (3, 1), 50), (38, 54, (4, 4), 50)]


def _ctx(factory, **kw):
    from vdmi import weights
    ctx = factory(**{**NET, **kw})
    if not getattr(ctx, "_plates_loaded", False):
        ctx.load_weights(1, weights.yolov8n_state_dict(0))
        ctx._plates_loaded = True
    ctx.hold_reset()
    return ctx


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()                                # the context reads it on its own stream
    return t


def _cuda16(a):
    return _cuda(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16))


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def _nv12_view(nv, h, w):
    """Packed NV12 frames as a device view with a luma pitch > w, the luma plane padded by 4 rows
    (chroma offset > pitch * h) and frames further apart than their rows; -> (view, height)."""
    import torch
    n, hp = len(nv), h + 4
    big = torch.full((n, hp * 3 // 2 + 5, w + 20), 0xA5, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(nv).cuda()
    big[:, :h, :w] = src[:, :h]
    big[:, hp:hp + h // 2, :w] = src[:, h:]
    torch.cuda.synchronize()
    return big[:, :hp * 3 // 2, :w], h


def _surf8(nv, lay, h, w):
    """The samples of packed NV12 frames in layout `lay` on the device: luma pitch w + 20, a chroma pitch of
    its own, the luma plane padded by 6 rows, 77 bytes between frames, the first byte misaligned."""
    import vdmi
    step = 2 if lay in ("nv12", "nv21") else 1
    buf, fd = yr.padded(yr.from_nv12(nv, lay), lay, w + 20, (w // 2 + 9) * step, h + 6, lay in ("yv12", "nv21"), 77, base_pad=3)
    dev = _cuda(buf)
    return vdmi.Yuv420(dev[fd["base"]:], h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"],
                       fd["chroma_step"], fd["frame_stride"])


def _surf16(nv, lay, depth, shift, h, w, seed):
    """... as 16-bit words whose 8-bit picture is those samples: random low value bits, random unused bits."""
    import vdmi
    s = y16.widen(yr.from_nv12(nv, lay), depth, shift, seed)
    assert np.array_equal(y16.D(s, depth, shift), yr.from_nv12(nv, lay)) and (s != y16.values(s, depth, shift) << shift).any()
    step = 2 if lay in y16.INTERLEAVED else 1
    buf, fd = y16.padded(s, lay, w + 21, (w // 2 + 9) * step, h + 6, lay in ("yv12", "nv21"), 13, base_pad_w=3)
    dev = _cuda16(buf)
    return vdmi.Yuv420_16(dev[fd["base"] // 2:], h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"],
                          fd["chroma_step"], fd["frame_stride"], depth=depth, shift=shift)


def _kinds(nv, h, w, seed):
    """(name, tiles hook, plain hook) of every kind of surface holding the samples of `nv`: NV12 through the
    NV12 hook, the four 8-bit layouts through the yuv420 hook, three 16-bit layouts."""
    out = []
    view, height = _nv12_view(nv, h, w)
    out.append(("nv12 hook", lambda c, m, r: c.letterbox_tiles_nv12(view, matrix=m, range=r, height=height),
                lambda c, m, r: c.letterbox_nv12(view, matrix=m, range=r, height=height)))
    for lay in yr.LAYOUTS:
        s = _surf8(nv, lay, h, w)
        out.append((lay, lambda c, m, r, s=s: c.letterbox_tiles_yuv420(s, matrix=m, range=r),
                    lambda c, m, r, s=s: c.letterbox_yuv420(s, matrix=m, range=r)))
    for k, (lay, depth, shift) in enumerate(WORDS):
        s = _surf16(nv, lay, depth, shift, h, w, seed + k)
        out.append((f"{lay}/{depth}/{shift}", lambda c, m, r, s=s: c.letterbox_tiles_yuv420_16(s, matrix=m, range=r),
                    lambda c, m, r, s=s: c.letterbox_yuv420_16(s, matrix=m, range=r)))
    return out


# ---- 1. the tile canvases ------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,wkind,h,w,tiles,ov",
                         [(p, "default") + s for p in ("fp32", "bf16") for s in LB_SHAPES] +
                         [(p, "mnet") + LB_SHAPES[0] for p in ("fp32", "bf16")])
def test_tile_canvases_equal_the_rgb_tile_canvases(face_ctx_factory, precision, wkind, h, w, tiles, ov):
    """letterbox_tiles_<kind>(surfaces) == letterbox_tiles(<kind>_to_rgb(surfaces)) as uint32, and canvas
    f * T is the untiled letterbox_<kind> canvas of frame f. Both colour settings on every kind of the
    first shape; on the other shapes the kinds alternate between them. resnet weights: the space-to-depth
    canvases, mnet weights: the NHWC ones."""
    n, T = 2, 1 + tiles[0] * tiles[1]
    ctx = face_ctx_factory(precision, max_batch=n * T, wkind=wkind, tiles=tiles, tile_overlap=ov)
    nv = _noise(n, h, w, h * 1000 + w + ov)
    want = {}
    for m, r in COLOURS:
        rgb = nr.to_rgb(nv, m, r)
        want[m, r] = _bits(ctx.letterbox_tiles(_cuda(rgb)))
        assert want[m, r].shape[0] == n * T
    assert not np.array_equal(want[COLOURS[0]], want[COLOURS[1]])
    for k, (name, tiled, plain) in enumerate(_kinds(nv, h, w, h + ov)):
        for j, (m, r) in enumerate(COLOURS):
            if (h, w, tiles, ov) != LB_SHAPES[0] and (j + k) % 2:
                continue
            got = _bits(tiled(ctx, m, r))
            for i in range(n * T):
                assert np.array_equal(got[i], want[m, r][i]), f"{name} {m} {r}: canvas {i} (frame {i // T}, rectangle {i % T})"
            whole = _bits(plain(ctx, m, r))
            for f in range(n):
                assert np.array_equal(got[f * T], whole[f]), f"{name} {m} {r}: frame {f} against the untiled canvas"


# ---- 2. a frame too wide for the staged path, tiles that take it -----------------------------------------

def test_wide_frame_unstaged_whole_frame_and_staged_tiles_in_one_launch(face_ctx_factory):
    """w = 5464: 3 * 5464 bytes exceed the staged-row limit (16384), so rectangle 0 takes the per-block path
    while the 2732-px tiles are staged, in the same launch; an 8-bit planar and a 16-bit interleaved surface."""
    h, w, n = 6, 5464, 1
    ctx = face_ctx_factory("fp32", max_batch=3, wkind="default", tiles=(1, 2), tile_overlap=0)
    assert ctx.tile_rects(h, w).tolist() == [[0, 0, w, h], [0, 0, 2732, h], [2732, 0, 2732, h]]
    nv = _noise(n, h, w, 7)
    m, r = COLOURS[1]
    want = _bits(ctx.letterbox_tiles(_cuda(nr.to_rgb(nv, m, r))))
    assert len({want[i].tobytes() for i in range(3)}) == 3
    for name, got in (("i420", ctx.letterbox_tiles_yuv420(_surf8(nv, "i420", h, w), matrix=m, range=r)),
                      ("p010", ctx.letterbox_tiles_yuv420_16(_surf16(nv, "nv12", 10, 6, h, w, 3), matrix=m, range=r))):
        for i in range(3):
            assert np.array_equal(_bits(got)[i], want[i]), f"{name}: canvas {i}"


# ---- 3. the plate net's tile inputs ----------------------------------------------------------------------

@pytest.mark.parametrize("tiling", [dict(tiles=(1, 3), tile_overlap=0), T22], ids=["1x3", "2x2"])
def test_plate_tile_inputs_equal_those_of_the_converted_frames(face_ctx_factory, tiling):
    h, w, n = 174, 212, 2
    ctx = _ctx(face_ctx_factory, **tiling, tile_nets="plates")
    nv = _noise(n, h, w, 91)
    for lay, (m, r) in zip(("i420", "nv21"), COLOURS):
        want = ctx.plate_raw_tiles(_cuda(nr.to_rgb(nv, m, r)))
        got = ctx.plate_raw_tiles_yuv420(_surf8(nv, lay, h, w), matrix=m, range=r)
        assert got.shape == want.shape and got.shape[0] == n * tiling["tiles"][0] * tiling["tiles"][1]
        assert np.abs(want).max() > 0
        assert np.array_equal(_bits(got), _bits(want)), lay


# ---- 4. end to end ---------------------------------------------------------------------------------------

def _all_flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _scene(idx, seed=5):
    """Synthetic 360 x 640 scenes on which the seeded weights fire (pixels doubled), as packed NV12."""
    from vdmi import synth
    rgb = np.stack([np.repeat(np.repeat(synth.frame(H // 2, W // 2, i, seed=seed), 2, 0), 2, 1) for i in idx])
    return nr.from_rgb(rgb)


def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _labels(boxes, b):
    return [int(v) for v in boxes.label[b, :int(boxes.count[b])]]


def _fields_equal(a, b, n):
    """Every field of every box of frames [0, n), bit by bit; -> the number of boxes."""
    assert np.array_equal(a.count[:n], b.count[:n])
    total = 0
    for i in range(n):
        for x, y in zip(a.frame(i), b.frame(i)):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y), i
        total += int(a.count[i])
    return total


def _arrays(lists):
    cap = max(1, max(len(b) for b in lists))
    xy = np.zeros((len(lists), cap, 4), np.int32)
    for i, b in enumerate(lists):
        xy[i, :len(b)] = np.asarray(b, np.int32).reshape(-1, 4)
    return xy, np.asarray([len(b) for b in lists], np.int32)


P010 = dict(layout="nv12", depth=10, shift=6)
ENTRIES = {
    # name: surfaces of packed NV12 frames, the call, the stand-alone blur of caller lists on those surfaces
    "nv12": (lambda nv: _cuda(nv),
             lambda c, s: c.process_nv12(s, flags=_all_flags()),
             lambda c, s, xy, cnt: c.mosaic_nv12(s, xy, cnt)),
    "i420_to_nv12": (lambda nv: _cuda(yr.from_nv12(nv, "i420")),
                     lambda c, s: c.process_yuv420(s, flags=_all_flags(), layout="i420", out_layout="nv12"),
                     lambda c, s, xy, cnt: c.mosaic_yuv420(s, xy, cnt, layout="i420", out_layout="nv12")),
    "p010": (lambda nv: _cuda16(y16.widen(nv, 10, 6, 17)),
             lambda c, s: c.process_yuv420_16(s, flags=_all_flags(), **P010),
             lambda c, s, xy, cnt: c.mosaic_yuv420_16(s, xy, cnt, **P010)),
}
MODES = {"pixelate_hold": dict(hold=2), "smooth_ellipse": dict(blur="gaussian", cells=8, mask="ellipse", mask_grow=42)}
_RGB = {}


def _rgb_run(ctx, mode, calls):
    """process() of the converted frames in the same tiled context: per call (faces, plates, held lists)."""
    if mode not in _RGB:
        ctx.hold_reset()
        runs = []
        for nv in calls:
            _, faces, plates = ctx.process(nr.to_rgb(nv), flags=_all_flags())
            n = len(nv)
            held = [_lists(ctx.read_held(n), i) for i in range(n)] if ctx.cfg.hold_frames else [[] for _ in range(n)]
            runs.append((faces, plates, held))
        _RGB[mode] = runs
    return _RGB[mode]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_process_lists_and_surfaces(face_ctx_factory, mode, entry):
    """tiles (2, 2), both nets tiled, faces + plates + mosaic + mosaic_plates. Lists: process() of the
    converted frames in an RGB call with the same settings, field by field; surfaces: the stand-alone
    surface blur of faces ++ plates ++ held on the input surfaces. pixelate_hold: hold = 2 over two
    consecutive calls; smooth_ellipse: the scaled smooth blur under an ellipse mask."""
    ctx = _ctx(face_ctx_factory, **T22, **SURF, **MODES[mode])
    assert ctx.tile_surfaces and ctx.frames_per_call() == 2
    calls = [_scene([0, 1]), _scene([2, 0])] if mode == "pixelate_hold" else [_scene([0, 1])]
    want = _rgb_run(ctx, mode, calls)
    ctx.hold_reset()
    surf, call, blur = ENTRIES[entry]
    nfaces = nheld = 0
    for nv, (faces0, plates0, held0) in zip(calls, want):
        s = surf(nv)
        out, faces, plates = call(ctx, s)
        nfaces += _fields_equal(faces, faces0, 2)
        _fields_equal(plates, plates0, 2)
        _fields_equal(ctx.read_boxes(0, 2), faces0, 2)       # the merged rows the library keeps
        held = [_lists(ctx.read_held(2), i) for i in range(2)] if ctx.cfg.hold_frames else [[], []]
        assert held == held0
        nheld += sum(len(x) for x in held)
        bl = [_lists(faces, i) + _lists(plates, i) + held[i] for i in range(2)]
        ref = blur(ctx, s, *_arrays(bl))
        np.testing.assert_array_equal(_np(out), _np(ref))
        assert not np.array_equal(_np(out), _np(s))
    assert nfaces > 0 and (mode != "pixelate_hold" or nheld > 0)
    # ... and tiling shows: the untiled context's face lists differ on some frame
    _, plain, _ = _ctx(face_ctx_factory).process(nr.to_rgb(calls[0]), flags=_all_flags())
    assert any(_lists(plain, i) != _lists(want[0][0], i) for i in range(2))


# ---- 5. look-ahead ---------------------------------------------------------------------------------------

LEAD = {
    "nv12": (lambda nv: _cuda(nv), lambda c, s, fl: c.process_lead_nv12(s, flags=_all_flags(), flush=fl),
             lambda c, s, xy, cnt: c.mosaic_nv12(s, xy, cnt)),
    "i420": (lambda nv: _cuda(yr.from_nv12(nv, "i420")), lambda c, s, fl: c.process_lead_yuv420(s, flags=_all_flags(), flush=fl),
             lambda c, s, xy, cnt: c.mosaic_yuv420(s, xy, cnt)),
    "rgb": (lambda nv: nr.to_rgb(nv), lambda c, s, fl: c.process_lead(s, flags=_all_flags(), flush=fl), None),
}


def _lead_run(ctx, kind, clip, cuts):
    """The clip through the look-ahead call of `kind` in `cuts`, the last call flushing: the emitted frames
    in order, D of every pushed frame, and (one library call per cut only) (B_t, labels) of every emitted one."""
    surf, push, _ = LEAD[kind]
    outs, D, B, lo = [], [], [], 0
    for k, n in enumerate(cuts):
        out, faces, plates = push(ctx, surf(clip[lo:lo + n]), k == len(cuts) - 1)
        D += [(_lists(faces, b), _lists(plates, b)) for b in range(n)]
        m = len(out)
        if n <= ctx.frames_per_call() and m:
            rows = ctx.read_lead(m, "all")
            B += [(_lists(rows, i), _labels(rows, i)) for i in range(m)]
        outs += list(_np(out))
        lo += n
    assert ctx.lead_pending() == 0 and len(outs) == len(clip)
    return outs, D, B


_LEAD_RGB = {}


@pytest.mark.parametrize("kind", ["nv12", "i420"])
def test_look_ahead_on_tiled_surfaces(face_ctx_factory, kind):
    """lead = 2, both nets tiled, 6 frames: the lists (read_lead) equal process_lead's on the converted
    frames, the emitted surfaces are the stand-alone blur of B_t, and calls of 4 + 2 (which Python splits
    into 2 + 2 and 2) give what calls of 2 + 2 + 2 give."""
    ctx = _ctx(face_ctx_factory, **T22, **SURF, lead=2)
    a, b, c = _scene([0, 1, 2])
    clip = np.stack([a, a, b, b, c, a])
    if "rgb" not in _LEAD_RGB:
        _LEAD_RGB["rgb"] = _lead_run(ctx, "rgb", clip, (2, 2, 2))[1:]
        ctx.hold_reset()
    D0, B0 = _LEAD_RGB["rgb"]
    outs, D, B = _lead_run(ctx, kind, clip, (2, 2, 2))
    assert D == D0 and B == B0 and len(B) == 6
    assert any(v < 0 for _, lab in B for v in lab) and sum(len(f) for f, _ in D) > 0      # some A_t is non-empty
    blur = LEAD[kind][2]
    ref = _np(blur(ctx, LEAD[kind][0](clip), *_arrays([b for b, _ in B])))
    for t in range(6):
        np.testing.assert_array_equal(outs[t], ref[t], err_msg=f"frame {t}")
    assert any(not np.array_equal(outs[t], _np(LEAD[kind][0](clip))[t]) for t in range(6))
    ctx.hold_reset()
    outs2, D2, _ = _lead_run(ctx, kind, clip, (4, 2))
    assert D2 == D
    for t in range(6):
        np.testing.assert_array_equal(outs2[t], outs[t], err_msg=f"4 + 2: frame {t}")


# ---- 6. the Python split ---------------------------------------------------------------------------------

def test_python_split_of_a_long_batch(face_ctx_factory):
    """max_batch 10, T = 5: a call carries 2 frames; process_yuv420 of 5 frames equals the calls of 2 + 2 + 1."""
    ctx = _ctx(face_ctx_factory, **T22, **SURF)
    assert ctx.frames_per_call() == 2
    s = yr.from_nv12(_scene([0, 1, 2, 0, 1]), "i420")
    dev = _cuda(s)
    out, faces, plates = ctx.process_yuv420(dev, flags=_all_flags())
    assert faces.n == 5 and plates.n == 5 and int(faces.count.sum()) > 0
    r = 0
    for lo in (0, 2, 4):
        o, f, p = ctx.process_yuv420(dev[lo:lo + 2], flags=_all_flags())
        k = len(o)
        for i in range(k):
            for x, y in zip(faces.frame(r) + plates.frame(r), f.frame(i) + p.frame(i)):
                assert np.array_equal(x, y), (r, i)
            r += 1
        np.testing.assert_array_equal(_np(out[lo:lo + k]), _np(o))
    assert r == 5
    host, fh, _ = ctx.process_yuv420(s, flags=_all_flags())                      # host frames split the same way
    np.testing.assert_array_equal(host, _np(out))
    _fields_equal(fh, faces, 5)


# ---- 7. the switch ---------------------------------------------------------------------------------------

def test_the_switch(gpu):
    import vdmi
    from conftest import face_weights
    from vdmi import _lib, weights
    ctx = vdmi.Context(precision="fp32", max_batch=10, hold=2, lead=0)
    lead = None
    try:
        ctx.load_weights(0, face_weights("dense"))
        ctx.load_weights(1, weights.yolov8n_state_dict(0))
        assert ctx.tile_surfaces is False
        nv = _scene([0, 1, 2])
        first, faces1, _ = ctx.process_nv12(nv[:2], flags=_all_flags())           # untiled: history of two frames
        held1 = [_lists(ctx.read_held(2), i) for i in range(2)]
        ctx.hold_reset()
        ctx.set_tiles((2, 2), 20)                                                 # (forgets the hold history itself)
        # default off: refused as ever, and the message says how to ask for it
        for call in (lambda: ctx.process_nv12(nv[:2], flags=_all_flags()),
                     lambda: ctx.process_yuv420(yr.from_nv12(nv[:2], "i420"), flags=_all_flags()),
                     lambda: ctx.process_yuv420_16(y16.widen(nv[:2], 10, 6, 1), flags=_all_flags(), **P010)):
            with pytest.raises(_lib.VdError, match="tile") as e:
                call()
            assert e.value.code == _lib.VD_ERR_STATE and "vd_tiles_surfaces" in str(e.value)
        # bad values: refused, the setting unchanged
        with pytest.raises(_lib.VdError) as e:
            ctx.set_tile_surfaces(2)
        assert e.value.code == _lib.VD_ERR_ARG and ctx.tile_surfaces is False
        assert ctx._lib.vd_tiles_surfaces(ctx._h, -1) == _lib.VD_ERR_ARG
        with pytest.raises(_lib.VdError, match="tile"):
            ctx.process_nv12(nv[:2], flags=_all_flags())
        # nothing changed: the untiled call gives what it gave
        ctx.set_tiles((1, 1), 20)
        again, faces2, _ = ctx.process_nv12(nv[:2], flags=_all_flags())
        np.testing.assert_array_equal(again, first)
        _fields_equal(faces2, faces1, 2)
        assert [_lists(ctx.read_held(2), i) for i in range(2)] == held1
        # turning it on keeps the hold history: the next untiled call holds what it would have held
        want_out, _, _ = ctx.process_nv12(nv[2:], flags=_all_flags())
        want_held = _lists(ctx.read_held(1), 0)
        ctx.hold_reset()
        ctx.process_nv12(nv[:2], flags=_all_flags())
        ctx.set_tile_surfaces(True)
        assert ctx.tile_surfaces is True
        ctx.set_tile_surfaces(True)                                               # the value it has: nothing happens
        got_out, _, _ = ctx.process_nv12(nv[2:], flags=_all_flags())
        assert _lists(ctx.read_held(1), 0) == want_held and len(want_held) > 0
        np.testing.assert_array_equal(got_out, want_out)
        # on: n * T <= max_batch through the C entry, as for RGB
        ctx.set_tiles((2, 2), 20)
        d, n, h, w, where, keep = vdmi.context._nv12_arg(nv)
        fb = _lib.HostBoxes(3, 16)
        rc = ctx._lib.vd_process_nv12(ctx._h, ctypes.byref(d), None, 3, h, w, where, _lib.VD_PROC_FACES,
                                      ctypes.byref(fb.struct()), None)
        assert rc == _lib.VD_ERR_ARG and "largest n: 2" in _lib.last_error()
        _, faces, _ = ctx.process_nv12(nv, flags=_lib.VD_PROC_FACES)              # Python splits 3 into 2 + 1
        assert faces.n == 3 and int(faces.count.sum()) > 0
        # rescue with tiling stays refused
        with pytest.raises(_lib.VdError, match="tiled detection") as e:
            ctx.rescue(0.3, 0.0)
        assert e.value.code == _lib.VD_ERR_STATE
        # refused while lead frames are pending
        lead = vdmi.Context(precision="fp32", max_batch=10, lead=1, tiles=(2, 2), tile_surfaces=True)
        lead.load_weights(0, face_weights("dense"))
        out, _, _ = lead.process_lead_nv12(nv[:1], flags=_lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC)
        assert len(out) == 0 and lead.lead_pending() == 1
        with pytest.raises(_lib.VdError, match="pending") as e:
            lead.set_tile_surfaces(False)
        assert e.value.code == _lib.VD_ERR_STATE and lead.tile_surfaces is True and lead.lead_pending() == 1
        lead.set_tile_surfaces(True)                                              # the value it has: nothing to refuse
        assert len(lead.lead_flush()) == 1
        lead.set_tile_surfaces(False)
        with pytest.raises(_lib.VdError, match="vd_tiles_surfaces"):
            lead.process_lead_nv12(nv[:1], flags=_lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC)
        assert lead.lead_pending() == 0
    finally:
        ctx.close()
        if lead is not None:
            lead.close()
