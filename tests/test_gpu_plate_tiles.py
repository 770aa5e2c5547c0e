"""Tiled plate detection on the GPU (include/vdmi.h at vd_tiles_nets): the tile inputs' raw heads
against the plain forward of the crops, the class-aware merge kernel against
tests/plate_tiles_ref.py, detect_plates / process end to end against the reference merge of
per-crop detections, the hold on merged lists, the defaults, the Python batch split, and the
refusals. 360 x 640 frames, n = 2, max_batch 10, the fp32 plan, synthetic plate weights."""
import ctypes

import numpy as np
import pytest

import hold_ref as hr
import plate_tiles_ref as pr
import tiles_ref as tr
from oracle import mosaic as omosaic

pytestmark = pytest.mark.gpu

H, W = 360, 640
# plate_conf is the default: naming it keeps these contexts (which also hold plate weights) apart
# from the face-only contexts other modules cache under the same settings
NET = dict(precision="fp32", max_batch=10, wkind="dense", plate_conf=0.5)
T22 = dict(tiles=(2, 2), tile_overlap=20)
T13 = dict(tiles=(1, 3), tile_overlap=0)
TILINGS = {"2x2": T22, "1x3": T13}
IOU = 0.7


def _ctx(factory, **kw):
    from vdmi import weights
    ctx = factory(**{**NET, **kw})
    if not getattr(ctx, "_plates_loaded", False):
        ctx.load_weights(1, weights.yolov8n_state_dict(0))
        ctx._plates_loaded = True
    return ctx


def _frames(n, seed=5):
    from vdmi import synth
    return np.stack([np.repeat(np.repeat(synth.frame(H // 2, W // 2, i, seed=seed), 2, 0), 2, 1) for i in range(n)])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(b, i):
    k = int(b.count[i])
    assert k <= b.cap
    return b.xyxy[i, :k], b.xyxy_f[i, :k], b.score[i, :k], b.label[i, :k]


def _assert_lists_equal(got, ref, frames, first=0):
    """got: HostBoxes (complete), rows [first, first + frames); ref: per frame (xyxy, xyxy_f, score, label, ..)."""
    for f in range(frames):
        xi, xf, sc, lab = _rows(got, first + f)
        assert len(xi) == len(ref[f][0]), f"frame {f}: count {len(xi)} != {len(ref[f][0])}"
        assert np.array_equal(xi, ref[f][0]), f"frame {f}: int boxes"
        assert np.array_equal(_bits(xf), _bits(ref[f][1])), f"frame {f}: float boxes"
        assert np.array_equal(_bits(sc), _bits(ref[f][2])), f"frame {f}: scores"
        assert np.array_equal(lab, ref[f][3]), f"frame {f}: labels"


def _same_rows(a, b, frames):
    assert np.array_equal(a.count[:frames], b.count[:frames])
    for f in range(frames):                               # entries past a frame's count are not defined
        for x, y in zip(_rows(a, f), _rows(b, f)):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y), f


def _crops(frames, rects, tiles_only=False):
    """The rectangles of every frame as standalone frames, in input order."""
    out = []
    for f in range(len(frames)):
        for (x0, y0, tw, th) in rects.tolist()[1 if tiles_only else 0:]:
            out.append(np.ascontiguousarray(frames[f, y0:y0 + th, x0:x0 + tw]))
    return out


# ---- 1. raw heads of the tile inputs ---------------------------------------------------------------

@pytest.mark.parametrize("tiling,pitched", [("2x2", False), ("1x3", False), ("2x2", True)])
def test_plate_raw_tiles_equals_plate_raw_of_the_crops(face_ctx_factory, tiling, pitched):
    """Input f * R * C + (t - 1) of plate_raw_tiles is, bit for bit, plate_raw() of a standalone
    frame holding tile t of frame f (the tile letterbox kernel and the forward over n * R * C
    inputs against the plain letterbox and a forward over one input); device frames whose row
    pitch exceeds 3w in one case."""
    import torch
    tiled = _ctx(face_ctx_factory, **TILINGS[tiling], tile_nets="plates")
    plain = _ctx(face_ctx_factory)
    frames = _frames(2)
    rects = tiled.tile_rects(H, W)
    RC = len(rects) - 1
    src = frames
    if pitched:
        big = torch.zeros((2, H, W + 13, 3), dtype=torch.uint8, device="cuda")
        big[:, :, :W] = torch.from_numpy(frames).cuda()
        src = big[:, :, :W]
        torch.cuda.synchronize()                            # the context reads them on its own stream
        assert src.stride(1) > 3 * W
    got = tiled.plate_raw_tiles(src)
    assert got.shape[0] == 2 * RC
    for i, crop in enumerate(_crops(frames, rects, tiles_only=True)):
        want = plain.plate_raw(crop[None])
        assert want.shape[1:] == got.shape[1:], (i, want.shape, got.shape)
        assert np.array_equal(_bits(got[i]), _bits(want[0])), i
    if tiling == "1x3":       # portrait tiles of a landscape frame: a 640 x 384 canvas against the frame's 384 x 640
        assert rects[1, 2] < rects[1, 3] and W > H


# ---- 2. the merge kernel alone ---------------------------------------------------------------------

def _object_lists(rng, n, rects, cap, nobj, labels, scores=None, keep=0.8):
    """HostBoxes of n * T rows: objects of the frame as every input that holds them sees them
    (moved by up to 2 px: most pairs overlap by more than 0.7, some by less), the class drawn per
    sighting, so inputs may disagree on it."""
    from vdmi import _lib
    T = len(rects)
    b = _lib.HostBoxes(n * T, cap)
    for f in range(n):
        x1 = rng.uniform(0, rects[0][2] - 100, nobj)
        y1 = rng.uniform(0, rects[0][3] - 40, nobj)
        x2, y2 = x1 + rng.uniform(12, 90, nobj), y1 + rng.uniform(6, 30, nobj)
        for t, (x0, y0, tw, th) in enumerate(rects.tolist()):
            seen = (x1 >= x0) & (y1 >= y0) & (x2 <= x0 + tw) & (y2 <= y0 + th) & (rng.uniform(size=nobj) < keep)
            k = min(int(seen.sum()), cap)
            r = f * T + t
            b.count[r] = k
            xy = np.stack([x1 - x0, y1 - y0, x2 - x0, y2 - y0], 1)[seen][:k] + rng.uniform(-2, 2, (k, 4))
            b.xyxy_f[r, :k] = xy
            b.score[r, :k] = rng.choice(scores, k) if scores is not None else rng.uniform(0.5, 1, k)
            b.label[r, :k] = rng.choice(labels, k)
    return b


def _device(b):
    import torch
    from vdmi.context import DeviceBoxes
    d = DeviceBoxes(b.n, b.cap, "cuda")
    for k in ("count", "xyxy", "xyxy_f", "score", "label"):
        getattr(d, k).copy_(torch.from_numpy(getattr(b, k)))
    torch.cuda.synchronize()                            # the context reads them on its own stream
    return d


MERGE_CASES = ["repeated_scores", "identical_box", "labels", "all_empty", "one_empty", "spill"]
_MERGE = {}


def _merge_case(case, rects):
    """(lists, reference) of a case, computed once for the host and the device run."""
    if case in _MERGE:
        return _MERGE[case]
    from vdmi import _lib
    n, T = 2, len(rects)
    rng = np.random.default_rng(100 + MERGE_CASES.index(case))
    one = np.asarray([0])
    if case == "repeated_scores":
        lists = _object_lists(rng, n, rects, 96, 90, one, scores=np.asarray([0.5, 0.625, 0.75, 0.9], np.float32))
    elif case == "identical_box":                           # one plate seen by the frame and by three tiles
        lists = _object_lists(rng, n, rects, 8, 4, one)
        lists.count[:] = np.maximum(lists.count, 2)
        for f in range(n):
            for t in (0, 1, 2, 4):
                x0, y0 = rects[t, 0], rects[t, 1]
                lists.xyxy_f[f * T + t, 1] = [700 - x0, 350 - y0, 760 - x0, 370 - y0]
                lists.score[f * T + t, 1] = 0.9990234375
                lists.label[f * T + t, 1] = 0
    elif case == "labels":
        lists = _object_lists(rng, n, rects, 96, 90, np.asarray([0, 1, 2]))
    elif case == "all_empty":
        lists = _lib.HostBoxes(n * T, 4)
    elif case == "one_empty":
        lists = _object_lists(rng, n, rects, 32, 40, one)
        lists.count[2::T] = 0
    else:                                                   # frame 0: more than the 2048 boxes held in LDS
        lists = _object_lists(rng, n, rects, 520, 1400, np.asarray([0, 1, 2]),
                              scores=np.linspace(0.5, 1, 300).astype(np.float32), keep=1.0)
        lists.count[T:] = np.minimum(lists.count[T:], 30)
    _MERGE[case] = (lists, pr.merge(lists, n, rects, IOU))
    return _MERGE[case]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", MERGE_CASES)
def test_tiles_merge_plates_equals_reference(face_ctx_factory, case, device):
    """plate_max_det 1000: lists of up to 1000 boxes per input, so T * 520 boxes spill past LDS."""
    ctx = _ctx(face_ctx_factory, **T22, tile_nets="plates", plate_max_det=1000)
    h, w, n, T = 720, 1280, 2, 5
    rects = ctx.tile_rects(h, w)
    lists, ref = _merge_case(case, rects)
    got = ctx.tiles_merge_plates(_device(lists) if device else lists, h, w)
    _assert_lists_equal(got, ref, n)
    total = int(np.minimum(lists.count, lists.cap).sum())
    kept = sum(len(r[0]) for r in ref)
    if case in ("repeated_scores", "labels", "one_empty", "spill"):
        assert 0 < kept < total
    if case == "labels":                                    # the classes matter: one class keeps fewer
        flat = type(lists).__new__(type(lists))
        flat.__dict__.update(lists.__dict__)
        flat.label = np.zeros_like(lists.label)
        assert sum(len(r[0]) for r in pr.merge(flat, n, rects, IOU)) < kept
        assert all(set(r[3].tolist()) == {0, 1, 2} for r in ref)
    if case == "identical_box":
        assert all((0, 1) in r[4] and not any(s in r[4] for s in ((1, 1), (2, 1), (4, 1))) for r in ref)
    if case == "all_empty":
        assert kept == 0
    if case == "spill":
        assert int(lists.count[:T].sum()) > 2048 and len(ref[0][0]) > 64
        # an output cap smaller than the merged count: count complete, arrays cut at cap
        from vdmi import _lib
        small = ctx.tiles_merge_plates(lists, h, w, out=_lib.HostBoxes(n, 64))
        for f in range(n):
            assert int(small.count[f]) == len(ref[f][0])
            k = min(64, len(ref[f][0]))
            assert np.array_equal(small.xyxy[f, :k], ref[f][0][:k])
            assert np.array_equal(_bits(small.xyxy_f[f, :k]), _bits(ref[f][1][:k]))
            assert np.array_equal(small.label[f, :k], ref[f][3][:k])


def test_tiles_merge_plates_label_optional_capacity_and_state(face_ctx_factory):
    from vdmi import _lib
    ctx = _ctx(face_ctx_factory, **T22, tile_nets="plates")
    rects = ctx.tile_rects(720, 1280)
    lists = _object_lists(np.random.default_rng(11), 1, rects, 8, 6, np.asarray([0, 1]))
    s = lists.struct()
    s.label = None                                          # no labels: every box of class 0
    out = _lib.HostBoxes(1, 64)
    _lib.check(ctx._lib.vd_tiles_merge_plates(ctx._h, ctypes.byref(s), 1, 720, 1280, ctypes.byref(out.struct())))
    lists.label[:] = 0
    _assert_lists_equal(out, pr.merge(lists, 1, rects, IOU), 1)
    lists.count[3] = 9                                      # a host list the caller does not hold
    with pytest.raises(_lib.VdCapacityError):
        ctx.tiles_merge_plates(lists, 720, 1280)
    lists.count[3] = 0
    big = _lib.HostBoxes(5, 301)                            # past the per-input keep capacity (plate_max_det 300)
    rc = ctx._lib.vd_tiles_merge_plates(ctx._h, ctypes.byref(big.struct()), 1, 720, 1280, None)
    assert rc == _lib.VD_ERR_ARG
    plain = _ctx(face_ctx_factory)
    rc = plain._lib.vd_tiles_merge_plates(plain._h, ctypes.byref(lists.struct()), 1, 720, 1280, None)
    assert rc == _lib.VD_ERR_STATE and "tiling is off" in _lib.last_error()
    faces_only = face_ctx_factory(precision="fp32", max_batch=10, wkind="dense", **T22)   # no plate weights
    rc = faces_only._lib.vd_tiles_merge_plates(faces_only._h, ctypes.byref(lists.struct()), 1, 720, 1280, None)
    assert rc == _lib.VD_ERR_STATE and "plate weights" in _lib.last_error()


# ---- 3. end to end ---------------------------------------------------------------------------------

_E2E = {}


def _e2e(factory, tiling):
    """2 frames through the context with the plate net tiled, and the reference merge of the
    untiled context's plate detections of the T rectangles of each frame (computed once)."""
    if tiling not in _E2E:
        from vdmi import _lib
        frames = _frames(2)
        tiled = _ctx(factory, **TILINGS[tiling], tile_nets="plates")
        plain = _ctx(factory)
        rects = tiled.tile_rects(H, W)
        T = len(rects)
        per = [plain.detect_plates(c[None]) for c in _crops(frames, rects)]
        lists = _lib.HostBoxes(2 * T, max(1, max(int(b.count[0]) for b in per)))
        for r, b in enumerate(per):
            k = int(b.count[0])
            lists.count[r] = k
            for name in ("xyxy", "xyxy_f", "score", "label"):
                getattr(lists, name)[r, :k] = getattr(b, name)[0, :k]
        _E2E[tiling] = (frames, tiled, plain, rects, lists, pr.merge(lists, 2, rects, IOU))
    return _E2E[tiling]


@pytest.mark.parametrize("tiling", ["2x2", "1x3"])
def test_detect_plates_equals_reference_merge_of_crop_detections(face_ctx_factory, tiling):
    frames, tiled, plain, rects, lists, ref = _e2e(face_ctx_factory, tiling)
    got = tiled.detect_plates(frames)
    print("per-input counts", lists.count.tolist(), "merged", [len(r[0]) for r in ref])
    _assert_lists_equal(got, ref, 2)
    # the inputs show something: kept boxes from the whole frame and from tiles, and (2 x 2: the
    # tiles overlap) boxes the cross-input NMS removed
    src = [s for r in ref for s in r[4]]
    assert any(t == 0 for t, _ in src) and any(t > 0 for t, _ in src)
    if tiling == "2x2":
        assert sum(len(r[0]) for r in ref) < int(lists.count.sum())
    else:
        assert np.all(lists.count > 0)
    # the per-input lists left in the library are untouched by the merge: read_boxes is the merged rows
    _assert_lists_equal(tiled.read_boxes(1, 2), ref, 2)


def test_detect_plates_bf16_equals_reference_merge(face_ctx_factory):
    """The same identity on the bf16 plan (one run, 2 x 2)."""
    from vdmi import _lib
    frames = _frames(2)
    kw = dict(precision="bf16")
    tiled = _ctx(face_ctx_factory, **kw, **T22, tile_nets="plates")
    plain = _ctx(face_ctx_factory, **kw)
    rects = tiled.tile_rects(H, W)
    per = [plain.detect_plates(c[None]) for c in _crops(frames, rects)]
    lists = _lib.HostBoxes(len(per), max(1, max(int(b.count[0]) for b in per)))
    for r, b in enumerate(per):
        k = int(b.count[0])
        lists.count[r] = k
        for name in ("xyxy", "xyxy_f", "score", "label"):
            getattr(lists, name)[r, :k] = getattr(b, name)[0, :k]
    ref = pr.merge(lists, 2, rects, IOU)
    assert sum(len(r[0]) for r in ref) > 0
    _assert_lists_equal(tiled.detect_plates(frames), ref, 2)


# ---- 4. process ------------------------------------------------------------------------------------

def _all_flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _concat(faces, plates, n):
    """faces ++ plates per frame as one HostBoxes (the blur list of VD_PROC_MOSAIC_PLATES)."""
    from vdmi import _lib
    out = _lib.HostBoxes(n, max(1, int((faces.count[:n] + plates.count[:n]).max())))
    for f in range(n):
        a, b = _rows(faces, f)[0], _rows(plates, f)[0]
        out.count[f] = len(a) + len(b)
        out.xyxy[f, :len(a)] = a
        out.xyxy[f, len(a):len(a) + len(b)] = b
    return out


@pytest.mark.parametrize("nets", ["plates", "both"])
def test_process_mosaics_faces_and_merged_plates(face_ctx_factory, nets):
    frames, _, plain, rects, lists, ref = _e2e(face_ctx_factory, "2x2")
    ctx = _ctx(face_ctx_factory, **T22, tile_nets=nets)
    out, faces, plates = ctx.process(frames, flags=_all_flags())
    rp = ctx.read_boxes(1, 2)
    _assert_lists_equal(rp, ref, 2)
    assert np.array_equal(plates.count, rp.count)
    rf = ctx.read_boxes(0, 2)
    if nets == "plates":      # the face net is not tiled: the untiled context's faces, bit for bit
        _same_rows(rf, plain.detect(frames), 2)
    else:                     # both: the merged face lists of a faces-only tiling
        _same_rows(rf, _ctx(face_ctx_factory, **T22).detect(frames), 2)
    assert int(rf.count.sum()) > 0
    both = _concat(rf, rp, 2)
    assert np.array_equal(out, ctx.mosaic(frames, both))
    b0 = [tuple(int(v) for v in b) for b in both.xyxy[0, :int(both.count[0])]]
    assert np.array_equal(out[0], omosaic.mosaic_frame(frames[0], b0, 8))
    assert not np.array_equal(out, ctx.mosaic(frames, rf))   # the plates are blurred too


def test_hold_runs_on_faces_and_merged_plates(face_ctx_factory):
    """hold = 2 over two calls: read_held equals tests/hold_ref.py applied to faces ++ merged plates."""
    K, P = 2, 30
    ctx = _ctx(face_ctx_factory, **T22, tile_nets="plates", hold=K)
    ctx.hold_reset()
    fr = _frames(3)
    seq = [fr[0], fr[1], fr[2], fr[0]]
    D, Hs, ages, nplates = [], [], [], 0
    for lo in (0, 2):
        _, faces, plates = ctx.process(np.stack(seq[lo:lo + 2]), flags=_all_flags())
        rf, rp = ctx.read_boxes(0, 2), ctx.read_boxes(1, 2)
        held = ctx.read_held(2)
        for b in range(2):
            D.append([tuple(int(v) for v in r) for r in list(_rows(rf, b)[0]) + list(_rows(rp, b)[0])])
            nplates += int(rp.count[b])
            k = int(held.count[b])
            Hs.append([tuple(int(v) for v in r) for r in held.xyxy[b, :k]])
            ages.append([int(v) for v in held.label[b, :k]])
    _, Hr, ar, _ = hr.hold_lists(D, H, W, K, P)
    assert Hs == Hr and ages == ar
    assert nplates > 0 and sum(len(h) for h in Hr) > 0


# ---- 5. defaults, and the Python split -------------------------------------------------------------

def _fam5_launches(ctx, frames):
    from vdmi import _lib
    ctx.timing(True)
    ctx.timing_reset()
    boxes = ctx.detect_plates(frames)
    ctx.sync()
    n = ctx.timing_read(_lib.FAM_PLATE_CONV)[1]
    ctx.timing(False)
    return boxes, n


def test_defaults_leave_the_plate_net_untiled(face_ctx_factory):
    frames = _frames(2)
    plain = _ctx(face_ctx_factory)
    want, launches = _fam5_launches(plain, frames)
    assert int(want.count.sum()) > 0 and launches > 0
    faces = _ctx(face_ctx_factory, **T22)                   # tile_nets left alone: faces only
    assert faces.tile_nets == "faces" and faces.frames_per_call(faces=False) == 10
    got, n = _fam5_launches(faces, frames)
    _same_rows(got, want, 2)
    assert n == launches
    _same_rows(faces.detect_plates(_frames(7)), plain.detect_plates(_frames(7)), 7)   # 7 frames: no n * T bound
    for nets in ("plates", "both"):                         # tiles (1, 1): any tile_nets is the untiled context
        off = _ctx(face_ctx_factory, tiles=(1, 1), tile_nets=nets)
        assert off.frames_per_call() == 10
        got, n = _fam5_launches(off, frames)
        _same_rows(got, want, 2)
        assert n == launches
    tiled, n = _fam5_launches(_ctx(face_ctx_factory, **T22, tile_nets="plates"), frames)
    assert n > launches                                     # and tiling the plate net does run more convs


def test_python_split_of_a_long_batch(face_ctx_factory):
    """max_batch 10, T = 5: a call that runs the tiled plate net carries 2 frames; detect_plates /
    process of 5 frames equal the sub-batches passed by hand; detect() of the untiled face net
    still takes all 5 at once."""
    ctx = _ctx(face_ctx_factory, **T22, tile_nets="plates")
    assert ctx.frames_per_call() == 2 and ctx.frames_per_call(plates=False) == 10
    frames = _frames(5)
    whole = ctx.detect_plates(frames)
    parts = [ctx.detect_plates(frames[s:s + 2]) for s in (0, 2, 4)]
    r = 0
    for p in parts:
        for i in range(p.n):
            for x, y in zip(_rows(whole, r), _rows(p, i)):
                assert np.array_equal(x, y)
            r += 1
    assert r == 5 and int(whole.count.sum()) > 0
    out, faces, plates = ctx.process(frames, flags=_all_flags())
    assert np.array_equal(plates.count, whole.count)
    _same_rows(faces, ctx.detect(frames), 5)
    for s in (0, 2, 4):
        ph, fh, qh = ctx.process(frames[s:s + 2], flags=_all_flags())
        assert np.array_equal(out[s:s + 2], ph)
        assert np.array_equal(plates.count[s:s + 2], qh.count)


# ---- 6. refusals -----------------------------------------------------------------------------------

def test_refusals_leave_the_state_unchanged(face_ctx_factory):
    from vdmi import _lib
    import vdmi
    ctx = _ctx(face_ctx_factory, **T22, tile_nets="plates")
    frames = _frames(3)
    want = ctx.detect_plates(frames[:2])
    for bad in (0, 4, -1, 7):                               # bad nets: refused, the setting unchanged
        assert ctx._lib.vd_tiles_nets(ctx._h, bad) == _lib.VD_ERR_ARG
    with pytest.raises(ValueError):
        ctx.set_tile_nets("plate")
    with pytest.raises(ValueError):
        vdmi.Context(precision="fp32", max_batch=1, tile_nets="all")
    out = _lib.HostBoxes(3, 16)                             # n * T > max_batch for a plates-only call
    rc = ctx._lib.vd_detect_plates(ctx._h, frames.ctypes.data, 3, H, W, W * 3, _lib.VD_HOST, ctypes.byref(out.struct()))
    assert rc == _lib.VD_ERR_ARG and "largest n: 2" in _lib.last_error()
    rc = ctx._lib.vd_process(ctx._h, frames.ctypes.data, None, 3, H, W, W * 3, _lib.VD_HOST, _lib.VD_PROC_PLATES, None,
                             ctypes.byref(out.struct()))
    assert rc == _lib.VD_ERR_ARG and "largest n: 2" in _lib.last_error()
    fo = _lib.HostBoxes(3, 16)                              # ... while a faces-only call of this context is not tiled
    _lib.check(ctx._lib.vd_detect(ctx._h, frames.ctypes.data, 3, H, W, W * 3, _lib.VD_HOST, ctypes.byref(fo.struct())))
    with pytest.raises(_lib.VdError, match="tiled detection") as e:   # rescue with tiling on, whatever the nets
        ctx.rescue(0.0, 0.3)
    assert e.value.code == _lib.VD_ERR_STATE
    nv = np.zeros((2, H * 3 // 2, W), np.uint8)             # an NV12 call that would run the tiled plate net
    with pytest.raises(_lib.VdError, match="tile") as e:
        ctx.process_nv12(nv, flags=_lib.VD_PROC_PLATES)
    assert e.value.code == _lib.VD_ERR_STATE
    ctx.process_nv12(nv, flags=_lib.VD_PROC_FACES)          # the untiled face net still takes NV12 frames
    _same_rows(ctx.detect_plates(frames[:2]), want, 2)      # nothing changed
    assert ctx.tile_nets == "plates" and ctx.frames_per_call() == 2


def test_tile_nets_change_is_refused_while_lead_frames_are_pending(face_ctx_factory):
    from vdmi import _lib
    ctx = _ctx(face_ctx_factory, **T22, tile_nets="plates", lead=1)
    frames = _frames(2)
    out, _, _ = ctx.process_lead(frames[:1], flags=_all_flags())
    assert len(out) == 0 and ctx.lead_pending() == 1
    with pytest.raises(_lib.VdError, match="pending") as e:
        ctx.set_tile_nets("both")
    assert e.value.code == _lib.VD_ERR_STATE
    assert ctx.tile_nets == "plates" and ctx.lead_pending() == 1
    ctx.set_tile_nets("plates")                             # the value it already has: nothing to refuse
    out, _, plates = ctx.process_lead(frames[1:], flags=_all_flags(), flush=True)
    assert len(out) == 2 and ctx.lead_pending() == 0
    _, _, _, _, _, ref = _e2e(face_ctx_factory, "2x2")
    _assert_lists_equal(ctx.read_boxes(1, 1), ref[1:], 1)   # the frame pushed last: its merged plate list
    ctx.set_tile_nets("both")                               # nothing pending: the change goes through
    ctx.set_tile_nets("plates")
