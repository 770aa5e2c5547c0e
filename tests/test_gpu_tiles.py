"""Tiled face detection on the GPU (include/vdmi.h at vd_tiles): the tile letterbox against the
plain letterbox of the crops, the merge kernel against tests/tiles_ref.py, detect / process end
to end against the reference merge of per-crop detections, the hold on merged lists, the
tiling-off identity, the Python batch split, and the refusals."""
import ctypes

import numpy as np
import pytest

import gaussian_ref as gr
import hold_ref as hr
import tiles_ref as tr
from oracle import mosaic as omosaic

pytestmark = pytest.mark.gpu

A640 = 16800           # anchors of the 640 x 640 canvas: 2 * (80^2 + 40^2 + 20^2)
H, W = 360, 640
NET = dict(precision="fp32", max_batch=10, wkind="dense")
TILED = dict(tiles=(2, 2), tile_overlap=20)


def _frames(n, seed=5):
    from vdmi import synth
    return np.stack([np.repeat(np.repeat(synth.frame(H // 2, W // 2, i, seed=seed), 2, 0), 2, 1) for i in range(n)])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(b, i):
    k = int(b.count[i])
    assert k <= b.cap
    return b.xyxy[i, :k], b.xyxy_f[i, :k], b.score[i, :k], b.label[i, :k]


def _assert_lists_equal(got, ref, frames):
    """got: HostBoxes (complete); ref: per frame (xyxy, xyxy_f, score, label, ..)."""
    for f in range(frames):
        xi, xf, sc, lab = _rows(got, f)
        assert len(xi) == len(ref[f][0]), f"frame {f}: count {len(xi)} != {len(ref[f][0])}"
        assert np.array_equal(xi, ref[f][0]), f"frame {f}: int boxes"
        assert np.array_equal(_bits(xf), _bits(ref[f][1])), f"frame {f}: float boxes"
        assert np.array_equal(_bits(sc), _bits(ref[f][2])), f"frame {f}: scores"
        assert np.array_equal(lab, ref[f][3]), f"frame {f}: labels"


# ---- 1. letterbox ---------------------------------------------------------------------------

LB_SHAPES = [(173, 211, (2, 2), 20), (173, 211, (1, 3), 0), (173, 211, (3, 1), 50), (37, 53, (4, 4), 50)]


@pytest.mark.parametrize("precision,wkind,h,w,tiles,ov",
                         [(p, "default") + s for p in ("fp32", "bf16") for s in LB_SHAPES] +
                         [(p, "mnet") + LB_SHAPES[0] for p in ("fp32", "bf16")])
def test_letterbox_tiles_equals_letterbox_of_the_crops(face_ctx_factory, precision, wkind, h, w, tiles, ov):
    """Canvas f * T + t of letterbox_tiles is, bit for bit, letterbox() of a standalone frame
    holding rectangle t of frame f; frames with a row pitch larger than 3w. resnet weights: the
    space-to-depth canvases (fp16 / bf16), mnet weights: the NHWC ones (f32 / bf16)."""
    import torch
    n, T = 2, 1 + tiles[0] * tiles[1]
    ctx = face_ctx_factory(precision, max_batch=n * T, wkind=wkind, tiles=tiles, tile_overlap=ov)
    rng = np.random.default_rng(h * 1000 + w)
    host = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    big = torch.zeros((n, h, w + 13, 3), dtype=torch.uint8, device="cuda")
    big[:, :, :w] = torch.from_numpy(host).cuda()
    view = big[:, :, :w]
    torch.cuda.synchronize()                            # the context reads them on its own stream
    assert view.stride(1) > 3 * w
    got = ctx.letterbox_tiles(view)
    rects = ctx.tile_rects(h, w)
    assert np.array_equal(rects, tr.tile_rects(h, w, tiles[0], tiles[1], ov)) and got.shape[0] == n * T
    done = {}
    for f in range(n):
        for t, (x0, y0, tw, th) in enumerate(rects.tolist()):
            crop = np.ascontiguousarray(host[f, y0:y0 + th, x0:x0 + tw])
            key = (f, x0, y0)
            if key + (tw, th) not in done:                  # coinciding tiles: one letterbox call
                done[key + (tw, th)] = ctx.letterbox(crop[None])[0]
            assert np.array_equal(_bits(got[f * T + t]), _bits(done[key + (tw, th)])), (f, t)


# ---- 2. the merge kernel alone -----------------------------------------------------------------

def _random_lists(rng, n, T, cap, tw, th, fill, scores=None):
    """HostBoxes of n * T rows with `fill(r)` boxes in row r, inside a tw x th rectangle."""
    from vdmi import _lib
    b = _lib.HostBoxes(n * T, cap)
    for r in range(n * T):
        k = fill(r)
        b.count[r] = k
        x1 = rng.uniform(-4, tw - 8, k)
        y1 = rng.uniform(-4, th - 8, k)
        b.xyxy_f[r, :k, 0], b.xyxy_f[r, :k, 1] = x1, y1
        b.xyxy_f[r, :k, 2] = x1 + rng.uniform(4, 90, k)
        b.xyxy_f[r, :k, 3] = y1 + rng.uniform(4, 90, k)
        b.score[r, :k] = rng.choice(scores, k) if scores is not None else rng.uniform(0.5, 1, k)
        b.label[r, :k] = rng.integers(0, A640, k)
    return b


def _device(b):
    import torch
    from vdmi.context import DeviceBoxes
    d = DeviceBoxes(b.n, b.cap, "cuda")
    for k in ("count", "xyxy", "xyxy_f", "score", "label"):
        getattr(d, k).copy_(torch.from_numpy(getattr(b, k)))
    torch.cuda.synchronize()                            # the context reads them on its own stream
    return d


MERGE_CASES = ["repeated_scores", "identical_box", "iou_pair", "all_empty", "one_empty", "spill"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", MERGE_CASES)
def test_tiles_merge_equals_reference(face_ctx_factory, case, device):
    ctx = face_ctx_factory(**NET, **TILED)
    h, w, n, T = 720, 1280, 2, 5
    rects = ctx.tile_rects(h, w)
    tw, th = int(rects[1, 2]), int(rects[1, 3])
    rng = np.random.default_rng(MERGE_CASES.index(case))
    if case == "repeated_scores":
        lists = _random_lists(rng, n, T, 96, tw, th, lambda r: int(rng.integers(0, 97)),
                              scores=np.asarray([0.5, 0.625, 0.75, 0.9], np.float32))
    elif case == "identical_box":                           # one face seen by the frame and by three tiles
        lists = _random_lists(rng, n, T, 8, tw, th, lambda r: 3)
        for f in range(n):
            for t in (0, 1, 2, 4):
                x0, y0 = rects[t, 0], rects[t, 1]
                lists.xyxy_f[f * T + t, 1] = [700 - x0, 350 - y0, 760 - x0, 420 - y0]
                lists.score[f * T + t, 1] = 0.9990234375
    elif case == "iou_pair":                                # IoU 0.4 (float32 quotient > 0.4) and 0.25, across inputs
        lists = _random_lists(rng, n, T, 4, tw, th, lambda r: 0)
        lists.count[[0, 1, 5, 6]] = 1
        lists.xyxy_f[0, 0], lists.xyxy_f[1, 0] = [0, 0, 10, 10], [0, 0, 10, 4]
        lists.xyxy_f[5, 0], lists.xyxy_f[6, 0] = [0, 0, 10, 10], [0, 0, 10, 2.5]
        lists.score[[0, 5], 0], lists.score[[1, 6], 0] = 0.9, 0.8
    elif case == "all_empty":
        lists = _random_lists(rng, n, T, 4, tw, th, lambda r: 0)
    elif case == "one_empty":
        lists = _random_lists(rng, n, T, 32, tw, th, lambda r: 0 if r % T == 2 else 20)
    else:                                                   # frame 0: 5 * 520 = 2600 boxes > the 2048 held in LDS
        lists = _random_lists(rng, n, T, 520, tw, th, lambda r: 520 if r < T else 30,
                              scores=np.linspace(0.5, 1, 300).astype(np.float32))
    ref = tr.merge(lists, n, rects, A640, 0.4)
    got = ctx.tiles_merge(_device(lists) if device else lists, h, w)
    _assert_lists_equal(got, ref, n)
    if case == "iou_pair":
        assert [len(r[0]) for r in ref] == [1, 2]
    if case == "identical_box":
        assert all((0, 1) in r[4] and not any(s in r[4] for s in ((1, 1), (2, 1), (4, 1))) for r in ref)
    if case == "spill":
        assert int(lists.count[:T].sum()) > 2048 and len(ref[0][0]) > 64
        # an output cap smaller than the merged count: count complete, arrays cut at cap
        from vdmi import _lib
        small = ctx.tiles_merge(lists, h, w, out=_lib.HostBoxes(n, 64))
        for f in range(n):
            assert int(small.count[f]) == len(ref[f][0])
            k = min(64, len(ref[f][0]))
            assert np.array_equal(small.xyxy[f, :k], ref[f][0][:k])
            assert np.array_equal(_bits(small.xyxy_f[f, :k]), _bits(ref[f][1][:k]))
            assert np.array_equal(small.label[f, :k], ref[f][3][:k])


def test_tiles_merge_label_optional_and_capacity(face_ctx_factory):
    from vdmi import _lib
    ctx = face_ctx_factory(**NET, **TILED)
    rng = np.random.default_rng(11)
    lists = _random_lists(rng, 1, 5, 8, 700, 400, lambda r: 4)
    s = lists.struct()
    s.label = None
    out = _lib.HostBoxes(1, 32)
    _lib.check(ctx._lib.vd_tiles_merge(ctx._h, ctypes.byref(s), 1, 720, 1280, ctypes.byref(out.struct())))
    lists.label[:] = 0
    _assert_lists_equal(out, tr.merge(lists, 1, ctx.tile_rects(720, 1280), A640, 0.4), 1)
    lists.count[3] = 9                                      # a host list the caller does not hold
    with pytest.raises(_lib.VdCapacityError):
        ctx.tiles_merge(lists, 720, 1280)


# ---- 3. end to end -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def e2e(face_ctx_factory):
    """2 frames of 360 x 640 through the tiled context, and the reference merge of the untiled
    context's detections of the 5 rectangles of each frame."""
    from vdmi import _lib
    frames = _frames(2)
    tiled = face_ctx_factory(**NET, **TILED)
    plain = face_ctx_factory(**NET)
    rects = tiled.tile_rects(H, W)
    T = len(rects)
    per = []
    for f in range(2):
        for (x0, y0, tw, th) in rects.tolist():
            per.append(plain.detect(np.ascontiguousarray(frames[f, y0:y0 + th, x0:x0 + tw])[None]))
    lists = _lib.HostBoxes(2 * T, max(1, max(int(b.count[0]) for b in per)))
    for r, b in enumerate(per):
        k = int(b.count[0])
        lists.count[r] = k
        for name in ("xyxy", "xyxy_f", "score", "label"):
            getattr(lists, name)[r, :k] = getattr(b, name)[0, :k]
    return frames, tiled, plain, rects, lists, tr.merge(lists, 2, rects, A640, 0.4)


def test_detect_equals_reference_merge_of_crop_detections(e2e):
    frames, tiled, plain, rects, lists, ref = e2e
    got = tiled.detect(frames)
    _assert_lists_equal(got, ref, 2)
    # the inputs show something: kept boxes from the whole frame and from tiles, and boxes the
    # cross-input NMS removed
    src = [s for r in ref for s in r[4]]
    assert any(t == 0 for t, _ in src) and any(t > 0 for t, _ in src)
    assert sum(len(r[0]) for r in ref) < int(lists.count.sum())
    # the per-input lists left in the library are untouched by the merge: read_boxes is the merged rows
    rb = tiled.read_boxes(0, 2)
    _assert_lists_equal(rb, ref, 2)


# ---- 4. process --------------------------------------------------------------------------------

def test_process_mosaic_and_gaussian_blur_the_merged_lists(face_ctx_factory, e2e):
    frames, tiled, plain, rects, lists, ref = e2e
    out, faces, _ = tiled.process(frames)
    rb = tiled.read_boxes(0, 2)
    _assert_lists_equal(rb, ref, 2)
    assert np.array_equal(faces.count, rb.count)
    assert np.array_equal(out, tiled.mosaic(frames, rb))
    f0 = [tuple(int(v) for v in b) for b in ref[0][0]]
    assert np.array_equal(out[0], omosaic.mosaic_frame(frames[0], f0, 8))
    g = face_ctx_factory(**NET, **TILED, blur="gaussian", blur_ksize=9)
    out, faces, _ = g.process(frames)
    rb = g.read_boxes(0, 2)
    _assert_lists_equal(rb, ref, 2)
    assert np.array_equal(out, g.blur(frames, rb))


def test_hold_runs_on_the_merged_lists(face_ctx_factory):
    """hold = 2 over two calls: read_held equals tests/hold_ref.py applied to the merged lists."""
    K, P = 2, 30
    ctx = face_ctx_factory(precision="fp32", max_batch=10, **TILED, hold=K)
    ctx.hold_reset()
    fr = _frames(3)
    seq = [fr[0], fr[1], fr[2], fr[0]]
    D, Hs, ages = [], [], []
    for lo in (0, 2):
        _, faces, _ = ctx.process(np.stack(seq[lo:lo + 2]))
        held = ctx.read_held(2)
        for b in range(2):
            D.append([tuple(int(v) for v in r) for r in _rows(faces, b)[0]])
            k = int(held.count[b])
            Hs.append([tuple(int(v) for v in r) for r in held.xyxy[b, :k]])
            ages.append([int(v) for v in held.label[b, :k]])
    _, Hr, ar, _ = hr.hold_lists(D, H, W, K, P)
    assert Hs == Hr and ages == ar
    assert sum(len(d) for d in D) > 0


# ---- 5. tiling off, and the Python split -----------------------------------------------------

def test_tiles_1x1_is_the_untiled_context(face_ctx_factory):
    frames = _frames(2)
    off = face_ctx_factory(**NET, tiles=(1, 1))
    plain = face_ctx_factory(**NET)
    a, b = off.detect(frames), plain.detect(frames)
    assert np.array_equal(a.count, b.count) and int(a.count.sum()) > 0
    for f in range(2):                                  # entries past a frame's count are not defined
        for x, y in zip(_rows(a, f), _rows(b, f)):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y), f
    oa, fa, _ = off.process(frames)
    ob, fb, _ = plain.process(frames)
    assert np.array_equal(oa, ob) and np.array_equal(fa.count, fb.count)
    for f in range(2):
        assert np.array_equal(_rows(fa, f)[0], _rows(fb, f)[0])
    assert off.frames_per_call() == 10


def test_python_split_of_a_long_batch(face_ctx_factory):
    """max_batch 10, T = 5: a call carries 2 frames; detect / process of 5 frames equal the
    sub-batches passed by hand."""
    import torch
    from vdmi.context import DeviceBoxes
    ctx = face_ctx_factory(**NET, **TILED)
    assert ctx.frames_per_call() == 2
    frames = _frames(5)
    whole = ctx.detect(frames)
    parts = [ctx.detect(frames[s:s + 2]) for s in (0, 2, 4)]
    r = 0
    for p in parts:
        for i in range(p.n):
            for x, y in zip(_rows(whole, r), _rows(p, i)):
                assert np.array_equal(x, y)
            r += 1
    assert r == 5
    dev = DeviceBoxes(5, 64, "cuda")
    dframes = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    out, faces, _ = ctx.process(dframes, faces=dev)
    ctx.sync()                                          # device outputs are queued on the context stream
    assert faces is dev and np.array_equal(dev.count.cpu().numpy(), whole.count)
    k = min(64, int(whole.count[4]))
    assert np.array_equal(dev.xyxy[4, :k].cpu().numpy(), whole.xyxy[4, :k])
    ph, _, _ = ctx.process(frames[4:5])
    assert np.array_equal(out[4].cpu().numpy(), ph[0])


# ---- 6. errors ---------------------------------------------------------------------------------

def test_refusals(face_ctx_factory):
    from vdmi import _lib
    import vdmi
    ctx = face_ctx_factory(**NET, **TILED)
    frames = _frames(3)
    out = _lib.HostBoxes(3, 16)
    rc = ctx._lib.vd_detect(ctx._h, frames.ctypes.data, 3, H, W, W * 3, _lib.VD_HOST, ctypes.byref(out.struct()))
    assert rc == _lib.VD_ERR_ARG and "largest n: 2" in _lib.last_error()
    assert ctx._lib.vd_tiles(ctx._h, 5, 1, 20) == _lib.VD_ERR_ARG
    assert ctx._lib.vd_tiles(ctx._h, 2, 2, 51) == _lib.VD_ERR_ARG
    assert ctx.letterbox_tiles(frames[:1]).shape[0] == 5          # the setting is unchanged
    with pytest.raises(ValueError):
        vdmi.Context(precision="fp32", max_batch=1, tiles=(5, 1))
    with pytest.raises(ValueError):
        vdmi.Context(precision="fp32", max_batch=1, tiles=(2, 2), tile_overlap=51)
    plain = face_ctx_factory(**NET)
    lists = _lib.HostBoxes(5, 4)
    rc = plain._lib.vd_tiles_merge(plain._h, ctypes.byref(lists.struct()), 1, H, W, None)
    assert rc == _lib.VD_ERR_STATE and "tiling is off" in _lib.last_error()
    with pytest.raises(_lib.VdError, match="tiling is off"):
        plain.letterbox_tiles(frames[:1])
