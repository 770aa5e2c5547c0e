"""Box hold on the GPU (csrc/hold.hip through vd_hold, vd_process and the pipeline), exact
against the definition in tests/hold_ref.py: lists, ages, history across calls, and the
pixels of the frames blurred with B_t = D_t ++ H_t."""
import io
import os

import numpy as np
import pytest

import gaussian_ref as gr
import hold_ref as hr
from oracle import mosaic as omosaic

pytestmark = pytest.mark.gpu

LDS_BOXES = 2048       # csrc/hold.hip: clipped reference boxes (frames t .. t-K+1) the kernel keeps in LDS

_CTX = {}


@pytest.fixture(scope="module")
def hold_ctx(gpu):
    """Weight-less hold contexts by (K, P): vd_hold needs no network."""
    import vdmi

    def make(K, P=30):
        if (K, P) not in _CTX:
            _CTX[(K, P)] = vdmi.Context(precision="fp32", max_batch=4, hold=K, hold_iou_pct=P)
        _CTX[(K, P)].hold_reset()
        return _CTX[(K, P)]

    yield make
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _host_boxes(seq, cap=None):
    from vdmi import _lib
    hb = _lib.HostBoxes(len(seq), cap or max(1, max(len(d) for d in seq)))
    for i, d in enumerate(seq):
        hb.count[i] = len(d)
        if len(d):
            hb.xyxy[i, :len(d)] = np.asarray(d, np.int32).reshape(-1, 4)
    return hb


def _device_boxes(seq):
    import torch
    from vdmi.context import DeviceBoxes
    hb = _host_boxes(seq)
    db = DeviceBoxes(hb.n, hb.cap, "cuda:0")
    db.count.copy_(torch.from_numpy(hb.count))
    db.xyxy.copy_(torch.from_numpy(hb.xyxy))
    torch.cuda.synchronize()
    return db


def _rows(boxes, i):
    k = int(boxes.count[i])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[i, :k]], [int(v) for v in boxes.label[i, :k]]


def _step(ctx, seq, h, w, K, P, history, device=False):
    """One vd_hold call over seq, checked against the reference continued from `history`:
    B_t with label = age through `out`, H_t through read_held. Returns the reference."""
    from vdmi import _lib
    B, H, ages, hist = hr.hold_lists(seq, h, w, K, P, history)
    out = _lib.HostBoxes(len(seq), max(1, max(len(b) for b in B)))
    ctx.hold(_device_boxes(seq) if device else _host_boxes(seq), h, w, out=out)
    held = ctx.read_held(len(seq))
    for i in range(len(seq)):
        got, lab = _rows(out, i)
        assert got == B[i], (i, got, B[i])
        assert lab == [0] * (len(B[i]) - len(H[i])) + ages[i], i
        got_h, lab_h = _rows(held, i)
        assert got_h == H[i] and lab_h == ages[i], i
    return B, H, ages, hist


A, FAR = (10, 10, 30, 30), (60, 60, 90, 95)
EMPTIES = [(200, 200, 240, 230), (60, 30, 60, 50), (-50, -50, -10, -10)]
CRAFTED = {   # name: (sequence, K, P, expected H per frame) on a 100 x 100 frame (tests/test_hold_ref.py)
    "gap_fill": ([[A], [], [], []], 2, 30, [[], [A], [A], []]),
    "chain": ([[A], [A], []], 2, 30, [[], [], [A]]),
    "two_back": ([[A], [FAR], []], 2, 30, [[], [A], [FAR, A]]),
    "inclusive_match": ([[(0, 0, 10, 10)], [(0, 0, 10, 3)]], 1, 30, [[], []]),
    "just_below": ([[(0, 0, 10, 10)], [(0, 0, 9, 3)]], 1, 30, [[], [(0, 0, 10, 10)]]),
    "empties_never_held": ([EMPTIES, []], 2, 30, [[], []]),
    "empties_never_match": ([[(50, 20, 70, 60)], EMPTIES], 1, 30, [[], [(50, 20, 70, 60)]]),
    "held_unclipped": ([[(-5, -5, 10, 10)], []], 1, 30, [[], [(-5, -5, 10, 10)]]),
    "p100_identical_clipped": ([[(-5, -5, 10, 10)], [(0, 0, 10, 10)]], 1, 100, [[], []]),
    "p100_differs": ([[(0, 0, 10, 10)], [(0, 0, 10, 9)]], 1, 100, [[], [(0, 0, 10, 10)]]),
    "p1_match": ([[(0, 0, 10, 10)], [(9, 0, 19, 10)]], 1, 1, [[], []]),
    "p1_touching": ([[(0, 0, 10, 10)], [(10, 0, 20, 10)]], 1, 1, [[], [(0, 0, 10, 10)]]),
    "both_overlapping_held": ([[(10, 10, 30, 30), (12, 12, 32, 32)], []], 1, 30,
                              [[], [(10, 10, 30, 30), (12, 12, 32, 32)]]),
    "age_then_list_order": ([[(20, 0, 30, 10), (0, 0, 10, 10)], [(60, 0, 70, 10), (40, 0, 50, 10)], [FAR]], 2, 30,
                            [[], [(20, 0, 30, 10), (0, 0, 10, 10)],
                             [(60, 0, 70, 10), (40, 0, 50, 10), (20, 0, 30, 10), (0, 0, 10, 10)]]),
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_vd_hold_known_answers(hold_ctx, name):
    seq, K, P, want = CRAFTED[name]
    _, H, _, _ = _step(hold_ctx(K, P), seq, 100, 100, K, P, None)
    assert H == want


def _random_sequence(seed, frames=12, h=120, w=160, most=40):
    """0..most boxes per frame with coordinates in [-20, 180] (clipped, degenerate and outside
    boxes among them); half of each frame's boxes are copies of the previous frame's, most of
    them jittered by up to 6 pixels."""
    rng = np.random.default_rng(seed)
    seq, prev = [], []
    for _ in range(frames):
        k = int(rng.integers(0, most + 1))
        cur = []
        for _ in range(k):
            if prev and rng.random() < 0.5:
                b = np.asarray(prev[int(rng.integers(len(prev)))])
                if rng.random() < 0.75:                  # the rest are exact copies: matches at P = 100
                    b = b + rng.integers(-6, 7, 4)
            else:
                x1, y1 = rng.integers(-20, 181, 2)
                b = np.asarray([x1, y1, x1 + rng.integers(-5, 60), y1 + rng.integers(-5, 60)])
            cur.append(tuple(int(v) for v in np.clip(b, -20, 180)))
        seq.append(cur)
        prev = cur
    return seq, h, w


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("P", [1, 30, 100])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_random_sequences(hold_ctx, K, P, device):
    seq, h, w = _random_sequence(100 * K + P)
    _, H, ages, _ = _step(hold_ctx(K, P), seq, h, w, K, P, None, device=device)
    held1 = sum(a.count(1) for a in ages)
    cands1 = sum(1 for d in seq[:-1] for b in d if hr.clip_box(b, h, w))
    assert held1 > 0 and cands1 - held1 > 0          # both outcomes: held, and matched away
    assert any(hr.clip_box(b, h, w) is None for d in seq for b in d)


def test_call_split_invariance_reset_and_size_change(hold_ctx):
    """12 frames as one call, as 5 + 7 and as twelve calls of one frame (K = 3: the history
    shifts with n < K) give the same B_t; hold_reset and another frame size clear it."""
    K, P = 3, 30
    seq, h, w = _random_sequence(7)
    ctx = hold_ctx(K, P)
    one = _step(ctx, seq, h, w, K, P, None)
    for cuts in ((5, 12), tuple(range(1, 13))):
        ctx.hold_reset()
        hist, B, lo = None, [], 0
        for hi in cuts:
            b, _, _, hist = _step(ctx, seq[lo:hi], h, w, K, P, hist)
            B += b
            lo = hi
        assert B == one[0], cuts
    assert sum(len(x) for x in one[1]) > 0
    # the history is still the sequence's tail: frame 0 of a new stream holds nothing after a reset
    ctx.hold_reset()
    _, H, _, hist = _step(ctx, [[]], h, w, K, P, None)
    assert H == [[]]
    _, H, _, hist = _step(ctx, seq[:2], h, w, K, P, hist)
    assert sum(len(x) for x in H) > 0
    # another (h, w): the old history is gone, without a reset
    _, H, _, hist = _step(ctx, [[]], h + 8, w, K, P, None)
    assert H == [[]]
    _, H, _, _ = _step(ctx, [[]], h, w, K, P, None)   # ... and back: cleared again
    assert H == [[]]


def test_global_memory_path_and_cap_overflow(hold_ctx):
    """600 boxes per frame at K = 8 on 4 frames: frame 3 compares against 2400 clipped boxes,
    more than the LDS_BOXES the kernel keeps in LDS, so it reads them from global memory;
    frames 0..2 (600 / 1200 / 1800) take the LDS path. Then a caller cap smaller than B_t."""
    from vdmi import _lib
    K, P = 8, 30
    rng = np.random.default_rng(3)
    seq = []
    for t in range(4):
        xy = rng.integers(0, 1800, (600, 2))
        wh = rng.integers(4, 40, (600, 2))
        seq.append([tuple(int(v) for v in (x, y, x + a, y + b)) for (x, y), (a, b) in zip(xy, wh)])
    assert 3 * 600 <= LDS_BOXES < 4 * 600
    ctx = hold_ctx(K, P)
    B, H, ages, hist = _step(ctx, seq, 1080, 1920, K, P, None, device=True)
    assert len(H[3]) > 0 and sum(1 for d in seq[:3] for _ in d) - len(H[3]) > 0
    # the next frame's B_t exceeds the caller's cap: count complete, arrays the first cap entries
    nxt = [seq[0][:5]]
    Bn, _, agn, _ = hr.hold_lists(nxt, 1080, 1920, K, P, hist)
    cap = 100
    assert len(Bn[0]) > cap
    out = _lib.HostBoxes(1, cap)
    ctx.hold(_host_boxes(nxt), 1080, 1920, out=out)
    assert int(out.count[0]) == len(Bn[0])
    assert [tuple(int(v) for v in r) for r in out.xyxy[0]] == Bn[0][:cap]
    assert [int(v) for v in out.label[0]] == ([0] * 5 + agn[0])[:cap]
    # Context.hold without a target sizes the lists itself
    ctx.hold_reset()
    auto = ctx.hold(seq[:2], 1080, 1920)
    assert _rows(auto, 1)[0] == B[1] and int(auto.count[0]) == 600


def test_refusals(gpu, hold_ctx):
    import vdmi
    from vdmi import _lib
    off = vdmi.Context(precision="fp32", max_batch=2)
    try:
        with pytest.raises(_lib.VdError) as e:
            off.hold([[A]], 100, 100)
        assert e.value.code == _lib.VD_ERR_STATE
        with pytest.raises(_lib.VdError) as e:
            off.read_held(1)
        assert e.value.code == _lib.VD_ERR_STATE
        off.hold_reset()                     # harmless without hold
    finally:
        off.close()
    ctx = hold_ctx(2)
    hb = _lib.HostBoxes(1, 2)
    hb.count[0] = 3
    with pytest.raises(_lib.VdCapacityError) as e:
        ctx.hold(hb, 100, 100, out=_lib.HostBoxes(1, 8))
    assert e.value.code == _lib.VD_ERR_CAPACITY
    cfg = _lib.default_cfg()
    for frames, pct in ((9, 0), (-1, 0), (1, 101), (1, -1)):
        cfg.hold_frames, cfg.hold_iou_pct = frames, pct
        import ctypes
        h = ctypes.c_void_p()
        assert _lib.load().vd_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib.VD_ERR_ARG


# ---- end to end through vd_process -------------------------------------------------------

def _frame(i):
    from vdmi import synth
    return np.repeat(np.repeat(synth.frame(180, 320, i, seed=5), 2, 0), 2, 1)     # 360x640, faces fire


_NETS = {}


@pytest.fixture(scope="module")
def net_ctx(gpu):
    """fp32 contexts with seeded RetinaFace + YOLO weights by (hold, blur)."""
    import vdmi
    from vdmi import weights

    def make(hold, blur="pixelate"):
        if (hold, blur) not in _NETS:
            kw = dict(blur="gaussian", blur_ksize=9) if blur == "gaussian" else {}
            c = vdmi.Context(precision="fp32", max_batch=4, hold=hold, **kw)
            c.load_weights(0, weights.retinaface_state_dict(0))
            c.load_weights(1, weights.yolov8n_state_dict(0))
            _NETS[(hold, blur)] = c
        _NETS[(hold, blur)].hold_reset()
        return _NETS[(hold, blur)]

    yield make
    for c in _NETS.values():
        c.close()
    _NETS.clear()


def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _process_sequence(ctx, frames, calls, K):
    """frames through ctx.process in `calls` (faces | plates | mosaic of both): per frame
    (output, D_t), and read_held's (H_t, ages) of every call."""
    from vdmi import _lib
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES
    outs, D, H, ages = [], [], [], []
    lo = 0
    for n in calls:
        out, faces, plates = ctx.process(np.stack(frames[lo:lo + n]), flags=flags)
        held = ctx.read_held(n) if K else None
        for b in range(n):
            outs.append(out[b])
            D.append(_lists(faces, b) + _lists(plates, b))
            if K:
                rows, lab = _rows(held, b)
                H.append(rows)
                ages.append(lab)
        lo += n
    return outs, D, H, ages


@pytest.fixture(scope="module")
def clip_frames():
    a, b, c = _frame(0), _frame(1), _frame(2)
    return [a, a, b, b, c, a]


def test_process_holds_boxes_across_calls(net_ctx, clip_frames):
    """[A, A, B, B, C, A] as calls of 4 + 2 in a hold=2 context: read_held equals the
    reference over the returned lists, every output frame is the oracle mosaic of B_t, a
    repeated frame holds nothing from its twin, and something is held."""
    K, P = 2, 30
    outs, D, H, ages = _process_sequence(net_ctx(K), clip_frames, (4, 2), K)
    B, Hr, ar, _ = hr.hold_lists(D, 360, 640, K, P)
    assert H == Hr and ages == ar
    for t, fr in enumerate(clip_frames):
        np.testing.assert_array_equal(outs[t], omosaic.mosaic_frame(fr, B[t], 8), err_msg=f"frame {t}")
    assert sum(len(d) for d in D) > 0
    assert 1 not in ages[1] and 1 not in ages[3]        # A after A, B after B
    assert sum(len(h) for h in H) > 0
    # the same frames without hold: the same detections, pixels of D_t alone
    outs0, D0, _, _ = _process_sequence(net_ctx(0), clip_frames, (4, 2), 0)
    assert D0 == D
    for t, fr in enumerate(clip_frames):
        np.testing.assert_array_equal(outs0[t], omosaic.mosaic_frame(fr, D[t], 8), err_msg=f"frame {t}")
    assert any(not np.array_equal(x, y) for x, y in zip(outs, outs0))


def test_process_holds_boxes_gaussian(net_ctx, clip_frames):
    from vdmi import _lib
    K, P = 2, 30
    frames = clip_frames[1:5]                            # A, B, B, C
    outs, D, H, ages = _process_sequence(net_ctx(K, "gaussian"), frames, (4,), K)
    B, Hr, ar, _ = hr.hold_lists(D, 360, 640, K, P)
    assert H == Hr and ages == ar and sum(len(h) for h in H) > 0
    q = _lib.blur_weights(9, 0.0)
    for t, fr in enumerate(frames):
        np.testing.assert_array_equal(outs[t], gr.blur_frame(fr, B[t], 9, 0.0, q=q), err_msg=f"frame {t}")


def test_process_without_mosaic_updates_the_history(net_ctx, clip_frames):
    """A call without VD_PROC_MOSAIC still feeds the history (how a shard warms up)."""
    from vdmi import _lib
    K, P = 2, 30
    ctx = net_ctx(K)
    det = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC_PLATES
    _, f0, p0 = ctx.process(np.stack(clip_frames[1:3]), flags=det)          # A, B: detect only
    D01 = [_lists(f0, b) + _lists(p0, b) for b in range(2)]
    outs, D, H, ages = _process_sequence(ctx, clip_frames[4:5], (1,), K)    # C
    _, Hr, ar, _ = hr.hold_lists(D, 360, 640, K, P, history=D01)
    assert H == Hr and ages == ar and len(H[0]) > 0


# ---- pipeline ---------------------------------------------------------------------------------

N = 9


def _jpeg_dir(d):
    from PIL import Image
    d.mkdir(exist_ok=True)
    src = {}
    for i in range(N):
        b = io.BytesIO()
        Image.fromarray(_frame(i)).save(b, "JPEG", quality=95)
        (d / f"f{i:03d}.jpg").write_bytes(b.getvalue())
        src[f"f{i:03d}.jpg"] = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
    return src


def _detectors(device_ids, hold):
    import vdmi
    from vdmi import weights
    face = vdmi.Retinaface(input_shape=[640, 640, 3], nms_iou=0.4, max_batch=4, device_ids=device_ids,
                           weights=weights.retinaface_state_dict(0), hold=hold)
    plate = vdmi.YOLO(weights="random", max_batch=4, device_ids=device_ids)
    return face, plate


def _record_lists(rec, name):
    out = []
    for key in ("faces", "plates"):
        v = rec[name][key]
        if v is not None:
            assert int(v[3]) <= len(v[0])                # the record carries every box of the frame
            out += [tuple(int(x) for x in b) for b in v[0][:int(v[3])]]
    return out


@pytest.mark.parametrize("codec", [True, False], ids=["gpu_codec", "host_frames"])
def test_batch_process_images_hold(gpu, tmp_path, codec):
    """batch_process_images(hold=2, batch_size=4) over 9 JPEG frames: the written frames equal
    the oracle mosaic of B_t built from the recorded boxes over the sorted names; two device
    shards (warm-up before the second) and a second run on the same detectors (reset at the
    start, cached contexts) write the same files."""
    from PIL import Image
    from vdmi.pipeline import batch_process_images
    K, P = 2, 30
    src = _jpeg_dir(tmp_path / "in")
    frames = src if codec else {f"f{i:03d}.jpg": _frame(i) for i in range(N)}
    kw = {} if codec else {"loader": lambda p: frames[os.path.basename(p)]}
    dets = {"one": _detectors([0], K), "two": _detectors([0, 0], K)}
    runs = {}
    for name, det, shard in (("one", "one", None), ("two", "two", "devices"), ("one_again", "one", None)):
        saved, rec = {}, {}
        if not codec:
            kw["saver"] = lambda img, p, saved=saved: saved.__setitem__(os.path.basename(p), img.copy())
        out = tmp_path / name
        tot = batch_process_images(str(tmp_path / "in"), str(out), *dets[det], batch_size=4, shard=shard,
                                   records=rec, mosaic_plates=True, hold=K, hold_iou_pct=P, **kw)
        files = {f: (out / f).read_bytes() for f in sorted(os.listdir(out))} if codec else saved
        runs[name] = (tot, rec, files)
    tot, rec, files = runs["one"]
    names = sorted(frames)
    assert tot[0] == N and tot[1] > 0 and sorted(rec) == names
    D = [_record_lists(rec, n) for n in names]
    assert tot[1] + tot[2] == sum(len(d) for d in D)     # totals and records: the detections only
    B, H, _, _ = hr.hold_lists(D, 360, 640, K, P)
    assert sum(len(h) for h in H) > 0
    for t, n in enumerate(names):
        exp = omosaic.mosaic_frame(frames[n], B[t], 8)
        if codec:
            b = io.BytesIO()
            Image.fromarray(exp).save(b, "JPEG", quality=95, subsampling=2)
            assert files[f"processed_{n}"] == b.getvalue(), n
        else:
            np.testing.assert_array_equal(files[f"processed_{n}"], exp, err_msg=n)
    for other in ("two", "one_again"):
        t2, r2, f2 = runs[other]
        assert t2 == tot and r2 == rec and sorted(f2) == sorted(files), other
        for k in files:
            if codec:
                assert files[k] == f2[k], (other, k)
            else:
                np.testing.assert_array_equal(files[k], f2[k], err_msg=f"{other} {k}")


def test_batch_process_images_hold_needs_matching_detector(gpu, tmp_path):
    from vdmi.pipeline import batch_process_images
    (tmp_path / "in").mkdir()
    face, plate = _detectors([0], 0)
    with pytest.raises(ValueError, match="hold"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, hold=2)


def test_dropped_batch_resets_the_history(gpu, tmp_path):
    """A batch whose inference fails is dropped (combine_detect.py:226-228); the batch after it
    must not hold boxes from before the gap: its frames are blurred with their own boxes only."""
    from vdmi.pipeline import batch_process_images, fused_context
    K, P = 2, 30
    frames = {f"f{i:03d}.jpg": _frame(i) for i in range(N)}
    (tmp_path / "in").mkdir()
    for n in frames:
        (tmp_path / "in" / n).write_bytes(b"")
    face, plate = _detectors([0], K)
    ctx = fused_context(face, plate, 4)
    real, calls = ctx.process, []

    def flaky(*a, **k):
        calls.append(1)
        if len(calls) == 2:                              # the second batch: frames 4..7
            raise RuntimeError("inference failure")
        return real(*a, **k)

    ctx.process = flaky
    saved, rec = {}, {}
    tot = batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, batch_size=4, shard=None,
                               records=rec, mosaic_plates=True, hold=K, hold_iou_pct=P,
                               loader=lambda p: frames[os.path.basename(p)],
                               saver=lambda img, p: saved.__setitem__(os.path.basename(p), img.copy()))
    kept = [f"f{i:03d}.jpg" for i in (0, 1, 2, 3, 8)]
    assert tot[0] == 5 and sorted(saved) == [f"processed_{n}" for n in kept] and len(calls) == 3
    D = [_record_lists(rec, n) for n in kept]
    np.testing.assert_array_equal(saved["processed_f008.jpg"], omosaic.mosaic_frame(frames["f008.jpg"], D[4], 8))
    # without the reset frame 8 would have held boxes of frames 2 and 3
    assert len(hr.hold_lists(D, 360, 640, K, P)[1][4]) > 0
