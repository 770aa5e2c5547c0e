"""Box hold with the linear motion model on the GPU (csrc/hold.hip in motion mode through
vd_hold, vd_process and the pipeline), exact against the definition in
tests/hold_motion_ref.py: moved boxes, ages, the K + 1 deep history across calls, the resets,
and the pixels of the frames blurred with B_t = D_t ++ H_t."""
import os

import numpy as np
import pytest

import gaussian_ref as gr
import hold_motion_ref as mr
import hold_ref as hr
from oracle import mosaic as omosaic
from test_gpu_hold import (LDS_BOXES, _device_boxes, _host_boxes, _lists, _process_sequence, _random_sequence,
                           _record_lists, _rows)

pytestmark = pytest.mark.gpu

_CTX = {}


@pytest.fixture(scope="module")
def motion_ctx(gpu):
    """Weight-less hold contexts in motion mode by (K, P): vd_hold needs no network."""
    import vdmi

    def make(K, P=30):
        if (K, P) not in _CTX:
            _CTX[(K, P)] = vdmi.Context(precision="fp32", max_batch=4, hold=K, hold_iou_pct=P, hold_motion=True)
        c = _CTX[(K, P)]
        c.set_hold_motion(True)
        c.hold_reset()
        return c

    yield make
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _step(ctx, seq, h, w, K, P, history, device=False, motion=True):
    """One vd_hold call over seq, checked against the reference continued from `history`:
    B_t with label = age through `out`, H_t through read_held. Returns the reference."""
    from vdmi import _lib
    if motion:
        B, H, ages, hist, stored = mr.hold_motion_lists(seq, h, w, K, P, history)
    else:
        B, H, ages, hist = hr.hold_lists(seq, h, w, K, P, history)
        stored = H
    out = _lib.HostBoxes(len(seq), max(1, max(len(b) for b in B)))
    ctx.hold(_device_boxes(seq) if device else _host_boxes(seq), h, w, out=out)
    held = ctx.read_held(len(seq))
    for i in range(len(seq)):
        got, lab = _rows(out, i)
        assert got == B[i], (i, got, B[i])
        assert lab == [0] * (len(B[i]) - len(H[i])) + ages[i], i
        got_h, lab_h = _rows(held, i)
        assert got_h == H[i] and lab_h == ages[i], i
    return B, H, ages, hist, stored


def _moved(H, stored):
    return sum(m != s for hm, hs in zip(H, stored) for m, s in zip(hm, hs))


C, LEFT, RIGHT = (10, 10, 30, 30), (8, 10, 28, 30), (12, 10, 32, 30)
CRAFTED = {   # name: (sequence, K, P, expected H per frame) on a 100 x 100 frame (tests/test_hold_motion_ref.py)
    "moving": ([[(10, 10, 30, 30)], [(14, 10, 34, 30)], [], []], 2, 30,
               [[], [], [(14, 10, 38, 30)], [(14, 10, 42, 30)]]),
    "shrinking": ([[(10, 10, 30, 30)], [(16, 10, 24, 30)], [], []], 2, 30,
                  [[], [], [(16, 10, 24, 30)], [(16, 10, 24, 30)]]),
    "leaving": ([[(2, 40, 22, 60)], [(-4, 40, 16, 60)], [], []], 2, 30,
                [[], [], [(-4, 40, 16, 60)], [(-4, 40, 16, 60)]]),
    "tie_lowest_index": ([[RIGHT, LEFT], [C], []], 1, 30, [[], [], [(8, 10, 30, 30)]]),
    "tie_lowest_index_swapped": ([[LEFT, RIGHT], [C], []], 1, 30, [[], [], [(10, 10, 32, 30)]]),
    "best_iou_not_first": ([[(4, 10, 24, 30), (9, 10, 29, 30)], [C], []], 1, 30, [[], [], [(10, 10, 31, 30)]]),
    "no_predecessor_at_start": ([[C], [], []], 2, 30, [[], [C], [C]]),
    "no_predecessor_matches": ([[(60, 60, 90, 95)], [C], []], 1, 30, [[], [(60, 60, 90, 95)], [C]]),
    "p100_moves_nothing": ([[(-5, 10, 30, 30)], [(0, 10, 30, 30)], [(1, 10, 30, 30)], []], 2, 100,
                           [[], [], [(0, 10, 30, 30)], [(1, 10, 30, 30), (0, 10, 30, 30)]]),
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_vd_hold_known_answers(motion_ctx, name):
    seq, K, P, want = CRAFTED[name]
    _, H, _, _, _ = _step(motion_ctx(K, P), seq, 100, 100, K, P, None)
    assert H == want


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("P", [1, 30, 100])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_random_sequences(motion_ctx, K, P, device):
    seq, h, w = _random_sequence(100 * K + P)
    _, H, ages, _, stored = _step(motion_ctx(K, P), seq, h, w, K, P, None, device=device)
    if P == 100:
        assert _moved(H, stored) == 0 and sum(len(x) for x in H) > 0
    else:
        assert _moved(H, stored) >= 10               # the reference alone: no vacuous pass


def test_call_boundaries(motion_ctx):
    """K = 8, 12 frames: one call, twelve calls of one frame (an age-8 candidate's predecessor
    sits in the deepest history slot) and calls of 2, 5 and 5 frames (n < K + 1 shifts the
    history) give the same lists."""
    K, P = 8, 30
    seq, h, w = _random_sequence(100 * K + P)
    ctx = motion_ctx(K, P)
    one = _step(ctx, seq, h, w, K, P, None)
    assert _moved(one[1], one[4]) >= 10
    deep = [(m, s) for hm, hs, ag in zip(one[1], one[4], one[2]) for m, s, a in zip(hm, hs, ag) if a == K and m != s]
    assert deep                                      # boxes of age K moved by a predecessor of age K + 1
    for cuts in (tuple(range(1, 13)), (2, 7, 12)):
        ctx.hold_reset()
        hist, B, lo = None, [], 0
        for hi in cuts:
            b, _, _, hist, _ = _step(ctx, seq[lo:hi], h, w, K, P, hist)
            B += b
            lo = hi
        assert B == one[0], cuts
        assert len(hist) == K + 1


MOVE = [[(10, 10, 30, 30)], [(14, 10, 34, 30)], []]       # held at frame 2: (14, 10, 38, 30), or as stored
MOVED, STORED = (14, 10, 38, 30), (14, 10, 34, 30)


def _held_after(ctx, between, h2=100, w2=100):
    """D_0 in one call, `between`, then D_1 and an empty frame: the box held in the last frame."""
    ctx.hold(_host_boxes(MOVE[:1]), 100, 100)
    between()
    ctx.hold(_host_boxes(MOVE[1:]), h2, w2)
    rows, lab = _rows(ctx.read_held(2), 1)
    assert lab == [1]
    return rows[0]


def test_resets(gpu, motion_ctx):
    import vdmi
    from vdmi import _lib
    ctx = motion_ctx(2)
    assert _held_after(ctx, lambda: None) == MOVED
    ctx.hold_reset()
    assert _held_after(ctx, lambda: ctx.set_hold_motion(True)) == MOVED     # the same mode: the history stays
    assert ctx.hold_motion is True
    ctx.hold_reset()
    assert _held_after(ctx, ctx.hold_reset) == STORED                       # no predecessor left
    ctx.hold_reset()
    assert _held_after(ctx, lambda: None, h2=108) == STORED                 # another frame size
    ctx.hold_reset()

    def off_and_on():
        ctx.set_hold_motion(False)
        ctx.set_hold_motion(True)
    assert _held_after(ctx, off_and_on) == STORED                           # each change of mode forgets
    # a change of mode also forgets what plain hold would keep: nothing is held from before it
    ctx.hold_reset()
    ctx.hold(_host_boxes(MOVE[1:2]), 100, 100)
    ctx.set_hold_motion(False)
    assert ctx.hold_motion is False
    ctx.hold(_host_boxes([[]]), 100, 100)
    assert int(ctx.read_held(1).count[0]) == 0
    # mode off in the same context: plain hold, exact against hold_ref, across calls
    seq, h, w = _random_sequence(7)
    _, _, _, hist, _ = _step(ctx, seq[:5], h, w, 2, 30, None, motion=False)
    _step(ctx, seq[5:], h, w, 2, 30, hist, motion=False)
    ctx.set_hold_motion(True)
    _step(ctx, seq, h, w, 2, 30, None)
    # refusals
    lib = _lib.load()
    assert lib.vd_hold_motion(ctx.handle, 2) == _lib.VD_ERR_ARG
    assert lib.vd_hold_motion(ctx.handle, -1) == _lib.VD_ERR_ARG
    with pytest.raises(_lib.VdError) as e:
        ctx.hold(MOVE, 40000, 100)
    assert e.value.code == _lib.VD_ERR_ARG
    with pytest.raises(_lib.VdError) as e:
        ctx.hold(MOVE, 100, 32769)
    assert e.value.code == _lib.VD_ERR_ARG
    ctx.hold_reset()
    # the largest frame: inter * union near 2^60 in the best-IoU comparison
    _, H, _, _, _ = _step(ctx, [[(0, 0, 32768, 32768), (0, 1, 32768, 32768)], [(1, 1, 32768, 32768)], []],
                          32768, 32768, 2, 30, None)
    assert H[2] == [(1, 1, 32768, 32768)] and H[1] == []
    off = vdmi.Context(precision="fp32", max_batch=2)
    try:
        assert lib.vd_hold_motion(off.handle, 1) == _lib.VD_ERR_STATE
        assert lib.vd_hold_motion(off.handle, 0) == _lib.VD_OK
        with pytest.raises(_lib.VdError) as e:
            off.set_hold_motion(True)
        assert e.value.code == _lib.VD_ERR_STATE and off.hold_motion is False
    finally:
        off.close()


def test_global_memory_path(motion_ctx):
    """K = 2 on a 2000 x 2000 virtual frame: 1122 boxes on a grid that shifts by (3, 2) pixels
    per frame, every third box missing from frame 2 on. From frame 1 the clipped boxes of ages
    0..K number more than the LDS_BOXES the kernel stages, so every comparison and the
    predecessor search read global memory; frame 0 takes the LDS path."""
    K, P = 2, 30
    grid = [(20 + 58 * i, 15 + 58 * j) for j in range(33) for i in range(34)]
    seq = []
    for t in range(4):
        d = [(x + 3 * t, y + 2 * t, x + 3 * t + 40, y + 2 * t + 44) for x, y in grid]
        seq.append([b for k, b in enumerate(d) if t < 2 or k % 3])
    assert len(seq[0]) <= LDS_BOXES < len(seq[0]) + len(seq[1])
    B, H, ages, _, stored = _step(motion_ctx(K, P), seq, 2000, 2000, K, P, None, device=True)
    gone = len(grid) - len(seq[2])
    assert [len(x) for x in H] == [0, 0, gone, gone] and ages[3] == [2] * gone
    assert _moved(H, stored) == 2 * gone
    assert H[3][0] == (20 + 3, 15 + 2, 20 + 3 + 40 + 6, 15 + 2 + 44 + 4)    # q = c + 2 * (3, 2, 3, 2)


# ---- end to end through vd_process -------------------------------------------------------

def _small_frame(i):
    from vdmi import synth
    return np.repeat(np.repeat(synth.frame(60, 80, i, seed=5), 2, 0), 2, 1)       # 120 x 160


_NETS = {}


@pytest.fixture(scope="module")
def net_ctx(gpu):
    """fp32 hold=2 contexts in motion mode with seeded RetinaFace + YOLO weights by blur."""
    import vdmi
    from vdmi import weights

    def make(blur="pixelate"):
        if blur not in _NETS:
            kw = dict(blur="gaussian", blur_ksize=9) if blur == "gaussian" else {}
            c = vdmi.Context(precision="fp32", max_batch=4, hold=2, hold_motion=True, **kw)
            c.load_weights(0, weights.retinaface_state_dict(0))
            c.load_weights(1, weights.yolov8n_state_dict(0))
            _NETS[blur] = c
        _NETS[blur].hold_reset()
        return _NETS[blur]

    yield make
    for c in _NETS.values():
        c.close()
    _NETS.clear()


@pytest.mark.parametrize("blur", ["pixelate", "gaussian"])
def test_process_moves_held_boxes(net_ctx, blur):
    """4 frames of 120 x 160 as calls of 3 + 1 in a hold=2 motion context: read_held equals the
    reference over the returned detections, and every output frame is the oracle's blur of
    the reference's B_t."""
    from vdmi import _lib
    K, P = 2, 30
    frames = [_small_frame(i) for i in (0, 1, 2, 0)]
    outs, D, H, ages = _process_sequence(net_ctx(blur), frames, (3, 1), K)
    B, Hr, ar, _, stored = mr.hold_motion_lists(D, 120, 160, K, P)
    assert H == Hr and ages == ar
    assert sum(len(d) for d in D) > 0 and sum(len(h) for h in H) > 0
    assert _moved(H, stored) > 0                         # the pixels below cover a moved box
    q = _lib.blur_weights(9, 0.0)
    for t, fr in enumerate(frames):
        exp = omosaic.mosaic_frame(fr, B[t], 8) if blur == "pixelate" else gr.blur_frame(fr, B[t], 9, 0.0, q=q)
        np.testing.assert_array_equal(outs[t], exp, err_msg=f"frame {t}")


# ---- pipeline ---------------------------------------------------------------------------------

N = 7


def _detectors(device_ids):
    import vdmi
    from vdmi import weights
    face = vdmi.Retinaface(input_shape=[640, 640, 3], nms_iou=0.4, max_batch=4, device_ids=device_ids,
                           weights=weights.retinaface_state_dict(0), hold=2, hold_motion=True)
    plate = vdmi.YOLO(weights="random", max_batch=4, device_ids=device_ids)
    return face, plate


def test_batch_process_images_hold_motion(gpu, tmp_path):
    """batch_process_images(hold=2, hold_motion=True) over 7 small frames: two shards (the
    second warms up on the K + 1 frames before it) write what one context writes, and that is
    the oracle mosaic of the reference's B_t over the recorded boxes."""
    from vdmi.pipeline import batch_process_images
    K, P = 2, 30
    frames = {f"f{i:03d}.jpg": _small_frame(i) for i in range(N)}
    (tmp_path / "in").mkdir()
    for n in frames:
        (tmp_path / "in" / n).write_bytes(b"")
    runs = {}
    for name, ids, shard in (("one", [0], None), ("two", [0, 0], "devices")):
        saved, rec = {}, {}
        tot = batch_process_images(str(tmp_path / "in"), str(tmp_path / name), *_detectors(ids), batch_size=4,
                                   shard=shard, records=rec, mosaic_plates=True, hold=K, hold_iou_pct=P,
                                   hold_motion=True, loader=lambda p: frames[os.path.basename(p)],
                                   saver=lambda img, p, saved=saved: saved.__setitem__(os.path.basename(p), img.copy()))
        runs[name] = (tot, rec, saved)
    tot, rec, files = runs["one"]
    names = sorted(frames)
    assert tot[0] == N and sorted(rec) == names
    D = [_record_lists(rec, n) for n in names]
    B, H, _, _, stored = mr.hold_motion_lists(D, 120, 160, K, P)
    assert sum(len(h) for h in H) > 0 and _moved(H, stored) > 0
    for t, n in enumerate(names):
        np.testing.assert_array_equal(files[f"processed_{n}"], omosaic.mosaic_frame(frames[n], B[t], 8), err_msg=n)
    t2, r2, f2 = runs["two"]
    assert t2 == tot and r2 == rec and sorted(f2) == sorted(files)
    for k in files:
        assert files[k].tobytes() == f2[k].tobytes(), k


def test_pipeline_needs_a_detector_in_the_same_mode(gpu, tmp_path):
    import vdmi
    from vdmi import weights
    from vdmi.pipeline import batch_process_images
    (tmp_path / "in").mkdir()
    face = vdmi.Retinaface(input_shape=[640, 640, 3], max_batch=2, device_ids=[0],
                           weights=weights.retinaface_state_dict(0), hold=2)
    plate = vdmi.YOLO(weights="random", max_batch=2, device_ids=[0])
    with pytest.raises(ValueError, match="hold_motion"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, hold=2, hold_motion=True)
