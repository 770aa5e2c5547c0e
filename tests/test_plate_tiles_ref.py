"""The tiled plate merge's numpy reference (tests/plate_tiles_ref.py) against the face merge's
(tests/tiles_ref.py) and against hand-made cases, and the pure-Python tile_nets validator. No GPU."""
import numpy as np
import pytest

import plate_tiles_ref as pr
import tiles_ref as tr

F32 = np.float32


def _random_lists(rng, rects, kmax, labels):
    """Per input up to kmax boxes, relative to its rectangle: objects of the frame as every input
    that holds them sees them (moved by up to 2 px, so most pairs overlap by more than 0.7 and some
    by less), with repeated scores."""
    objs = []
    for _ in range(kmax):
        x1, y1 = rng.uniform(0, rects[0][2] - 100), rng.uniform(0, rects[0][3] - 40)
        objs.append((x1, y1, x1 + rng.uniform(12, 90), y1 + rng.uniform(6, 30)))
    out = []
    for (x0, y0, tw, th) in rects.tolist():
        xf, lab = [], []
        for (x1, y1, x2, y2) in objs:
            if x1 >= x0 and y1 >= y0 and x2 <= x0 + tw and y2 <= y0 + th and rng.uniform() < 0.8:
                xf.append(np.asarray([x1 - x0, y1 - y0, x2 - x0, y2 - y0]) + rng.uniform(-2, 2, 4))
                lab.append(rng.choice(labels))          # per sighting: inputs may disagree on the class
        sc = rng.choice(np.asarray([0.5, 0.625, 0.75, 0.9, 0.95], F32), len(xf))
        out.append((np.asarray(xf, F32).reshape(-1, 4), sc, np.asarray(lab, np.int32)))
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("iou", [0.7, 0.4])
def test_one_class_is_the_face_merge(seed, iou):
    """With all labels equal the class test never fires: counts, boxes, scores and the kept
    sources equal tiles_ref.merge_frame at the same IoU (its label rule aside)."""
    rects = tr.tile_rects(720, 1280, 2, 2, 20)
    origins = [(int(q[0]), int(q[1])) for q in rects]
    rng = np.random.default_rng(seed)
    lists = _random_lists(rng, rects, 40, np.asarray([3]))
    a = pr.merge_frame(lists, origins, iou)
    b = tr.merge_frame(lists, origins, 16800, iou)
    assert len(a[0]) == len(b[0]) and 0 < len(a[0]) < sum(len(l[1]) for l in lists)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert a[4] == b[4]
    assert np.all(a[3] == 3)                                # label = the class id
    none = [(xf, sc, None) for xf, sc, _ in lists]          # no labels: class 0
    c = pr.merge_frame(none, origins, iou)
    assert c[4] == a[4] and np.all(c[3] == 0)


def test_classes_split_the_merge():
    """More classes can only keep more: every class's kept boxes are the one-class merge of that
    class's boxes alone, interleaved in score order."""
    rects = tr.tile_rects(720, 1280, 2, 2, 20)
    origins = [(int(q[0]), int(q[1])) for q in rects]
    rng = np.random.default_rng(7)
    lists = _random_lists(rng, rects, 40, np.asarray([0, 1, 2]))
    got = pr.merge_frame(lists, origins, 0.7)
    for c in (0, 1, 2):
        own = [(xf[lab == c], sc[lab == c], lab[lab == c]) for xf, sc, lab in lists]
        ref = pr.merge_frame(own, origins, 0.7)
        sel = got[3] == c
        assert np.array_equal(got[1][sel].view(np.uint32), ref[1].view(np.uint32))
        assert np.array_equal(got[2][sel].view(np.uint32), ref[2].view(np.uint32))
    keys = [(-int(np.asarray(s, F32).view(np.uint32)), t, p) for s, (t, p) in zip(got[2], got[4])]
    assert keys == sorted(keys)
    one = pr.merge_frame([(xf, sc, np.zeros_like(lab)) for xf, sc, lab in lists], origins, 0.7)
    assert len(got[0]) > len(one[0])


def test_identical_boxes_of_two_classes_are_both_kept():
    box = np.asarray([[100, 50, 160, 70]], F32)
    origins = [(0, 0), (0, 0)]
    two = pr.merge_frame([(box, np.asarray([0.9], F32), np.asarray([0])),
                          (box, np.asarray([0.8], F32), np.asarray([1]))], origins, 0.7)
    assert two[4] == [(0, 0), (1, 0)] and two[3].tolist() == [0, 1]
    same = pr.merge_frame([(box, np.asarray([0.9], F32), np.asarray([1])),
                           (box, np.asarray([0.8], F32), np.asarray([1]))], origins, 0.7)
    assert same[4] == [(0, 0)] and same[3].tolist() == [1]
    # equal scores: the lower input wins the tie
    tie = pr.merge_frame([(box, np.asarray([0.8], F32), np.asarray([1])),
                          (box, np.asarray([0.8], F32), np.asarray([1]))], origins, 0.7)
    assert tie[4] == [(0, 0)]


@pytest.mark.parametrize("height,kept", [(7.001, 1), (6.999, 2), (7.0, 2)])
def test_iou_pair_across_inputs_at_0_7(height, kept):
    """A 10 x 10 whole-frame box against a 10 x `height` box seen by tile (1, 1), whose origin
    moves it onto the first: IoU just above 0.7 is suppressed, just below is kept. An IoU of
    exactly 7 / 10 is kept too: its float32 quotient lies below the double 0.7."""
    rects = tr.tile_rects(360, 640, 2, 2, 20)
    origins = [(int(q[0]), int(q[1])) for q in rects]
    x0, y0 = origins[4]
    assert x0 > 0 and y0 > 0
    a = np.asarray([[x0 + 20, y0 + 30, x0 + 30, y0 + 40]], F32)
    b = np.asarray([[20, 30, 30, 30 + height]], F32)
    empty = (np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32))
    lists = [(a, np.asarray([0.9], F32), np.asarray([0])), empty, empty, empty,
             (b, np.asarray([0.8], F32), np.asarray([0]))]
    got = pr.merge_frame(lists, origins, 0.7)
    assert len(got[0]) == kept
    assert got[4][0] == (0, 0)
    if kept == 2:
        assert got[4][1] == (4, 0)
        assert np.array_equal(got[1][1], (b[0] + np.asarray([x0, y0, x0, y0], F32)).astype(F32))
        assert got[0][1].tolist() == [x0 + 20, y0 + 30, x0 + 30, y0 + 30 + int(height)]


def test_check_tile_nets():
    from vdmi import _lib
    for name, bits in (("faces", 1), ("plates", 2), ("both", 3)):
        assert _lib.check_tile_nets(name) == name and _lib.TILE_NETS[name] == bits
    assert (_lib.VD_TILE_FACES, _lib.VD_TILE_PLATES) == (1, 2)
    for bad in ("face", "BOTH", "", None, 3, 2.0, ("plates",), b"plates"):
        with pytest.raises(ValueError):
            _lib.check_tile_nets(bad)
