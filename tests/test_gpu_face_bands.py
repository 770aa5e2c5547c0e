"""Letterbox bands on the GPU (option face_bands): a context that leaves the stem's and
layer1's band tiles alone between calls against one that computes every tile in every call
(face_bands = 0), same weights, bit for bit, over call sequences that reuse, invalidate and
overwrite the kept tiles. vdt_face_band_stats shows that tiles really were left alone.

fp32 plan, net input 256x256, max_batch 4; frames of 256x64 letterbox by copy to canvas rows
96..159 (pool map 64x64): the stem has 3 + 4 band tile rows of 6, each layer1 block 2 + 2 of 8."""
import numpy as np
import pytest

import face_bands_ref as ref

pytestmark = pytest.mark.gpu

N = 4
OPS = 4


def _noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def pair(gpu):
    """(bands context, reference context): face_bands 1 (the default) and 0, same weights."""
    import vdmi
    from conftest import face_weights
    ctxs = []
    for bands in (None, 0):
        c = vdmi.Context(precision="fp32", max_batch=N, input_shape=(256, 256),
                         options={} if bands is None else {"face_bands": bands})
        c.load_weights(0, face_weights("default"))
        ctxs.append(c)
    yield tuple(ctxs)
    for c in ctxs:
        c.close()


def _heads(pair, frames):
    """forward_heads on both contexts (equal, bit for bit) -> the bands context's stats."""
    a, b = pair
    ha, hb = a.forward_heads(frames), b.forward_heads(frames)
    for x, y in zip(ha, hb):
        assert np.array_equal(x, y)
    assert not b.face_band_stats().any()          # the reference context never runs with bands
    return a.face_band_stats()


def _fresh(pair):
    """Both contexts forget their tags (any option change does)."""
    for c in pair:
        c.set_option("mosaic_nt", 0)


def _expect_rows(st, canvas_h, top, nh):
    want = ref.rule(canvas_h, top, nh, 0)
    assert [(int(r[0]), int(r[1]), int(r[2])) for r in st] == [(lo, hi, tr) for _, _, tr, lo, hi in want]


def test_same_frames_three_times(pair):
    _fresh(pair)
    f = _noise(N, 64, 256, 1)
    st = _heads(pair, f)
    _expect_rows(st, 256, 96, 64)
    assert [(int(r[0]), int(r[1]), int(r[2])) for r in st] == [(3, 7, 11), (2, 6, 8), (2, 6, 8), (2, 6, 8)]
    assert (st[:, 3] == 0).all() and (st[:, 4] == N).all()        # call 1: nothing to keep
    for _ in range(2):
        st = _heads(pair, f)
        assert (st[:, 3] == N).all() and (st[:, 4] == 0).all()    # calls 2, 3: every (frame, op) kept


def test_content_change_moves_an_exponent(pair):
    """Slot 0 alternates between noise and a frame of the pad colour (a constant canvas: the
    pooled map's maximum, and with it layer1.0's input exponent, differs from the noise frame's)."""
    _fresh(pair)
    a = _noise(N, 64, 256, 2)
    b = a.copy()
    b[0] = 128
    _heads(pair, a)
    for frames in (b, a, b, a):               # A B A B A: a tag from two calls back is not current
        st = _heads(pair, frames)
        assert st[0, 3] == N                  # the stem's tiles depend on no exponent
        # layer1.2's tag holds all three exponents: any move shows there; a block whose input
        # exponent moved takes the later blocks with it. Not vacuous: no move fails the test
        assert st[3, 4] >= 1 and st[3, 4] >= st[2, 4] >= st[1, 4], st
        assert (st[:, 3] == N - st[:, 4]).all()
        assert (st[1:, 3] >= N - 1).all(), st   # ... and only slot 0 ran band tiles
    st = _heads(pair, a)                      # the same frames again: kept
    assert (st[:, 3] == N).all()


def test_varying_n(pair):
    _fresh(pair)
    f, g = _noise(N, 64, 256, 3), _noise(2, 64, 256, 4)
    st = _heads(pair, f)
    assert (st[:, 4] == N).all()
    st = _heads(pair, g)
    assert (st[:, 3] + st[:, 4] == 2).all() and st[0, 3] == 2
    st = _heads(pair, f)                      # slots 2, 3 were not touched by the call of two
    assert (st[:, 3] + st[:, 4] == N).all() and (st[:, 3] >= 2).all() and st[0, 3] == N


def test_frame_sizes(pair):
    _fresh(pair)
    f64, f128 = _noise(N, 64, 256, 5), _noise(N, 128, 256, 6)
    for frames, top, nh in ((f64, 96, 64), (f128, 64, 128), (f64, 96, 64)):
        st = _heads(pair, frames)
        _expect_rows(st, 256, top, nh)
        assert (st[:, 3] == 0).all() and (st[:, 4] == N).all()    # first call of a size: nothing kept
        st = _heads(pair, frames)
        assert (st[:, 3] == N).all()


def test_frames_without_row_bands(pair):
    """A portrait frame (bands are columns) and a square one run without bands, and forget the tags."""
    _fresh(pair)
    f = _noise(N, 64, 256, 7)
    _heads(pair, f)
    for h, w in ((256, 64), (128, 128)):
        assert not _heads(pair, _noise(N, h, w, 8)).any()
        st = _heads(pair, f)
        assert (st[:, 3] == 0).all() and (st[:, 4] == N).all()


def test_invalidation(pair):
    from vdmi import weights
    _fresh(pair)
    f = _noise(N, 64, 256, 9)
    a, b = pair

    def first_then_kept():
        st = _heads(pair, f)
        assert (st[:, 3] == 0).all() and (st[:, 4] == N).all()
        st = _heads(pair, f)
        assert (st[:, 3] == N).all() and (st[:, 4] == 0).all()

    first_then_kept()
    a.set_option("face_bands", 0)             # off: every tile computed, no stats
    assert not _heads(pair, f).any()
    a.set_option("face_bands", 1)
    first_then_kept()
    for c in pair:                            # another option
        c.set_option("face_groups", 1)
    first_then_kept()
    for c in pair:
        c.set_option("face_groups", 2)
    first_then_kept()
    sd = weights.yolov8n_state_dict(0)        # a weight load (the face net loads once per context)
    for c in pair:
        c.load_weights(1, sd)
    first_then_kept()


def _process(pair, frames):
    a, b = pair
    oa, fa, _ = a.process(frames)
    ob, fb, _ = b.process(frames)
    assert np.array_equal(oa, ob)
    assert np.array_equal(fa.count, fb.count)
    for i in range(len(frames)):
        for x, y in zip(fa.frame(i), fb.frame(i)):
            assert np.array_equal(x, y)
    return a.face_band_stats()


def test_frame_groups_and_a_tiled_call(pair):
    """vd_process with one launch per layer and with two frame groups; a tiled call (its net
    inputs overwrite the canvases' buffers) between two plain ones."""
    a, b = pair
    f = _noise(N, 128, 512, 10)               # letterboxed to rows 96..159 by a 2x reduction
    try:
        for groups in (1, 2):
            for c in pair:
                c.set_option("face_groups", groups)
            st = _process(pair, f)
            assert (st[:, 4] == N).all()
            st = _process(pair, f)
            assert (st[:, 3] == N).all()
        for c in pair:
            c.set_tiles((1, 2))               # 3 net inputs per frame: one frame per call
        assert not _process(pair, f[:1]).any()
        for c in pair:
            c.set_tiles((1, 1))
        st = _process(pair, f)
        assert (st[:, 3] == 0).all() and (st[:, 4] == N).all()
        st = _process(pair, f)
        assert (st[:, 3] == N).all()
    finally:
        for c in pair:
            c.set_tiles((1, 1))
            c.set_option("face_groups", 2)
