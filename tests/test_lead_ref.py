"""The look-ahead hold's definition (tests/lead_ref.py) against known answers, its stream
simulator against the whole-stream lists, and the Python-side argument check. No GPU."""
import numpy as np
import pytest

import hold_ref as hr
import lead_ref as lr

A, FAR = (10, 10, 30, 30), (60, 60, 90, 95)
EMPTIES = [(200, 200, 240, 230), (60, 30, 60, 50), (-50, -50, -10, -10)]


def test_led_before_the_first_detection():
    """A box first seen in frame 2 is led into frames 0 (age 2) and 1 (age 1); frame 3 matches
    frame 2, so nothing is led from it."""
    Al, ages = lr.lead_lists([[], [], [A], [A]], 100, 100, 2, 30)
    assert Al == [[A], [A], [], []]
    assert ages == [[2], [1], [], []]


def test_order_is_age_then_list_order():
    Al, ages = lr.lead_lists([[], [FAR], [A]], 100, 100, 2, 30)
    assert Al[0] == [FAR, A] and ages[0] == [1, 2]
    assert Al[1] == [A] and ages[1] == [1]
    assert Al[2] == [] and ages[2] == []


def test_motion_stretches_backwards_along_the_way_the_face_came():
    seq = [[], [], [(40, 40, 60, 60)], [(45, 40, 65, 60)]]
    Al, ages = lr.lead_lists(seq, 100, 100, 2, 30, motion=True)
    assert Al[0] == [(30, 40, 60, 60)] and ages[0] == [2]
    assert Al[1] == [(35, 40, 60, 60)] and ages[1] == [1]
    # without motion: the boxes as stored
    Al0, ages0 = lr.lead_lists(seq, 100, 100, 2, 30)
    assert Al0[0] == [(40, 40, 60, 60)] and Al0[1] == [(40, 40, 60, 60)] and ages0 == ages
    # the last frame of a stream has no predecessor frame: led as stored
    Al, _ = lr.lead_lists(seq[:3], 100, 100, 2, 30, motion=True)
    assert Al[0] == [(40, 40, 60, 60)]


def test_match_is_inclusive_and_judged_on_clipped_boxes():
    # inter 30, union 100: 100 * 30 >= 30 * 100 matches; 27 of 100 does not
    assert lr.lead_lists([[(0, 0, 10, 3)], [(0, 0, 10, 10)]], 100, 100, 1, 30)[0] == [[], []]
    assert lr.lead_lists([[(0, 0, 9, 3)], [(0, 0, 10, 10)]], 100, 100, 1, 30)[0] == [[(0, 0, 10, 10)], []]
    # P = 100: identical after clipping matches
    assert lr.lead_lists([[(0, 0, 10, 10)], [(-5, -5, 10, 10)]], 100, 100, 1, 100)[0] == [[], []]


def test_empties_are_never_led_and_never_match():
    assert lr.lead_lists([[], EMPTIES], 100, 100, 2, 30)[0] == [[], []]
    assert lr.lead_lists([EMPTIES, [(50, 20, 70, 60)]], 100, 100, 1, 30)[0] == [[(50, 20, 70, 60)], []]


def test_led_boxes_are_stored_unclipped():
    assert lr.lead_lists([[], [(-5, -5, 10, 10)]], 100, 100, 1, 30)[0] == [[(-5, -5, 10, 10)], []]


def test_a_box_matched_in_between_is_not_led_further():
    """Frame 1 matches frame 2's box, so frame 0 is led frame 1's box (age 1) only."""
    near = (12, 12, 32, 32)
    Al, ages = lr.lead_lists([[], [near], [A]], 100, 100, 2, 30)
    assert Al[0] == [near] and ages[0] == [1]


def test_blur_list_order_and_labels():
    """B_t = D_t ++ H_t ++ A_t with labels 0, +a, -a."""
    seq = [[A], [], [FAR]]
    B, L = lr.blur_lists(seq, 100, 100, 2, 30, K=2)
    assert B[1] == [A, FAR] and L[1] == [1, -1]
    assert B[0] == [A, FAR] and L[0] == [0, -2]
    assert B[2] == [FAR, A] and L[2] == [0, 2]


def _random_sequence(seed, frames=12, h=120, w=160, most=40):
    rng = np.random.default_rng(seed)
    seq, prev = [], []
    for _ in range(frames):
        cur = []
        for _ in range(int(rng.integers(0, most + 1))):
            if prev and rng.random() < 0.5:
                b = np.asarray(prev[int(rng.integers(len(prev)))])
                if rng.random() < 0.75:
                    b = b + rng.integers(-6, 7, 4)
            else:
                x1, y1 = rng.integers(-20, 181, 2)
                b = np.asarray([x1, y1, x1 + rng.integers(-5, 60), y1 + rng.integers(-5, 60)])
            cur.append(tuple(int(v) for v in np.clip(b, -20, 180)))
        seq.append(cur)
        prev = cur
    return seq, h, w


@pytest.mark.parametrize("motion", [False, True], ids=["still", "motion"])
@pytest.mark.parametrize("K", [0, 2])
def test_simulator_is_call_split_invariant(K, motion):
    """12 random frames as one push + flush, as 5 + 7 and as twelve pushes of one frame (J = 3:
    pushes smaller than the delay) give the lists of the whole stream."""
    J, P = 3, 30
    seq, h, w = _random_sequence(11)
    want = lr.blur_lists(seq, h, w, J, P, motion, K=K, hold_motion=motion and K > 0)
    assert sum(1 for l in want[1] for v in l if v < 0) > 0
    delay = J + (1 if motion else 0)
    for cuts in ((12,), (5, 12), tuple(range(1, 13))):
        s = lr.Stream(h, w, J, P, motion, K=K, hold_motion=motion and K > 0)
        B, L, lo, pend = [], [], 0, 0
        for hi in cuts:
            b, l = s.push(seq[lo:hi])
            assert len(b) == max(0, pend + (hi - lo) - delay)
            pend += (hi - lo) - len(b)
            assert s.pending == pend
            B += b
            L += l
            lo = hi
        b, l = s.flush()
        assert len(b) == pend and s.pending == 0
        assert (B + b, L + l) == want, cuts


def test_a_flush_ends_the_stream():
    """Nothing is led across a flush: the frame after it is frame 0 of a new stream."""
    s = lr.Stream(100, 100, 2, 30)
    B, L = s.push([[], []], flush=True)
    assert B == [[], []]
    B, L = s.push([[A]], flush=True)
    assert B == [[A]] and L == [[0]]


def test_check_lead_refuses_bad_settings():
    from vdmi import _lib
    assert _lib.check_lead(0) == (0, False)
    assert _lib.check_lead(8, True) == (8, True)
    assert _lib.VD_LEAD_MAX == 8
    for bad in (9, -1):
        with pytest.raises(ValueError, match="lead"):
            _lib.check_lead(bad)
    with pytest.raises(ValueError, match="lead_motion"):
        _lib.check_lead(0, True)
