"""The rescue definition (tests/rescue_ref.py) against known answers and its own invariants, on the CPU."""
import pytest

import hold_ref as hr
import rescue_ref as rr

SETTINGS = [(1, 1, 30), (3, 5, 30), (8, 4, 1), (1, 255, 100), (2, 3, 30)]   # (W, S, P)


@pytest.mark.parametrize("name", sorted(rr.CRAFTED))
def test_known_answers(name):
    strong, weak, W, S, P, want_r, want_s = rr.CRAFTED[name]
    E, since, R, idx, _ = rr.rescue_lists(strong, weak, 100, 100, W, S, P)
    assert R == want_r
    for t in range(len(strong)):
        assert E[t] == list(strong[t]) + R[t]
        assert since[t] == [0] * len(strong[t]) + want_s[t]
        assert [weak[t][i] for i in idx[t]] == R[t]


def test_chain_reaches_the_span_and_no_further():
    for S in (1, 2, 7):
        n = S + 3
        strong = [[rr.A]] + [[] for _ in range(n - 1)]
        weak = [[]] + [[rr.A] for _ in range(n - 1)]
        _, since, R, _, _ = rr.rescue_lists(strong, weak, 100, 100, 1, S, 30)
        assert [s for s in since[1:S + 1]] == [[k] for k in range(1, S + 1)]
        assert all(r == [] for r in R[S + 1:])


def test_gap_of_W_is_bridged():
    for W in (1, 3, 8):
        for gap, hit in ((W, True), (W + 1, False)):
            strong = [[rr.A]] + [[] for _ in range(gap)]
            weak = [[] for _ in range(gap)] + [[rr.A2]]
            _, since, R, _, _ = rr.rescue_lists(strong, weak, 100, 100, W, 255, 30)
            assert R[-1] == ([rr.A2] if hit else []) and since[-1] == ([gap] if hit else [])


@pytest.mark.parametrize("W,S,P", SETTINGS)
@pytest.mark.parametrize("seed", range(6))
def test_random_sequences_have_every_outcome_and_split_anywhere(seed, W, S, P):
    strong, weak, h, w = rr.random_sequence(seed)
    E, since, R, idx, _ = rr.rescue_lists(strong, weak, h, w, W, S, P)
    assert sum(len(r) for r in R) > 0
    assert sum(len(k) for k in weak) - sum(len(r) for r in R) > 0
    assert any(hr.clip_box(b, h, w) is None for k in weak for b in k)
    assert R[0] == []
    if S >= 2:
        assert any(s >= 2 for row in since for s in row)
    assert all(0 <= s <= S for row in since for s in row)
    # call-split invariance through the history
    for cuts in ((5, 12), tuple(range(1, 13))):
        hist, got, lo = None, [], 0
        for hi in cuts:
            e, s, _, _, hist = rr.rescue_lists(strong[lo:hi], weak[lo:hi], h, w, W, S, P, hist)
            got += list(zip(e, s))
            lo = hi
        assert got == list(zip(E, since)), cuts


@pytest.mark.parametrize("W,S,P", SETTINGS[:3] + SETTINGS[4:])
def test_horizon(W, S, P):
    """E_t depends on frames [t - S, t] only: a stream that starts S frames early reproduces it."""
    for seed in range(6):
        strong, weak, h, w = rr.random_sequence(seed, frames=16)
        E, since, _, _, _ = rr.rescue_lists(strong, weak, h, w, W, S, P)
        for t0 in range(S, 16):
            e, s, _, _, _ = rr.rescue_lists(strong[t0 - S:], weak[t0 - S:], h, w, W, S, P)
            assert e[S:] == E[t0:] and s[S:] == since[t0:], (seed, t0)
