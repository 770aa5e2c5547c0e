"""Look-ahead hold, the definition (include/vdmi.h "look-ahead hold") on top of the
box-hold references: A_t is the hold list of the time-reversed stream.

The checker of tests/test_lead_ref.py and tests/test_gpu_lead.py; it never imports vdmi.

For a stream D_0 .. D_{T-1} (T frames between two stream ends) the lead list A_t is
H_{T-1-t} of the reversed stream D_{T-1} .. D_0 under K = J: for a = 1..J (t + a < T), in the
order of D_{t+a}, every box of D_{t+a} that is non-empty after clipping and matches no box of
D_t .. D_{t+a-1}, stored unclipped. With motion the predecessor is sought in D_{t+a+1} and the
stored box is the hull of b and c + a * (c - clip(p)). Frame t is blurred with
B_t = D_t ++ H_t ++ A_t, H_t the (forward) hold list, empty when K == 0.
"""
import hold_motion_ref as hm
import hold_ref as hr


def lead_lists(seq, h, w, J, P, motion=False):
    """seq: the D lists of ONE whole stream. -> (A, ages): per frame the led boxes (int
    4-tuples) and their ages a (the box was first seen in frame t + a)."""
    seq = [hr._as_list(d) for d in seq]
    if J <= 0:
        return [[] for _ in seq], [[] for _ in seq]
    rev = seq[::-1]
    if motion:
        _, H, ages, _, _ = hm.hold_motion_lists(rev, h, w, J, P)
    else:
        _, H, ages, _ = hr.hold_lists(rev, h, w, J, P)
    return [list(x) for x in H[::-1]], [list(a) for a in ages[::-1]]


def hold_part(seq, h, w, K, P, motion=False):
    """The forward hold lists (H, ages) of one whole stream; empty lists when K == 0."""
    seq = [hr._as_list(d) for d in seq]
    if K <= 0:
        return [[] for _ in seq], [[] for _ in seq]
    if motion:
        _, H, ages, _, _ = hm.hold_motion_lists(seq, h, w, K, P)
    else:
        _, H, ages, _ = hr.hold_lists(seq, h, w, K, P)
    return H, ages


def blur_lists(seq, h, w, J, P, motion=False, K=0, hold_motion=False):
    """-> (B, labels): per frame B_t = D_t ++ H_t ++ A_t and the labels 0 (own), +a (held from
    frame t - a), -a (led from frame t + a)."""
    seq = [hr._as_list(d) for d in seq]
    H, ha = hold_part(seq, h, w, K, P, hold_motion)
    A, la = lead_lists(seq, h, w, J, P, motion)
    B = [d + list(H[t]) + A[t] for t, d in enumerate(seq)]
    labels = [[0] * len(d) + list(ha[t]) + [-a for a in la[t]] for t, d in enumerate(seq)]
    return B, labels


class Stream:
    """The stream simulator: push n frames, get the m frames whose look-ahead is complete.

    It keeps what the library keeps: the pending frames' D lists (and, for the forward hold,
    the whole stream's D lists so far). A frame is emitted once D_{t+delay} is known (delay =
    J + motion), or at a flush, and its lists are computed from the frames known at that
    moment only -- never from the whole stream -- so equality with lead_lists() over the whole
    stream is the call-split invariance of the definition."""

    def __init__(self, h, w, J, P, motion=False, K=0, hold_motion=False):
        self.h, self.w, self.J, self.P, self.motion = h, w, int(J), P, bool(motion)
        self.K, self.hold_motion = int(K), bool(hold_motion)
        self.delay = self.J + (1 if self.motion else 0)
        self.reset()

    def reset(self):
        self.seen = []          # D lists since the last stream end
        self.emitted = 0        # frames of `seen` already emitted

    @property
    def pending(self):
        return len(self.seen) - self.emitted

    def push(self, seq, flush=False):
        """-> (B, labels) of the m emitted frames; m = max(0, pending + n - delay), or
        pending + n with flush (which ends the stream)."""
        n = len(seq)
        m = self.pending + n if flush else max(0, self.pending + n - self.delay)
        self.seen += [hr._as_list(d) for d in seq]
        B, L = [], []
        H, ha = hold_part(self.seen, self.h, self.w, self.K, self.P, self.hold_motion)
        for t in range(self.emitted, self.emitted + m):
            # what frame t may look at: t .. t + delay, clipped to the frames known
            win = self.seen[t:t + self.delay + 1]
            A, la = lead_lists(win, self.h, self.w, self.J, self.P, self.motion)
            B.append(self.seen[t] + list(H[t]) + A[0])
            L.append([0] * len(self.seen[t]) + list(ha[t]) + [-a for a in la[0]])
        self.emitted += m
        if flush:
            self.reset()
        return B, L

    def flush(self):
        return self.push([], flush=True)
