"""Cost of box hold at the bench shape: Context.process on 64 synthetic 1080p frames already
in HBM (fp32, faces | plates | mosaic, as bench.py's flagship step) with hold 0 / 2 / 8.

    python tools/holdbench.py [--steps 20] [--warmup 3] [--json PATH]

Per setting: ms/step (warm-up first, then the steps ended by one synchronise), held boxes
per frame, and the hold launch's own time -- timing family 3 (post: decode, NMS, hold) of a
separately timed step, against the hold-0 run's. The seeded noise frames share nothing
from one frame to the next, so a box of the last `hold` frames is held unless another box
matches it by chance: the heavy case for the hold kernel and for the mosaic behind it (a
video holds a box only where a detection went missing). The first holding call also
allocates the merged rows and the larger mosaic table; it is part of the warm-up, not of the
timed steps.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--holds", default="0,2,8")
    ap.add_argument("--json", help="also write the result line to this file")
    a = ap.parse_args()
    import vdmi
    from vdmi import _lib, synth, weights
    B, H, W = a.batch, 1080, 1920
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(synth.frames(B, H, W, seed=0)).to(dev)
    out = torch.empty_like(frames)
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC
    fw, pw = weights.retinaface_state_dict(0), weights.yolov8n_state_dict(0)
    res = {"batch": B, "frame": [H, W], "precision": "fp32", "steps": a.steps, "warmup": a.warmup,
           "note": "noise frames: a box of the last `hold` frames is held unless matched by chance (heavy case)"}
    base_post = None
    for hold in [int(v) for v in a.holds.split(",")]:
        ctx = vdmi.Context(device=0, precision="fp32", max_batch=B, hold=hold)
        ctx.load_weights(_lib.VD_NET_RETINAFACE, fw)
        ctx.load_weights(_lib.VD_NET_YOLOV8N, pw)
        faces, plates = vdmi.DeviceBoxes(B, 256, dev), vdmi.DeviceBoxes(B, 256, dev)
        torch.cuda.synchronize()
        step = lambda: ctx.process(frames, out, faces=faces, plates=plates, flags=flags)
        for _ in range(max(a.warmup, 1)):
            step()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        r = {"ms_per_step": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
             "faces_per_frame": float(faces.count.float().mean().item())}
        if hold:
            r["held_per_frame"] = float(ctx.read_held(B, cap=1).count.mean())
        # the post family alone, in steps of their own (events around every launch slow the step)
        ctx.timing(True)
        ctx.timing_reset()
        for _ in range(5):
            step()
        post_ms, launches, _ = ctx.timing_read(_lib.FAM_POST)
        ctx.timing(False)
        r["post_ms_per_step"] = round(post_ms / 5, 4)
        r["post_launches_per_step"] = launches / 5
        if hold == 0:
            base_post = post_ms / 5
        elif base_post is not None:
            r["hold_launch_ms"] = round(post_ms / 5 - base_post, 4)
        res[f"hold_{hold}"] = r
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
