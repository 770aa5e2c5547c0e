"""Cost of mask shaping at the bench shape: Context.process on 64 synthetic 1080p frames already
in HBM (fp32, faces | plates | mosaic, as bench.py's flagship step) with the mask off and
grow 30 / 42 as rect and as ellipse, pixelating and Gaussian (k = 31).

    python tools/maskbench.py [--steps 20] [--warmup 3] [--json PATH]

Per setting: ms/step (warm-up first, then the steps ended by one synchronise) and, from
separately event-timed steps, timing family 3 (post: decode, NMS, mask grow) and family 1 (the
rectangular pass, and the mask's restore pass behind it). The two new launches' own times are
differences inside one build: grow = family 3 minus the mask-off run's; restore = family 1 of
the ellipse run minus family 1 of the rect run at the same grow (both blur the same grown
lists). Against the traffic model: the grow launch moves 16 B per box, the restore pass 6 B
(3 read, 3 written) per pixel of a clipped grown box outside its own ellipse, counted here
exactly from the lists read back (pixels inside another box's ellipse are not moved, so this
is an upper bound).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SETTINGS = [("off", "rect", 0), ("rect_30", "rect", 30), ("ellipse_30", "ellipse", 30), ("rect_42", "rect", 42),
            ("ellipse_42", "ellipse", 42)]


def outside_pixels(box, h, w):
    """(pixels of the clipped box, those of them outside the box's ellipse), vdmi.h's predicate."""
    x1, y1, x2, y2 = (int(v) for v in box)
    W, H = x2 - x1, y2 - y1
    cx1, cy1, cx2, cy2 = max(0, x1), max(0, y1), min(w, x2), min(h, y2)
    if cx2 <= cx1 or cy2 <= cy1:
        return 0, 0
    area = (cx2 - cx1) * (cy2 - cy1)
    if W > 32768 or H > 32768:
        return area, 0
    dx = (2 * np.arange(cx1, cx2, dtype=np.int64) + 1 - (x1 + x2))[None, :]
    dy = (2 * np.arange(cy1, cy2, dtype=np.int64) + 1 - (y1 + y2))[:, None]
    return area, int((dx * dx * H * H + dy * dy * W * W > W * W * H * H).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--fam-steps", type=int, default=10, help="event-timed steps behind the family figures")
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
           "fam_steps": a.fam_steps}
    for blur in ("pixelate", "gaussian"):
        ctx = vdmi.Context(device=0, precision="fp32", max_batch=B, blur=blur)
        ctx.load_weights(_lib.VD_NET_RETINAFACE, fw)
        ctx.load_weights(_lib.VD_NET_YOLOV8N, pw)
        faces, plates = vdmi.DeviceBoxes(B, 256, dev), vdmi.DeviceBoxes(B, 256, dev)
        step = lambda: ctx.process(frames, out, faces=faces, plates=plates, flags=flags)
        rows = {}
        for name, shape, g in SETTINGS:
            ctx.set_mask(shape, g)
            torch.cuda.synchronize()
            for _ in range(max(a.warmup, 1)):
                step()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            # the families alone, in steps of their own (events around every launch slow the step)
            ctx.timing(True)
            ctx.timing_reset()
            for _ in range(a.fam_steps):
                step()
            ctx.sync()
            post_ms, post_n, _ = ctx.timing_read(_lib.FAM_POST)
            blur_ms, blur_n, _ = ctx.timing_read(_lib.FAM_MOSAIC)
            ctx.timing(False)
            r = {"ms_per_step": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
                 "post_ms_per_step": round(post_ms / a.fam_steps, 4), "post_launches_per_step": post_n / a.fam_steps,
                 "blur_ms_per_step": round(blur_ms / a.fam_steps, 4), "blur_launches_per_step": blur_n / a.fam_steps}
            full = ctx.read_boxes(_lib.VD_NET_RETINAFACE, B)
            grown = ctx.mask_boxes(full)
            nbox = area = outside = 0
            for f in range(B):
                for b in grown.xyxy[f, :int(grown.count[f])]:
                    ar, o = outside_pixels(b, H, W)
                    nbox, area, outside = nbox + 1, area + ar, outside + o
            r["boxes_per_frame"] = nbox / B
            r["grown_box_pixels_per_frame"] = area / B
            r["model_grow_bytes_per_step"] = 16 * nbox
            if shape == "ellipse":
                r["model_restore_bytes_per_step"] = 6 * outside
                r["outside_share_of_box_area"] = round(outside / max(area, 1), 4)
            rows[name] = r
        for name, shape, g in SETTINGS[1:]:
            rows[name]["grow_launch_ms"] = round(rows[name]["post_ms_per_step"] - rows["off"]["post_ms_per_step"], 4)
            rows[name]["added_ms_per_step"] = round(rows[name]["ms_per_step"] - rows["off"]["ms_per_step"], 3)
        for g in (30, 42):
            e, r = rows[f"ellipse_{g}"], rows[f"rect_{g}"]
            e["restore_launch_ms"] = round(e["blur_ms_per_step"] - r["blur_ms_per_step"], 4)
        res[blur] = rows
        ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
