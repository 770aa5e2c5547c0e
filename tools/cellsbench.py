"""Cost of box-scaled strength at the bench shape: Context.process on 64 synthetic 1080p frames
already in HBM (fp32, faces | plates | mosaic, as bench.py's flagship step), one context alive
at a time:

    row 1  pixelate, cells off          row 3  gaussian, ksize 31 (cells off)
    row 2  pixelate, cells 16           row 4  gaussian, cells 16 (the scaled smooth blur)
                                        row 5  gaussian, cells 16, mask ("ellipse", 42)

    python tools/cellsbench.py [--steps 20] [--warmup 3] [--json PATH]

Per row: ms/step (warm-up first, then the steps ended by one synchronise) and, from separately
event-timed steps, timing family 1 (the rectangular pass: mosaic output pass, Gaussian launches,
or the smooth blur's copy and box pass; the mask's restore pass behind it) as ms and launches
per step, in --repeats groups so that every figure comes with its own spread. The clipped area
of the blurred boxes is counted from the lists read back (the face keep lists; grown by the
mask where one is set). For the smooth blur the traffic model is 2 * n * W * H * 3 bytes for
the copy plus one read and one write of every clipped box, set against the 8 TB/s HBM peak.
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

HBM_PEAK = 8.0e12
ROWS = [("pixelate_off", "pixelate", 0, ("rect", 0)), ("pixelate_cells16", "pixelate", 16, ("rect", 0)),
        ("gaussian_k31", "gaussian", 0, ("rect", 0)), ("smooth_cells16", "gaussian", 16, ("rect", 0)),
        ("smooth_cells16_ellipse42", "gaussian", 16, ("ellipse", 42))]


def clipped_area(box, h, w):
    x1, y1, x2, y2 = (int(v) for v in box)
    return max(0, min(w, x2) - max(0, x1)) * max(0, min(h, y2) - max(0, y1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--fam-steps", type=int, default=5, help="event-timed steps per group behind the family figures")
    ap.add_argument("--repeats", type=int, default=3, help="groups of event-timed steps (the spread of family 1)")
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
           "fam_steps": a.fam_steps, "repeats": a.repeats, "rows": {}}
    for name, blur, cells, mask in ROWS:
        ctx = vdmi.Context(device=0, precision="fp32", max_batch=B, blur=blur, cells=cells, mask=mask[0],
                           mask_grow=mask[1])
        ctx.load_weights(_lib.VD_NET_RETINAFACE, fw)
        ctx.load_weights(_lib.VD_NET_YOLOV8N, pw)
        faces, plates = vdmi.DeviceBoxes(B, 256, dev), vdmi.DeviceBoxes(B, 256, dev)
        step = lambda: ctx.process(frames, out, faces=faces, plates=plates, flags=flags)
        torch.cuda.synchronize()
        for _ in range(max(a.warmup, 1)):
            step()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        # the family alone, in steps of their own (events around every launch slow the step)
        fam, launches = [], 0
        ctx.timing(True)
        for _ in range(a.repeats):
            ctx.timing_reset()
            for _ in range(a.fam_steps):
                step()
            ctx.sync()
            f_ms, f_n, _ = ctx.timing_read(_lib.FAM_MOSAIC)
            fam.append(round(f_ms / a.fam_steps, 4))
            launches = f_n / a.fam_steps
        ctx.timing(False)
        full = ctx.read_boxes(_lib.VD_NET_RETINAFACE, B)
        blurred = ctx.mask_boxes(full) if mask != ("rect", 0) else full
        nbox = area = 0
        for f in range(B):
            for b in blurred.xyxy[f, :int(blurred.count[f])]:
                nbox, area = nbox + 1, area + clipped_area(b, H, W)
        r = {"ms_per_step": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
             "fam1_ms_per_step": fam, "fam1_ms_mean": round(sum(fam) / len(fam), 4),
             "fam1_spread_ms": round(max(fam) - min(fam), 4), "fam1_launches_per_step": launches,
             "boxes_per_frame": nbox / B, "box_pixels_per_frame": area / B,
             "box_share_of_frame": round(area / B / (H * W), 4)}
        if blur == "gaussian" and cells:
            model = 2.0 * B * W * H * 3 + 2.0 * area * 3
            r["model_bytes_per_step"] = int(model)
            r["model_gb_per_s"] = round(model / (r["fam1_ms_mean"] * 1e-3) / 1e9, 1)
            r["share_of_hbm_peak"] = round(model / (r["fam1_ms_mean"] * 1e-3) / HBM_PEAK, 4)
        res["rows"][name] = r
        ctx.close()
        del ctx
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
