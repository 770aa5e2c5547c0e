"""Cost of tiled face detection at 4K: Context.process (faces | mosaic) on synthetic 3840x2160
frames already in HBM, fp32 and fp16, with tiling off and with tiles (2, 2, 20), in contexts of
one max_batch, so both push the same number of net inputs through the face net per step:
max_batch frames untiled, max_batch // 5 frames tiled.

    python tools/tilesbench.py [--max-batch 20] [--steps 100] [--warmup 3] [--repeats 5] [--json PATH]

Per precision the settings alternate `repeats` times, each run in a context of its own with no
other context alive (other work shares the machine: the
spread over the repeats is what a difference is judged against). Per run: ms/step (warm-up
first, then the steps ended by one synchronise) and, from separately event-timed steps, the ms
and launches per step of timing families 0 (face convs), 2 (letterbox) and 3 (post: decode / NMS
per input, and the tile merge). Reported as median, min and max over the repeats.

A third setting, off_crops, is a control: the untiled path on max_batch frames that are the
tiles themselves, i.e. the tiled run's net inputs without its letterbox and merge.

Two expectations, checked against the tiles-off runs of the same build with their own spread
(max - min over the repeats) as the margin, and recorded either way:
  conv_ms_per_input   family 0 per net input: the kernels and the batch are the same, so tiled
                      and untiled should agree;
  letterbox_ps_per_source_byte   family 2 per source byte read, n * (h*w + R*C*th*tw) * 3 tiled
                      against n * h*w * 3 untiled.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))

import torch  # noqa: E402

H, W = 2160, 3840
TILES, OVERLAP = (2, 2), 20
FAMS = {"conv": 0, "letterbox": 2, "post": 3}


def one_run(ctx, frames, out, faces, flags, a):
    step = lambda: ctx.process(frames, out, faces=faces, flags=flags)
    torch.cuda.synchronize()
    for _ in range(max(a.warmup, 1)):
        step()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    ctx.sync()
    r = {"ms_per_step": (time.perf_counter() - t0) * 1e3 / a.steps}
    # the families alone, in steps of their own (events around every launch slow the step)
    ctx.timing(True)
    ctx.timing_reset()
    for _ in range(a.fam_steps):
        step()
    ctx.sync()
    for name, fam in FAMS.items():
        ms, n, _ = ctx.timing_read(fam)
        r[f"{name}_ms_per_step"] = ms / a.fam_steps
        r[f"{name}_launches_per_step"] = n / a.fam_steps
    ctx.timing(False)
    return r


def summary(runs):
    out = {}
    for k in runs[0]:
        v = [r[k] for r in runs]
        out[k] = {"median": float(f"{statistics.median(v):.6g}"), "min": float(f"{min(v):.6g}"),
                  "max": float(f"{max(v):.6g}")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-batch", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fam-steps", type=int, default=10, help="event-timed steps behind the family figures")
    ap.add_argument("--precisions", default="fp32,fp16")
    ap.add_argument("--json", help="also write the result line to this file")
    a = ap.parse_args()
    import vdmi
    from vdmi import _lib, synth, weights
    T = 1 + TILES[0] * TILES[1]
    B = a.max_batch
    if B < T:
        raise SystemExit(f"--max-batch must be at least {T}")
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(synth.frames(B, H, W, seed=0)).to(dev)
    out = torch.empty_like(frames)
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
    fw = weights.retinaface_state_dict(0)
    rects = _lib.tile_rects(H, W, TILES, OVERLAP)
    tw, th = int(rects[1, 2]), int(rects[1, 3])
    tl = rects[1:].tolist()
    crops = torch.stack([frames[i // len(tl), y0:y0 + th, x0:x0 + tw]
                         for i, (x0, y0, _, _) in ((i, tl[i % len(tl)]) for i in range(B))]).contiguous()
    crops_out = torch.empty_like(crops)
    res = {"frame": [H, W], "max_batch": B, "tiles": list(TILES), "tile_overlap": OVERLAP, "tile": [th, tw],
           "net_inputs_per_frame": T, "steps": a.steps, "warmup": a.warmup, "fam_steps": a.fam_steps,
           "repeats": a.repeats}
    for prec in a.precisions.split(","):
        # off_crops: a control, the untiled path on max_batch frames that ARE tiles (the crops of the
        # first frames): the net inputs of the tiled run without its letterbox and merge
        cfgs = {"off": ((1, 1), B, frames, out), "tiled": (TILES, B // T, frames, out),
                "off_crops": ((1, 1), B, crops, crops_out)}
        # One context alive at a time, as a user's process has. With the settings' contexts alive side
        # by side the same setting ran in one of two regimes from run to run: the face net's two
        # frame-group streams overlapping (fp32 tiled 7.7 ms/step, family-0 sum twice the step) or back
        # to back (10.6 ms/step, sum equal to the step). Presumably two streams of one context then
        # share one of the process's few hardware queues; the cause was not isolated further.
        runs = {name: [] for name in cfgs}
        faces_per_frame = {}
        for _ in range(a.repeats):                        # alternate the settings
            for name, (tiles, n, src_frames, dst) in cfgs.items():
                c = vdmi.Context(device=0, precision=prec, max_batch=B, tiles=tiles, tile_overlap=OVERLAP)
                c.load_weights(_lib.VD_NET_RETINAFACE, fw)
                runs[name].append(one_run(c, src_frames[:n], dst[:n], vdmi.DeviceBoxes(n, 256, dev), flags, a))
                faces_per_frame[name] = float(c.read_boxes(_lib.VD_NET_RETINAFACE, n).count.mean())
                c.close()
                print(f"{prec} {name}: {runs[name][-1]['ms_per_step']:.3f} ms/step", file=sys.stderr, flush=True)
        rows = {}
        for name, (tiles, n, _, _) in cfgs.items():
            inputs = n * (T if name == "tiled" else 1)
            src = n * (H * W + TILES[0] * TILES[1] * th * tw if name == "tiled" else
                       th * tw if name == "off_crops" else H * W) * 3
            for r in runs[name]:
                r["frames_per_s"] = n / r["ms_per_step"] * 1e3
                r["conv_ms_per_input"] = r["conv_ms_per_step"] / inputs
                r["letterbox_ps_per_source_byte"] = r["letterbox_ms_per_step"] * 1e9 / src
            rows[name] = {"frames_per_step": n, "net_inputs_per_step": inputs, "source_bytes_per_step": src,
                          "faces_per_frame": faces_per_frame[name], **summary(runs[name])}
        checks = {}
        for k in ("conv_ms_per_input", "letterbox_ps_per_source_byte"):
            o, t = rows["off"][k], rows["tiled"][k]
            margin = o["max"] - o["min"]
            checks[k] = {"off": o["median"], "tiled": t["median"], "margin_off_spread": float(f"{margin:.6g}"),
                         "holds": abs(t["median"] - o["median"]) <= margin}
        rows["expectations"] = checks
        res[prec] = rows
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
