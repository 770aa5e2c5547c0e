"""Planar 4:2:0 against NV12 at 1080p: the output pass (timing family 1) and the letterbox (family 2)
of 64 device surfaces in 4-frame steps, all in one session.

    python tools/yuv420bench.py --parent-lib PATH/libvdmi.so [--repeats 3] [--passes 3]
                                [--json profiles/yuv420_1080p.json]

A child process per measurement (a fresh context, a fresh library), parent and this build alternating,
`--repeats` of each:
    parent   the PARENT commit's build (through VDMI_LIB; the *_yuv420 entries are not bound): the case
             nv12_old alone. Its run-to-run spread is the margin of every comparison below.
    this     this build, four cases:
               nv12_old    NV12 surfaces through the *_nv12 entries (must equal `parent` within the margin)
               nv12_new    the same surfaces through the *_yuv420 entries with layout "nv12" (the same kernels)
               i420_i420   I420 in, I420 out
               i420_nv12   I420 in, NV12 out (a decoder's layout into an encoder's)
Per case, over the face lists detected on synth's RGB frames of the same size (the dense box set of
tools/cellsbench.py, some 30 boxes a frame): ms per 4-frame step of
    mosaic      family 1 of mosaic_* (pixelation, level 8): one launch, 2 x 1.5 B/px
    smooth      family 1 of smooth_* (level 8, cells 16): the copy and the box pass
    letterbox   family 2 of process_* with VD_PROC_FACES: the face letterbox reading 1.5 B/px of source
each the mean over `--passes` passes over the 16 steps, events around every launch.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

YUV420_ENTRIES = ("vd_process_yuv420", "vd_mosaic_yuv420", "vd_smooth_yuv420", "vd_yuv420_to_rgb", "vdt_letterbox_yuv420")
CASES = ("nv12_old", "nv12_new", "i420_i420", "i420_nv12")
PASSES = ("mosaic", "smooth", "letterbox")
STEP, SURFACES, SCENES = 4, 64, 16


def to_i420(nv, H, W):
    """The I420 surfaces with the samples of packed NV12 surfaces (torch, on the device)."""
    import torch
    n, q = nv.shape[0], (H // 2) * (W // 2)
    out = torch.empty_like(nv)
    out[:, :H] = nv[:, :H]
    uv = nv[:, H:].reshape(n, H // 2, W // 2, 2)
    flat = out.view(n, -1)
    flat[:, H * W:H * W + q] = uv[..., 0].reshape(n, q)
    flat[:, H * W + q:] = uv[..., 1].reshape(n, q)
    return out


def one(a):
    """--one parent | this: every case this library has, one context, the same boxes."""
    import torch
    from vdmi import _lib
    parent = a.one == "parent"
    if parent:               # the parent's build does not export the *_yuv420 entries
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in YUV420_ENTRIES]
    import vdmi
    from nv12bench import nv12_frames
    from vdmi import synth, weights
    H, W = 1080, 1920
    dev = torch.device("cuda:0")
    # 64 surfaces: SCENES distinct scenes, each four times (a pass's time follows the boxes and the bytes)
    nv = nv12_frames(SCENES, H, W, dev).repeat(SURFACES // SCENES, 1, 1)
    i420 = to_i420(nv, H, W)
    ctx = vdmi.Context(device=0, precision="fp32", max_batch=STEP)
    ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
    steps = SURFACES // STEP
    # the box set of tools/cellsbench.py and tools/nv12bench.py --modes: the face lists of synth's RGB frames,
    # some 30 a frame (a pass's time follows the boxes, not the pixels under them)
    boxes = [vdmi.DeviceBoxes(STEP, 256, dev) for _ in range(steps)]
    rgb = torch.from_numpy(synth.frames(SCENES, H, W, seed=0)).to(dev)
    for s in range(steps):
        sc = (s * STEP) % SCENES
        ctx.process(rgb[sc:sc + STEP], flags=_lib.VD_PROC_FACES, faces=boxes[s])
    ctx.sync()
    del rgb
    out = torch.empty_like(nv)
    scratch = vdmi.DeviceBoxes(STEP, 256, dev)
    sl = lambda t, s: t[s * STEP:(s + 1) * STEP]

    def calls(case):
        if case == "nv12_old":
            return {"mosaic": lambda s: ctx.mosaic_nv12(sl(nv, s), boxes[s], level=a.level, out=sl(out, s)),
                    "smooth": lambda s: ctx.smooth_nv12(sl(nv, s), boxes[s], level=a.level, cells=a.cells, out=sl(out, s)),
                    "letterbox": lambda s: ctx.process_nv12(sl(nv, s), flags=_lib.VD_PROC_FACES, faces=scratch)}
        src = nv if case == "nv12_new" else i420
        li, lo = ("nv12", "nv12") if case == "nv12_new" else case.split("_")
        return {"mosaic": lambda s: ctx.mosaic_yuv420(sl(src, s), boxes[s], level=a.level, out=sl(out, s), layout=li,
                                                      out_layout=lo),
                "smooth": lambda s: ctx.smooth_yuv420(sl(src, s), boxes[s], level=a.level, cells=a.cells, out=sl(out, s),
                                                      layout=li, out_layout=lo),
                "letterbox": lambda s: ctx.process_yuv420(sl(src, s), flags=_lib.VD_PROC_FACES, faces=scratch, layout=li)}

    r = {"boxes_per_frame": float(sum(int(b.count.clamp(0, 256).sum()) for b in boxes)) / SURFACES, "cases": {}}
    ctx.timing(True)
    for case in (CASES[:1] if parent else CASES):
        row = {}
        for name, call in calls(case).items():
            fam = _lib.FAM_LETTERBOX if name == "letterbox" else _lib.FAM_MOSAIC
            for s in range(steps):   # warm-up: one pass
                call(s)
            ctx.sync()
            ctx.timing_reset()
            for _ in range(a.passes):
                for s in range(steps):
                    call(s)
            ctx.sync()
            t, k, work = ctx.timing_read(fam)
            row[name] = {"ms_per_step": round(t / (a.passes * steps), 5), "launches_per_step": k / (a.passes * steps),
                         "bytes_per_step": work / (a.passes * steps)}
        r["cases"][case] = row
    ctx.timing(False)
    ctx.close()
    print("YUV420BENCH " + json.dumps(r), flush=True)


def child(a, which):
    env = dict(os.environ)
    if which == "parent":
        env["VDMI_LIB"] = os.path.abspath(a.parent_lib)
    else:
        env.pop("VDMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", which, "--passes", str(a.passes), "--level", str(a.level),
           "--cells", str(a.cells)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{which} run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("YUV420BENCH "):
            return json.loads(line[len("YUV420BENCH "):])
    raise RuntimeError(f"{which} run printed no result:\n{p.stdout[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libvdmi.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3, help="passes over the 16 steps behind each figure")
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--cells", type=int, default=16)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one", choices=("parent", "this"), help="(internal) one measurement in this process")
    ap.add_argument("--json", help="also write the result line to this file")
    a = ap.parse_args()
    if a.one:
        return one(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's libvdmi.so is needed for the comparison")
    runs = {"parent": [], "this": []}
    for _ in range(a.repeats):                   # parent, this, parent, this, ...
        for which in ("parent", "this"):
            runs[which].append(child(a, which))  # a failed child raises: nothing more is started
    res = {"what": "family 1 (output pass) and family 2 (letterbox) per 4-frame step over 64 x 1080p device surfaces "
                   "(16 scenes, four times each) and the face lists of synth's RGB frames: NV12 through the *_nv12 entries "
                   "by the parent build and by this build, NV12 / I420 -> I420 / I420 -> NV12 through the *_yuv420 "
                   "entries by this build",
           "machine": "one MI355X, the runs alternating in one session, a process each",
           "frame": [1080, 1920], "step_frames": STEP, "surfaces": SURFACES, "level": a.level, "cells": a.cells,
           "repeats": a.repeats, "passes": a.passes, "boxes_per_frame": runs["this"][0]["boxes_per_frame"]}
    mean = lambda v: round(sum(v) / len(v), 5)
    for p in PASSES:
        par = [r["cases"]["nv12_old"][p]["ms_per_step"] for r in runs["parent"]]
        row = {"parent_nv12_ms": par, "parent_mean_ms": mean(par), "parent_spread_ms": round(max(par) - min(par), 5)}
        for c in CASES:
            v = [r["cases"][c][p]["ms_per_step"] for r in runs["this"]]
            row[c + "_ms"] = v
            row[c + "_mean_ms"] = mean(v)
            row[c + "_minus_parent_ms"] = round(mean(v) - mean(par), 5)
            row[c + "_within_parent_spread"] = bool(mean(v) - mean(par) <= max(par) - min(par))
            row[c + "_launches_per_step"] = runs["this"][0]["cases"][c][p]["launches_per_step"]
        res[p] = row
    res["runs"] = runs
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
