"""NV12 against RGB at the bench shape: 64 synthetic 1080p frames already in HBM (fp32, faces |
plates | mosaic, as bench.py's flagship step), all in one session.

    python tools/nv12bench.py --parent-lib PATH/libvdmi.so [--steps 20] [--warmup 3]
                              [--repeats 3] [--json profiles/nv12_1080p.json]

Kinds, a child process per measurement (a fresh context, a fresh library), alternating, `--repeats`
of each:
    parent   the PARENT commit's build (through VDMI_LIB; the NV12 entry points are not bound),
             Context.process on the RGB frames C(nv12 frames)
    rgb      this build, the same call: (a) must equal `parent` within the parent's own repeat spread,
             in the step time and in family 2 (the refactored letterbox wrappers are on this path)
    nv12     this build, Context.process_nv12 on the NV12 frames: (b) family 1 (the output pass)
             moves half the bytes of the RGB pass, family 2 reads 1.5 instead of 3 B/px of source
    torch    (c, informational, one run) what a caller does without this: a torch NV12 -> RGB and
             RGB -> NV12 round trip around Context.process
Per run: ms/step in the steady state (warm-up first, then the steps ended by one synchronise), then
event-timed steps of their own for the families' times, and for families 1 and 2 the share of the
8 TB/s HBM peak their algorithmic bytes reach.

    python tools/nv12bench.py --modes --parent-lib PATH/libvdmi.so [--repeats 5] [--fam-steps 5]
                              [--level 8] [--cells 16] [--json profiles/nv12_modes_1080p.json]

--modes: the scaled smooth blur and the ellipse mask on NV12 frames. Family 1 of one stand-alone call
(smooth_nv12, mosaic_nv12 under masks ("rect", 0), ("rect", 42), ("ellipse", 42)) over the face lists
detected on the frames -- the boxes tools/cellsbench.py blurs -- beside smooth / mosaic on
nv12_to_rgb of the same frames, by this build and, for the calls it has, by the parent's build: the
median of --repeats groups with their spread. The restore pass alone is the ellipse row minus the
("rect", 42) row of the same call.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))

NV12_ENTRIES = ("vd_process_nv12", "vd_mosaic_nv12", "vd_nv12_to_rgb", "vdt_letterbox_nv12")
KINDS = ("parent", "rgb", "nv12")
HBM_PEAK = 8.0e12
# BT.709 limited, real-valued: the frames only have to be plausible NV12, C() of them is the RGB input
KR, KB = 0.2126, 0.0722


def nv12_frames(B, H, W, dev):
    """Synthetic NV12 frames on the device: synth's RGB scenes through a real-valued forward matrix,
    chroma averaged over 2 x 2, frame by frame."""
    import torch
    from vdmi import synth
    out = torch.empty((B, H * 3 // 2, W), dtype=torch.uint8, device=dev)
    for i in range(B):
        rgb = torch.from_numpy(synth.frames(1, H, W, seed=0, start=i)[0]).to(dev).float()
        y = KR * rgb[..., 0] + (1 - KR - KB) * rgb[..., 1] + KB * rgb[..., 2]
        cb = ((rgb[..., 2] - y) / (2 * (1 - KB))).reshape(H // 2, 2, W // 2, 2).mean(dim=(1, 3))
        cr = ((rgb[..., 0] - y) / (2 * (1 - KR))).reshape(H // 2, 2, W // 2, 2).mean(dim=(1, 3))
        out[i, :H] = (y * (219 / 255) + 16).round().clamp(0, 255).to(torch.uint8)
        uv = torch.stack([cb, cr], dim=-1) * (224 / 255) + 128
        out[i, H:] = uv.round().clamp(0, 255).to(torch.uint8).reshape(H // 2, W)
    return out


def torch_to_rgb(nv, H, W):
    """What a caller writes today (float, full-frame passes): NV12 -> RGB."""
    import torch
    y = (nv[:, :H].float() - 16) * (255 / 219)
    uv = nv[:, H:].reshape(-1, H // 2, W // 2, 2).float() - 128
    uv = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * (255 / 224)
    r = y + 2 * (1 - KR) * uv[..., 1]
    b = y + 2 * (1 - KB) * uv[..., 0]
    g = (y - KR * r - KB * b) / (1 - KR - KB)
    return torch.stack([r, g, b], dim=-1).round().clamp(0, 255).to(torch.uint8)


def torch_to_nv12(rgb, out, H, W):
    import torch
    f = rgb.float()
    y = KR * f[..., 0] + (1 - KR - KB) * f[..., 1] + KB * f[..., 2]
    n = rgb.shape[0]
    cb = ((f[..., 2] - y) / (2 * (1 - KB))).reshape(n, H // 2, 2, W // 2, 2).mean(dim=(2, 4))
    cr = ((f[..., 0] - y) / (2 * (1 - KR))).reshape(n, H // 2, 2, W // 2, 2).mean(dim=(2, 4))
    out[:, :H] = (y * (219 / 255) + 16).round().clamp(0, 255).to(torch.uint8)
    out[:, H:] = (torch.stack([cb, cr], dim=-1) * (224 / 255) + 128).round().clamp(0, 255).to(torch.uint8).reshape(n, H // 2, W)


def one(a):
    """A single measurement in this process: --one parent | rgb | nv12 | torch."""
    import torch
    from vdmi import _lib
    if a.one == "parent":    # the parent's build does not export the NV12 entry points
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NV12_ENTRIES]
    import vdmi
    from vdmi import weights
    B, H, W = a.batch, 1080, 1920
    dev = torch.device("cuda:0")
    nv = nv12_frames(B, H, W, dev)
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC
    ctx = vdmi.Context(device=0, precision="fp32", max_batch=B)
    ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
    ctx.load_weights(_lib.VD_NET_YOLOV8N, weights.yolov8n_state_dict(0))
    faces, plates = vdmi.DeviceBoxes(B, 256, dev), vdmi.DeviceBoxes(B, 256, dev)
    if a.one == "nv12":
        out = torch.empty_like(nv)

        def step():
            ctx.process_nv12(nv, out, faces=faces, plates=plates, flags=flags)
    else:
        # C(nv12 frames) by the header's BT.709 limited table in int32 tensors (arithmetic shifts), frame by
        # frame: the same pixels for every RGB kind (the parent's build has no vd_nv12_to_rgb)
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        for i in range(B):
            uv = nv[i, H:].reshape(H // 2, W // 2, 2).to(torch.int32) - 128
            uv = uv.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
            u, v = uv[..., 0], uv[..., 1]
            tt = 298 * (nv[i, :H].to(torch.int32) - 16) + 128
            px = torch.stack([(tt + 459 * v) >> 8, (tt - 55 * u - 136 * v) >> 8, (tt + 541 * u) >> 8], dim=-1)
            rgb[i] = px.clamp(0, 255).to(torch.uint8)
        out = torch.empty_like(rgb)
        if a.one == "torch":
            back = torch.empty_like(nv)

            def step():
                ctx.process(torch_to_rgb(nv, H, W), out, faces=faces, plates=plates, flags=flags)
                ctx.sync()                         # the torch passes run on torch's stream
                torch_to_nv12(out, back, H, W)
                torch.cuda.synchronize()
        else:
            def step():
                ctx.process(rgb, out, faces=faces, plates=plates, flags=flags)
    torch.cuda.synchronize()
    for _ in range(max(a.warmup, 1)):
        step()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    r = {"ms_per_step": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
         "faces_per_frame": float(faces.count.float().mean().item()),
         "plates_per_frame": float(plates.count.float().mean().item())}
    ctx.timing(True)         # events around every launch slow the step: steps of their own
    ctx.timing_reset()
    for _ in range(a.fam_steps):
        step()
    fam = [ctx.timing_read(f) for f in range(7)]
    r["family_ms_per_step"] = [round(t / a.fam_steps, 4) for t, _, _ in fam]
    for f, name in ((_lib.FAM_MOSAIC, "mosaic"), (_lib.FAM_LETTERBOX, "letterbox")):
        t, launches, work = fam[f]
        r[name + "_ms_per_step"] = round(t / a.fam_steps, 4)
        r[name + "_launches_per_step"] = launches / a.fam_steps
        r[name + "_bytes_per_step"] = work / a.fam_steps
        r[name + "_share_of_peak"] = round(work / (t * 1e-3) / HBM_PEAK, 4) if t > 0 else None
    ctx.timing(False)
    ctx.close()
    print("NV12BENCH " + json.dumps(r), flush=True)


# ---- --modes: the stand-alone blurring passes, smooth and ellipse, NV12 beside RGB -------------------
# (row, call, mask): family 1 of one call over the face lists detected on the frames. The restore pass
# alone is the ("ellipse", 42) row minus the ("rect", 42) row of the same call: the same grown lists,
# the same rectangular pass.
MODE_ROWS = [("rgb_smooth", "smooth", ("rect", 0)), ("rgb_smooth_grow42", "smooth", ("rect", 42)),
             ("rgb_smooth_ellipse42", "smooth", ("ellipse", 42)),
             ("rgb_mosaic_grow42", "mosaic", ("rect", 42)), ("rgb_mosaic_ellipse42", "mosaic", ("ellipse", 42)),
             ("nv12_mosaic", "mosaic_nv12", ("rect", 0)), ("nv12_mosaic_grow42", "mosaic_nv12", ("rect", 42)),
             ("nv12_mosaic_ellipse42", "mosaic_nv12", ("ellipse", 42)),
             ("nv12_smooth", "smooth_nv12", ("rect", 0)), ("nv12_smooth_grow42", "smooth_nv12", ("rect", 42)),
             ("nv12_smooth_ellipse42", "smooth_nv12", ("ellipse", 42))]
PARENT_LACKS = ("nv12_mosaic_ellipse42", "nv12_smooth", "nv12_smooth_grow42", "nv12_smooth_ellipse42")
RESTORE = {"rgb_smooth": ("rgb_smooth_ellipse42", "rgb_smooth_grow42"),
           "rgb_mosaic": ("rgb_mosaic_ellipse42", "rgb_mosaic_grow42"),
           "nv12_mosaic": ("nv12_mosaic_ellipse42", "nv12_mosaic_grow42"),
           "nv12_smooth": ("nv12_smooth_ellipse42", "nv12_smooth_grow42")}


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else (s[len(s) // 2 - 1] + s[len(s) // 2]) / 2


def one_modes(a):
    """--one modes-parent | modes-this: every row this library has, one context, the same boxes."""
    import torch
    from vdmi import _lib
    parent = a.one == "modes-parent"
    if parent:               # the parent's build has no vd_smooth_nv12
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] != "vd_smooth_nv12"]
    import vdmi
    from vdmi import synth, weights
    B, H, W = a.batch, 1080, 1920
    dev = torch.device("cuda:0")
    nv = nv12_frames(B, H, W, dev)
    rgb = torch.from_numpy(vdmi.nv12_to_rgb(nv.cpu())).to(dev)
    ctx = vdmi.Context(device=0, precision="fp32", max_batch=B)
    ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
    boxes = vdmi.DeviceBoxes(B, 256, dev)
    # the box set of tools/cellsbench.py: the face lists of its RGB frames (a pass's time follows the boxes, not the pixels)
    ctx.process(torch.from_numpy(synth.frames(B, H, W, seed=0)).to(dev), flags=_lib.VD_PROC_FACES, faces=boxes)
    ctx.sync()
    cnt = boxes.count.cpu().numpy().clip(0, 256)
    xy = boxes.xyxy.cpu().numpy()
    area = sum(max(0, min(W, int(b[2])) - max(0, int(b[0]))) * max(0, min(H, int(b[3])) - max(0, int(b[1])))
               for f in range(B) for b in xy[f, :cnt[f]])
    out_rgb, out_nv = torch.empty_like(rgb), torch.empty_like(nv)
    calls = {"smooth": lambda: ctx.smooth(rgb, boxes, level=a.level, cells=a.cells, out=out_rgb),
             "mosaic": lambda: ctx.mosaic(rgb, boxes, level=a.level, out=out_rgb),
             "mosaic_nv12": lambda: ctx.mosaic_nv12(nv, boxes, level=a.level, out=out_nv),
             "smooth_nv12": lambda: ctx.smooth_nv12(nv, boxes, level=a.level, cells=a.cells, out=out_nv)}
    r = {"boxes_per_frame": float(cnt.sum()) / B, "box_pixels_per_frame": area / B, "rows": {}}
    ctx.timing(True)
    for name, call, mask in MODE_ROWS:
        if parent and name in PARENT_LACKS:
            continue
        ctx.set_mask(*mask)
        step = calls[call]
        for _ in range(max(a.warmup, 1)):
            step()
        ctx.sync()
        ms, launches = [], 0
        for _ in range(a.repeats):
            ctx.timing_reset()
            for _ in range(a.fam_steps):
                step()
            ctx.sync()
            t, k, _ = ctx.timing_read(_lib.FAM_MOSAIC)
            ms.append(round(t / a.fam_steps, 4))
            launches = k / a.fam_steps
        r["rows"][name] = {"fam1_ms_per_call": ms, "median_ms": round(median(ms), 4),
                           "spread_ms": round(max(ms) - min(ms), 4), "launches_per_call": launches}
    ctx.timing(False)
    ctx.close()
    print("NV12BENCH " + json.dumps(r), flush=True)


def modes(a):
    """The smooth and ellipse passes on NV12 frames beside their RGB counterparts and the parent build."""
    res = {"what": "family 1 (the blurring pass) of one stand-alone call on 64 x 1080p frames in HBM over the face "
                   "lists detected on them: smooth / mosaic on nv12_to_rgb(frames), smooth_nv12 / mosaic_nv12 on the "
                   "NV12 frames; *_grow42 is mask ('rect', 42), *_ellipse42 mask ('ellipse', 42), restore_ms their "
                   "difference of medians (the restore pass alone)",
           "machine": "one MI355X, parent and this build in one session, a process each",
           "batch": a.batch, "frame": [1080, 1920], "level": a.level, "cells": a.cells, "repeats": a.repeats,
           "fam_steps": a.fam_steps}
    for which in ("modes-parent", "modes-this"):
        r = child(a, which)
        for k, (e, g) in RESTORE.items():
            if e in r["rows"] and g in r["rows"]:
                r.setdefault("restore_ms", {})[k] = round(r["rows"][e]["median_ms"] - r["rows"][g]["median_ms"], 4)
        res[which.split("-")[1]] = r
    t = res["this"]["rows"]
    res["nv12_over_rgb"] = {k: round(t["nv12_" + k]["median_ms"] / t["rgb_" + k]["median_ms"], 4)
                            for k in ("smooth", "smooth_grow42", "smooth_ellipse42", "mosaic_grow42", "mosaic_ellipse42")}
    return res


# ---- --tiles: tiled detection on 4:2:0 surfaces at 4K ------------------------------------------------
TILES_NEW = ("vd_tiles_surfaces", "vdt_letterbox_tiles_nv12", "vdt_letterbox_tiles_yuv420", "vdt_letterbox_tiles_yuv420_16",
             "vdt_plate_raw_tiles_yuv420")
TILES_ROWS = ("rgb_tiled", "nv12", "i420", "p010", "nv12_tiled", "i420_tiled", "p010_tiled")


def one_tiles(a):
    """--one tiles-parent | tiles-this: every row this library has; an untiled and a tiled context."""
    import torch
    from vdmi import _lib
    parent = a.one == "tiles-parent"
    if parent:               # the parent's build has neither the switch nor the surface tile hooks
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in TILES_NEW]
    import vdmi
    from vdmi import weights
    B, H, W = 4, 2160, 3840
    dev = torch.device("cuda:0")
    nv = nv12_frames(B, H, W, dev)
    host = nv.cpu().numpy()
    rgb = torch.from_numpy(vdmi.nv12_to_rgb(host)).to(dev)
    planes = host[:, H:].reshape(B, H // 2, W // 2, 2)
    i420 = torch.from_numpy(host.copy()).to(dev)
    i420[:, H:] = torch.from_numpy(planes.transpose(0, 3, 1, 2).copy().reshape(B, H // 2, W)).to(dev)
    p010 = (nv.to(torch.int16) << 8)                       # 10 bits at shift 6: the 8-bit picture is nv
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC
    ctxs = {}
    for tiled in (False, True):
        kw = dict(tiles=(2, 2), tile_overlap=20) if tiled else {}
        if tiled and not parent:
            kw["tile_surfaces"] = True
        c = vdmi.Context(device=0, precision="fp32", max_batch=20, **kw)
        c.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
        c.load_weights(_lib.VD_NET_YOLOV8N, weights.yolov8n_state_dict(0))
        ctxs[tiled] = c
    faces, plates = vdmi.DeviceBoxes(B, 256, dev), vdmi.DeviceBoxes(B, 256, dev)
    out = {"rgb": torch.empty_like(rgb), "nv12": torch.empty_like(nv), "i420": torch.empty_like(i420), "p010": torch.empty_like(p010)}
    kw = dict(faces=faces, plates=plates, flags=flags)
    calls = {"rgb": lambda c: c.process(rgb, out["rgb"], **kw), "nv12": lambda c: c.process_nv12(nv, out["nv12"], **kw),
             "i420": lambda c: c.process_yuv420(i420, out["i420"], layout="i420", **kw),
             "p010": lambda c: c.process_yuv420_16(p010, out["p010"], layout="nv12", depth=10, shift=6, **kw)}
    torch.cuda.synchronize()
    r = {"rows": {}}
    for name in TILES_ROWS:
        tiled = name.endswith("_tiled")
        if parent and tiled and name != "rgb_tiled":
            continue
        ctx, step = ctxs[tiled], calls[name.split("_")[0]]
        for _ in range(max(a.warmup, 1)):
            step(ctx)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step(ctx)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        ctx.timing(True)
        ctx.timing_reset()
        for _ in range(a.fam_steps):
            step(ctx)
        ctx.sync()
        t, launches, work = ctx.timing_read(_lib.FAM_LETTERBOX)
        ctx.timing(False)
        r["rows"][name] = {"ms_per_step": round(ms, 3), "letterbox_ms_per_step": round(t / a.fam_steps, 4),
                           "letterbox_launches_per_step": launches / a.fam_steps,
                           "letterbox_bytes_per_step": work / a.fam_steps,
                           "faces_per_frame": float(faces.count.float().mean().item())}
    for c in ctxs.values():
        c.close()
    print("NV12BENCH " + json.dumps(r), flush=True)


def tiles(a):
    import numpy as np
    import vdmi
    runs = {"parent": [], "this": []}
    for _ in range(a.repeats):                   # parent, this, parent, this, ...
        for which in ("parent", "this"):
            runs[which].append(child(a, "tiles-" + which)["rows"])
    col = lambda k, row, key: [r[row][key] for r in runs[k] if row in r]
    mean = lambda v: round(sum(v) / len(v), 4)
    res = {"what": "4-frame steps of 3840x2160 device frames (faces | plates | mosaic, fp32, max_batch 20); *_tiled: tiles "
                   "(2, 2, 20) on the face net; nv12 / i420 / p010: surfaces, rgb: the converted frames; letterbox: "
                   "timing family 2, event-timed in steps of their own",
           "machine": "one MI355X, parent and this build alternating in one session, a process each",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "fam_steps": a.fam_steps, "rows": {}}
    for row in TILES_ROWS:
        e = {}
        for k in ("parent", "this"):
            for key in ("ms_per_step", "letterbox_ms_per_step"):
                v = col(k, row, key)
                if v:
                    e[f"{k}_{key}"] = v
                    e[f"{k}_{key}_mean"] = mean(v)
                    e[f"{k}_{key}_spread"] = round(max(v) - min(v), 4)
        b = col("this", row, "letterbox_bytes_per_step")
        e["letterbox_bytes_per_step"] = b[0] if b else None
        e["faces_per_frame"] = col("this", row, "faces_per_frame")[0]
        if "parent_ms_per_step_mean" in e:       # (a): this build minus the parent, beside the parent's own spread
            e["this_minus_parent_ms"] = round(e["this_ms_per_step_mean"] - e["parent_ms_per_step_mean"], 4)
        res["rows"][row] = e
    t = res["rows"]
    res["tiled_surface_over_tiled_rgb"] = {   # (b)
        k: {"step": round(t[k + "_tiled"]["this_ms_per_step_mean"] / t["rgb_tiled"]["this_ms_per_step_mean"], 4),
            "letterbox": round(t[k + "_tiled"]["this_letterbox_ms_per_step_mean"] /
                               t["rgb_tiled"]["this_letterbox_ms_per_step_mean"], 4)} for k in ("nv12", "i420", "p010")}
    nv = np.random.default_rng(0).integers(0, 256, (4, 2160 * 3 // 2, 3840), dtype=np.uint8)
    t0 = time.perf_counter()                     # (c)
    vdmi.nv12_to_rgb(nv)
    res["host_nv12_to_rgb_4x4k_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["staging_from_16B_rounded_down_address"] = (
        "not tried: at 3840x2160 the tile origins of (2, 2, 20) and (3, 3, 15) (x0 = 1536; 1184 and 2368) are multiples of 16, so "
        "their rows are staged with 16-B loads already; unaligned origins are staged byte-wise, as the RGB tile rows are (unmeasured)")
    return res


def child(a, which):
    env = dict(os.environ)
    if which in ("parent", "modes-parent", "tiles-parent"):
        env["VDMI_LIB"] = os.path.abspath(a.parent_lib)
    else:
        env.pop("VDMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", which, "--steps", str(a.steps), "--warmup",
           str(a.warmup), "--batch", str(a.batch), "--fam-steps", str(a.fam_steps), "--repeats", str(a.repeats),
           "--level", str(a.level), "--cells", str(a.cells)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{which} run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("NV12BENCH "):
            return json.loads(line[len("NV12BENCH "):])
    raise RuntimeError(f"{which} run printed no result:\n{p.stdout[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libvdmi.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fam-steps", type=int, default=5, help="event-timed steps behind the family figures")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--no-torch", action="store_true", help="skip the informational torch round trip")
    ap.add_argument("--tiles", action="store_true", help="tiled detection on 4:2:0 surfaces at 4K instead of the full step")
    ap.add_argument("--one", choices=KINDS + ("torch", "modes-parent", "modes-this", "tiles-parent", "tiles-this"),
                    help="(internal) one measurement in this process")
    ap.add_argument("--modes", action="store_true", help="the smooth and ellipse passes instead of the full step")
    ap.add_argument("--level", type=int, default=8, help="--modes: the base level")
    ap.add_argument("--cells", type=int, default=16, help="--modes: cells of the smooth blur")
    ap.add_argument("--json", help="also write the result line to this file")
    a = ap.parse_args()
    if a.one:
        return one_tiles(a) if a.one.startswith("tiles-") else one_modes(a) if a.one.startswith("modes-") else one(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's libvdmi.so is needed for the comparison")
    if a.modes or a.tiles:
        line = json.dumps(tiles(a) if a.tiles else modes(a))
        print(line, flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                f.write(line + "\n")
        return
    runs = {k: [] for k in KINDS}
    for _ in range(a.repeats):                   # parent, rgb, nv12, parent, rgb, nv12, ...
        for which in KINDS:
            runs[which].append(child(a, which))  # a failed child raises: nothing more is started
    torch_run = None if a.no_torch else child(a, "torch")
    mean = lambda v: round(sum(v) / len(v), 4)
    col = lambda k, key: [r[key] for r in runs[k]]
    res = {"what": "NV12 against RGB: process on C(frames) by the parent build and by this build, process_nv12 on "
                   "the NV12 frames by this build",
           "machine": "one MI355X, the runs alternating in one session, a process each",
           "batch": a.batch, "frame": [1080, 1920], "precision": "fp32", "steps": a.steps, "warmup": a.warmup,
           "hbm_peak_bytes_per_s": HBM_PEAK}
    for k in KINDS:
        res[k + "_ms_per_step"] = col(k, "ms_per_step")
        res[k + "_mean"] = mean(col(k, "ms_per_step"))
        for fam in ("mosaic", "letterbox"):
            res[f"{k}_{fam}_ms"] = col(k, fam + "_ms_per_step")
            res[f"{k}_{fam}_mean"] = mean(col(k, fam + "_ms_per_step"))
            res[f"{k}_{fam}_share_of_peak"] = col(k, fam + "_share_of_peak")
    res["parent_spread_ms"] = round(max(res["parent_ms_per_step"]) - min(res["parent_ms_per_step"]), 3)
    res["rgb_minus_parent_ms"] = round(res["rgb_mean"] - res["parent_mean"], 3)
    res["parent_letterbox_spread_ms"] = round(max(res["parent_letterbox_ms"]) - min(res["parent_letterbox_ms"]), 4)
    res["rgb_minus_parent_letterbox_ms"] = round(res["rgb_letterbox_mean"] - res["parent_letterbox_mean"], 4)
    res["nv12_minus_rgb_ms"] = round(res["nv12_mean"] - res["rgb_mean"], 3)
    res["nv12_over_rgb_mosaic"] = round(res["nv12_mosaic_mean"] / res["rgb_mosaic_mean"], 4)
    res["nv12_over_rgb_letterbox"] = round(res["nv12_letterbox_mean"] / res["rgb_letterbox_mean"], 4)
    res["torch_round_trip"] = torch_run
    res.update({k + "_runs": runs[k] for k in KINDS})
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
