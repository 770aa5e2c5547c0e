"""Cost of the look-ahead hold at the bench shape: Context.process_lead at lead=2 on 64
synthetic 1080p frames already in HBM (fp32, faces | plates | mosaic, as bench.py's flagship
step), against Context.process on the PARENT commit's build, both in one session.

    python tools/leadbench.py --parent-lib PATH/libvdmi.so [--steps 20] [--warmup 3]
                              [--repeats 3] [--json profiles/lead_1080p.json]

Every measurement is a child process of its own (a fresh context, a fresh library: the parent's
build is loaded through VDMI_LIB, where the entry points it lacks are simply not bound), the two
builds alternating, `--repeats` of each. Per run: ms/step in the steady state -- warm-up first,
which also fills the pending ring, then the steps ended by one synchronise; from then on every
process_lead call pushes 64 frames and emits 64. The added work per step is one list launch
(timing family 3) and the device-to-device copy of the `delay` frames that stay pending
(family 4: 2 x delay x 6.2 MB read and written at 1080p), so the step should sit inside the
parent's own repeat spread plus that copy. The seeded noise frames share nothing from one frame
to the next, so nearly every box of the next `lead` frames is led: the heavy case for the list
kernel and for the mosaic behind it (a video leads a box only before a first detection).
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

LEAD_ENTRIES = ("vd_lead", "vd_lead_pending", "vd_process_lead", "vd_lead_lists", "vd_read_lead")


def one(a):
    """A single measurement in this process: --one base (process) or --one lead (process_lead)."""
    import torch
    from vdmi import _lib
    if a.one == "base":      # the parent's build does not export the lead entry points
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in LEAD_ENTRIES]
    import vdmi
    from vdmi import synth, weights
    B, H, W = a.batch, 1080, 1920
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(synth.frames(B, H, W, seed=0)).to(dev)
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC
    lead = a.lead if a.one == "lead" else 0
    ctx = vdmi.Context(device=0, precision="fp32", max_batch=B, **({"lead": lead} if lead else {}))
    ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
    ctx.load_weights(_lib.VD_NET_YOLOV8N, weights.yolov8n_state_dict(0))
    faces, plates = vdmi.DeviceBoxes(B, 256, dev), vdmi.DeviceBoxes(B, 256, dev)
    out = torch.empty((B + lead, H, W, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    emitted = []
    if lead:
        def step():
            emitted.append(len(ctx.process_lead(frames, out, faces=faces, plates=plates, flags=flags)[0]))
    else:
        def step():
            ctx.process(frames, out, faces=faces, plates=plates, flags=flags)
    for _ in range(max(a.warmup, 1)):
        step()
    ctx.sync()
    del emitted[:]
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    r = {"ms_per_step": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
         "faces_per_frame": float(faces.count.float().mean().item())}
    if lead:
        assert emitted == [B] * a.steps, emitted          # the steady state: 64 in, 64 out
        r["led_per_frame"] = float(ctx.read_lead(B, "lead", cap=1).count.mean())
    # families 3 (post: decode, NMS, the list launch) and 4 (other: the ring copy among them) in
    # steps of their own (events around every launch slow the step); the lead run's figures minus
    # the parent's are the list launch and the copy
    ctx.timing(True)
    ctx.timing_reset()
    for _ in range(a.post_steps):
        step()
    for fam, key in ((_lib.FAM_POST, "post"), (_lib.FAM_OTHER, "other")):
        t, launches, _ = ctx.timing_read(fam)
        r[f"{key}_ms_per_step"] = round(t / a.post_steps, 4)
        r[f"{key}_launches_per_step"] = launches / a.post_steps
    ctx.timing(False)
    ctx.close()
    print("LEADBENCH " + json.dumps(r), flush=True)


def child(a, which):
    env = dict(os.environ)
    if which == "base":
        env["VDMI_LIB"] = os.path.abspath(a.parent_lib)
    else:
        env.pop("VDMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", which, "--steps", str(a.steps), "--warmup",
           str(a.warmup), "--batch", str(a.batch), "--lead", str(a.lead), "--post-steps", str(a.post_steps)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{which} run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("LEADBENCH "):
            return json.loads(line[len("LEADBENCH "):])
    raise RuntimeError(f"{which} run printed no result:\n{p.stdout[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libvdmi.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lead", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--post-steps", type=int, default=5, help="event-timed steps behind the family figures")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one", choices=("base", "lead"), help="(internal) one measurement in this process")
    ap.add_argument("--json", help="also write the result line to this file")
    a = ap.parse_args()
    if a.one:
        return one(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's libvdmi.so is needed for the comparison")
    runs = {"base": [], "lead": []}
    for _ in range(a.repeats):                   # parent, this, parent, this, ...
        for which in ("base", "lead"):
            runs[which].append(child(a, which))  # a failed child raises: nothing more is started
    pm = [r["ms_per_step"] for r in runs["base"]]
    lm = [r["ms_per_step"] for r in runs["lead"]]
    delay = a.lead
    frame_mb = 1080 * 1920 * 3 / 1e6
    res = {"what": f"look-ahead hold: process_lead at lead={a.lead} vs process on the parent commit's build",
           "machine": "one MI355X, the runs alternating in one session, a process each",
           "batch": a.batch, "frame": [1080, 1920], "precision": "fp32", "steps": a.steps, "warmup": a.warmup,
           "note": "noise frames: nearly every box of the next `lead` frames is led (heavy case)",
           "parent_process_ms_per_step": pm, "lead_process_lead_ms_per_step": lm,
           "parent_mean": round(sum(pm) / len(pm), 3), "lead_mean": round(sum(lm) / len(lm), 3),
           "difference_ms": round(sum(lm) / len(lm) - sum(pm) / len(pm), 3),
           "parent_spread_ms": round(max(pm) - min(pm), 3),
           "derived_ring_copy_mb_per_step": round(2 * delay * frame_mb, 1),
           "list_launch_ms": round(sum(r["post_ms_per_step"] for r in runs["lead"]) / len(lm)
                                   - sum(r["post_ms_per_step"] for r in runs["base"]) / len(pm), 4),
           "ring_copy_ms": round(sum(r["other_ms_per_step"] for r in runs["lead"]) / len(lm)
                                 - sum(r["other_ms_per_step"] for r in runs["base"]) / len(pm), 4),
           "lead_runs": runs["lead"], "parent_runs": runs["base"]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
