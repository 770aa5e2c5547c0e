"""bench.py's multi-rank branch (BASELINE config 4) exercised before the
driver's 8-GPU scaling run: two ranks launched by torch.distributed.run on the one
GPU of the test box (--same-device, gloo for the record all-gather), strong scaling
over one list of frames. The all-gathered per-frame box records must equal a
single-rank run over the same list (fp32: per-frame results do not depend on the
batch a frame lands in)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--scaling", "strong", "--frames", "6", "--batch", "6", "--steps", "1", "--warmup", "0", "--no-timing",
          "--compare", "", "--host-pipeline", "0", "--no-cpu-baseline"]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(cmd, out):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run(cmd + ["--records-out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("frames,batch", [(6, 6), (13, 4)])
def test_bench_two_ranks_strong_equals_single_rank(gpu, tmp_path, frames, batch):
    """(13, 4): shards of 7 / 6 frames in batches of 4 through vdmi.dist.process_frames
    (a short last batch on each rank, records padded to 7 rows)."""
    from vdmi.dist import unpack_records
    one = str(tmp_path / "one.npy")
    two = str(tmp_path / "two.npy")
    common = list(COMMON)
    common[common.index("--frames") + 1] = str(frames)
    common[common.index("--batch") + 1] = str(batch)
    _run([sys.executable, "bench.py"] + common, one)
    out = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2",
                "--backend", "gloo", "--same-device"] + common, two)
    assert '"n_gpus": 2' in out
    r1, r2 = unpack_records(np.load(one)), unpack_records(np.load(two))
    assert list(r1) == list(range(frames)) and list(r2) == list(range(frames))
    assert sum(v[3] for v in r1.values()) > 0
    assert r2 == r1


def test_bench_self_launch_two_ranks_equals_single_rank(gpu, tmp_path):
    """`python bench.py --gpus 2` with no torchrun around it starts both ranks itself."""
    from vdmi.dist import unpack_records
    one = str(tmp_path / "one.npy")
    two = str(tmp_path / "two.npy")
    _run([sys.executable, "bench.py"] + COMMON, one)
    out = _run([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--same-device"] + COMMON, two)
    assert '"n_gpus": 2' in out and "gloo all-gather" in out
    r1, r2 = unpack_records(np.load(one)), unpack_records(np.load(two))
    assert list(r2) == list(range(6)) and sum(v[3] for v in r1.values()) > 0
    assert r2 == r1


def test_bench_rccl_world1_equals_no_dist(gpu, tmp_path):
    """The nccl (= RCCL) branch of bench.py -- init_process_group("nccl", device_id=...)
    and all_gather_into_tensor of the box records on the device -- at one rank: the
    gathered records equal the no-dist run's."""
    from vdmi.dist import unpack_records
    one = str(tmp_path / "one.npy")
    rc = str(tmp_path / "rccl.npy")
    _run([sys.executable, "bench.py"] + COMMON, one)
    out = _run([sys.executable, "bench.py", "--gpus", "1", "--force-dist", "--backend", "nccl"] + COMMON, rc)
    assert '"n_gpus": 1' in out and "RCCL all-gather" in out
    r1, r2 = unpack_records(np.load(one)), unpack_records(np.load(rc))
    assert list(r2) == list(range(6)) and sum(v[3] for v in r1.values()) > 0
    assert r2 == r1


def test_bench_plain_line_and_dump_outputs(gpu, tmp_path):
    """A plain run (no --full) prints the headline line alone, with `ms_per_step` over
    exactly --steps steps, and --dump-outputs writes what the last timed step returned
    as float .npy files (<= 64 MB in all) whose box lists equal that step's records."""
    import json
    from vdmi.dist import unpack_records
    rec, dump = str(tmp_path / "one.npy"), tmp_path / "dump"
    out = _run([sys.executable, "bench.py", "--scaling", "strong", "--frames", "6", "--batch", "6", "--steps", "2",
                "--warmup", "0", "--dump-outputs", str(dump)], rec)
    line = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 2 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - 6) < 0.06
    for k in ("roofline", "blur_roofline", "modes", "cpu_baseline", "parity", "host_pipeline", "jpeg_pipeline"):
        assert k not in line, k
    arrs = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump)) if f.endswith(".npy")}
    assert {"frames_row_sums", "frames_sample", "faces_count", "faces_xyxy", "faces_score", "faces_label",
            "plates_count", "plates_xyxy"} <= set(arrs)
    assert all(v.dtype in (np.float32, np.float64) for v in arrs.values())
    assert sum(v.nbytes for v in arrs.values()) <= 64 << 20
    assert arrs["frames_row_sums"].shape == (6, 1080, 3) and arrs["frames_sample"].max() <= 255
    r = unpack_records(np.load(rec))
    assert sum(v[3] for v in r.values()) > 0
    for f in range(6):
        boxes, scores, anchors, count = r[f]
        k = len(boxes)
        assert arrs["faces_count"][f] == count
        assert [tuple(int(v) for v in b) for b in arrs["faces_xyxy"][f, :k]] == boxes
        assert arrs["faces_score"][f, :k].tolist() == scores and arrs["faces_label"][f, :k].astype(int).tolist() == anchors


def test_bench_full_keeps_the_extra_blocks(gpu, tmp_path):
    """--full runs what a plain run leaves out (here: the HIP-event pass with its
    rooflines and one compared precision; the slow legs switched off as before)."""
    import json
    out = _run([sys.executable, "bench.py", "--full", "--batch", "2", "--steps", "1", "--warmup", "0", "--compare", "fp16",
                "--host-pipeline", "0", "--no-cpu-baseline"], str(tmp_path / "one.npy"))
    line = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
    assert line["ms_per_step"] > 0 and line["dtype"] == "fp32"
    assert line["roofline"]["bound"] == "mfma" and line["blur_roofline"]["bound"] == "hbm"
    assert "fp16" in line["modes"] and "fp16_vs_fp32" in line["parity"]


@pytest.mark.parametrize("dist", [False, True])
def test_bench_inflight_records_equal_single_slot(gpu, tmp_path, dist):
    """bench.py --inflight 2 (two contexts taking consecutive steps on their own streams;
    the records of a step are packed, and with --force-dist all-gathered over RCCL, on
    that step's stream): the last step's records (slot 1's) equal a one-slot run's."""
    from vdmi.dist import unpack_records
    one = str(tmp_path / "one.npy")
    two = str(tmp_path / "two.npy")
    common = [c if c != "1" or i != COMMON.index("--steps") + 1 else "2" for i, c in enumerate(COMMON)]
    extra = ["--gpus", "1", "--force-dist", "--backend", "nccl"] if dist else []
    _run([sys.executable, "bench.py"] + extra + common, one)
    out = _run([sys.executable, "bench.py", "--inflight", "2"] + extra + common, two)
    assert '"batches_in_flight": 2' in out
    r1, r2 = unpack_records(np.load(one)), unpack_records(np.load(two))
    assert list(r2) == list(range(6)) and sum(v[3] for v in r1.values()) > 0
    assert r2 == r1
