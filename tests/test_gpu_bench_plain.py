"""A plain `python bench.py --gpus 1 --steps K --warmup W` run: the headline only (every field that
`--full` measures is null), K timed steps, and with `--dump-outputs DIR` the frame of the last timed
step in DIR/frame.npy, checked against the CPU oracle.  Ragged tiles (96 x 96 in 64 x 64 tiles).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

RES, SPP, DEPTH, STEPS = 96, 4, 4, 3


def _oracle_sums(oracle_scene, cornell, spp):
    cam = cornell[1].convert_to_taichi_camera().packed()
    return oracle_scene.render(cam, RES, RES, spp, DEPTH, seed=0).astype(np.float64)


@pytest.mark.parametrize("frames_per_launch", [1, 0])
def test_plain_run_is_lean_and_dumps_the_last_timed_frame(tmp_path, oracle_scene, cornell, frames_per_launch):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--res", str(RES),
           "--spp", str(SPP), "--depth", str(DEPTH), "--frames-per-launch", str(frames_per_launch),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - RES * RES * SPP / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * line["value"]
    for k in ("roofline", "work_per_sample", "work_totals", "cpu_baseline", "cpu_numpy", "l2_vs_cpu", "single_frame"):
        assert line[k] is None, k
    assert sorted(os.listdir(out)) == ["frame.npy"]
    frame = np.load(out / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (RES, RES, 3)
    if frames_per_launch == 1:
        # every step renders samples 0 .. spp-1: the oracle's frame, bit for bit
        assert line["config"]["frames_per_launch"] == 1
        assert np.array_equal(frame, _oracle_sums(oracle_scene, cornell, SPP).astype(np.float32))
    else:
        # one launch of STEPS progressive frames: the last one holds samples (STEPS-1)*spp .. STEPS*spp-1,
        # the difference of two oracle prefix sums.  Radiance is non-negative and every f32 addition
        # is off by at most 2^-24 of a partial sum <= the longer prefix sum: STEPS*spp + (STEPS-1)*spp
        # additions in the two prefixes and spp in the frame itself.
        assert line["config"]["frames_per_launch"] == STEPS
        hi = _oracle_sums(oracle_scene, cornell, STEPS * SPP)
        lo = _oracle_sums(oracle_scene, cornell, (STEPS - 1) * SPP)
        bound = 2 * STEPS * SPP * 2.0 ** -24 * hi
        err = np.abs(frame.astype(np.float64) - (hi - lo))
        print("max err", err.max(), "max bound", bound.max())
        assert (hi >= 0).all() and (err <= bound).all(), float((err - bound).max())
