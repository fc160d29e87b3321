"""Command-line parsing of the denoiser's flags and the --aov writer (no GPU)."""
import os

import numpy as np
import pytest

from pyrenderer_amd import main as M


def test_defaults_leave_the_denoiser_off():
    a = M.parse([])
    assert a.denoise is False and a.denoise_iterations is None and a.aov is None


def test_denoise_flags_parse():
    a = M.parse(["--samples", "8", "--denoise", "--aov", "aov/"])
    assert a.denoise is True and a.denoise_iterations is None and a.aov == "aov/" and a.samples == 8
    b = M.parse(["--denoise-iterations", "3"])
    assert b.denoise is True and b.denoise_iterations == 3   # the count implies the filter
    assert M.parse(["--denoise-iterations", "0", "--denoise"]).denoise_iterations == 0


@pytest.mark.parametrize("n", ["9", "-1", "x"])
def test_iterations_outside_the_accepted_range_are_a_usage_error(n, capsys):
    with pytest.raises(SystemExit) as e:
        M.parse(["--denoise-iterations", n])
    assert e.value.code == 2
    assert "--denoise-iterations" in capsys.readouterr().err


def test_write_aov_files(tmp_path):
    W, H = 6, 4
    feat = np.zeros((W, H, 8), np.float32)
    feat[..., 0:3] = (0.2, 0.4, 1.0)
    feat[..., 3:6] = (0.0, -1.0, 1.0)
    feat[..., 6] = np.arange(W * H, dtype=np.float32).reshape(W, H)
    paths = M.write_aov(str(tmp_path / "aov"), feat)
    assert [os.path.basename(p) for p in paths] == ["albedo.png", "normal.png", "depth.npy"]
    for p in paths[:2]:
        with open(p, "rb") as fh:
            assert fh.read(8) == b"\x89PNG\r\n\x1a\n"
    depth = np.load(paths[2])
    assert depth.dtype == np.float32 and depth.shape == (W, H) and np.array_equal(depth, feat[..., 6])
    # normal.png holds 0.5 n + 0.5: (0, -1, 1) -> (128, 0, 255)
    import zlib
    raw = open(paths[1], "rb").read()
    i = raw.index(b"IDAT")
    n = int.from_bytes(raw[i - 4:i], "big")
    row = zlib.decompress(raw[i + 4:i + 4 + n])
    assert tuple(row[1:4]) == (128, 0, 255)
