"""bench.py's --dump-outputs and the split between a plain run and --full.

CPU: dump_outputs on stand-in engines (names, dtypes, masking of dead rows, size budget) and the
command line.  GPU: one tiny plain run of bench.main, twice with the same arguments: the result
line carries the headline keys and none of the --full legs, the dumped arrays are what the stepped
engines hold, and both runs dump identical arrays."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench

LISTS = [n for n, _, _ in bench.DUMP_LISTS]
NAMES = {"poses", "num_pts", *bench.DUMP_COUNTS, *LISTS}


class _Eng:
    """The part of Engine that dump_outputs reads: B and the state tensors."""

    def __init__(self, B, ncap, fcap, seed):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32) + 1.0      # never 0: masking shows
        ri = lambda hi, *s: torch.randint(0, hi, s, generator=g, dtype=torch.int32)
        self.B = B
        self.t = {"lm_X": r(B, ncap, 3), "lm_kp": r(B, ncap, 2), "c_kp": r(B, ncap, 2), "c_first": r(B, ncap, 2),
                  "c_tau": ri(50, B, ncap) + 1, "inl_kp": r(B, ncap, 2), "outl_kp": r(B, ncap, 2),
                  "nL": ri(ncap, B), "nC": ri(ncap, B), "nInl": ri(ncap, B), "nOutl": ri(ncap, B),
                  "status": ri(3, B), "nF": torch.full((B,), fcap - 2, dtype=torch.int32),
                  "num_pts": ri(1000, B, fcap),
                  "pose_R": torch.rand(B, fcap, 9, generator=g, dtype=torch.float64),
                  "pose_t": torch.rand(B, fcap, 3, generator=g, dtype=torch.float64)}


def _packed(engs, fcap):
    return torch.cat([bench.Sh.pack_poses(e.t["pose_R"], e.t["pose_t"], e.t["nF"], fcap) for e in engs])


def test_dump_outputs_names_dtypes_and_masking(tmp_path):
    fcap, ncap = 80, 40                     # more pose slots than DUMP_POSES, lists shorter than DUMP_ROWS
    engs = [_Eng(3, ncap, fcap, 0), _Eng(2, ncap, fcap, 1)]
    shapes = bench.dump_outputs(str(tmp_path / "o"), engs, _packed(engs, fcap))
    files = sorted(os.listdir(tmp_path / "o"))
    assert files == sorted(n + ".npy" for n in NAMES) and set(shapes) == NAMES
    arr = {n: np.load(tmp_path / "o" / (n + ".npy")) for n in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    cat = lambda k: torch.cat([e.t[k] for e in engs]).numpy()
    nF = fcap - 2
    assert arr["poses"].shape == (5, bench.DUMP_POSES, 13) and (arr["poses"][:, :, 12] == 1).all()
    assert np.array_equal(arr["poses"][:, -1, 9:12], cat("pose_t")[:, nF - 1])      # newest pose last
    assert np.array_equal(arr["poses"][:, :, :9], cat("pose_R")[:, nF - bench.DUMP_POSES:nF])
    assert np.array_equal(arr["num_pts"], cat("num_pts")[:, nF - bench.DUMP_POSES:nF])
    for k in bench.DUMP_COUNTS:
        assert np.array_equal(arr[k], cat(k).astype(np.float64))
    for name, key, cnt in bench.DUMP_LISTS:
        src, n = cat(key), cat(cnt)
        assert arr[name].shape == src.shape
        for b in range(5):
            assert np.array_equal(arr[name][b, :n[b]], src[b, :n[b]].astype(np.float32))
            assert not arr[name][b, n[b]:].any()


def test_dump_outputs_stays_under_the_size_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 20000)
    engs = [_Eng(4, 300, 20, 2)]
    bench.dump_outputs(str(tmp_path), engs, _packed(engs, 20))
    total = sum(np.load(tmp_path / f).nbytes for f in os.listdir(tmp_path))
    assert total <= 20000
    rows = np.load(tmp_path / "landmarks.npy").shape[1]
    assert 1 <= rows < 300 and np.load(tmp_path / "cand_tau.npy").shape == (4, rows)


def test_real_budget_is_below_64_mb():
    assert bench.DUMP_BYTES <= 64 * 1000 * 1000


def test_command_line_defaults_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


FULL_ONLY = ("sequence", "seq00_frames_per_s", "single_chain", "cpu_baseline_allcores", "ate_vs_ref",
             "c3_sift_match", "c5_sift_match", "c5_hd1080", "roofline_matcher")


def _run_bench(argv):
    old, buf = sys.argv, io.StringIO()
    sys.argv = ["bench.py"] + argv
    try:
        with contextlib.redirect_stdout(buf):
            bench.main()
    finally:
        sys.argv = old
    return json.loads(buf.getvalue().strip().splitlines()[-1])


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """The same tiny plain run twice (6 chains in 2 stream groups, 1 warm-up + 3 timed steps)."""
    out = []
    for i in range(2):
        d = str(tmp_path_factory.mktemp(f"dump{i}"))
        line = _run_bench(["--gpus", "1", "--chains", "6", "--steps", "3", "--warmup", "1", "--dump-outputs", d])
        out.append((line, {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}, sorted(os.listdir(d))))
        torch.cuda.empty_cache()
    return out


@pytest.mark.gpu
def test_plain_run_result_line(plain_runs):
    line = plain_runs[0][0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["dtype"] == "mixed(u8,i32,f32,f64)"
    assert line["ms_per_step"] > 0
    # value = frames of the chains still tracking / timed seconds, ms_per_step = timed seconds / steps
    assert line["value"] == pytest.approx(line["frames_counted"] / (line["ms_per_step"] * 1e-3 * 3), rel=1e-3)
    assert line["chains_ok"] == 6 and line["frames_counted"] == 18
    assert not [k for k in FULL_ONLY if k in line]
    assert line["headline_vs_reference"] is None and line["cpu_baseline"] is None


@pytest.mark.gpu
def test_dump_is_what_the_last_step_left(plain_runs):
    line, arr, files = plain_runs[0]
    assert files == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64 * 1000 * 1000
    assert line["dumped_outputs"] == {n: list(a.shape) for n, a in arr.items()}
    # the bootstrap leaves its poses, then each of the 1 + 3 steps appends one
    nF = int(arr["nF"][0])
    assert nF >= 5 and (arr["nF"] == nF).all() and (arr["status"] == 0).all()
    assert arr["poses"].shape == (6, nF, 13) and (arr["poses"][:, :, 12] == 1).all()
    R = arr["poses"][:, :, :9].reshape(6, nF, 3, 3)
    assert np.allclose(R @ R.transpose(0, 1, 3, 2), np.eye(3), atol=1e-8)
    # the camera moved in the last step; group 0's live points are the line's points_last_step
    assert (np.abs(arr["poses"][:, -1, 9:12] - arr["poses"][:, -2, 9:12]).max(1) > 0).all()
    assert (arr["nL"] > 0).all() and (arr["num_pts"][:, 1:] > 0).all()
    assert line["points_last_step"] == int(arr["nL"][:3].sum() + arr["nC"][:3].sum())
    for name, _, cnt in bench.DUMP_LISTS:
        n = np.minimum(arr[cnt], arr[name].shape[1]).astype(int)
        for b in range(6):
            assert np.isfinite(arr[name][b]).all() and not arr[name][b, n[b]:].any()
            assert n[b] == 0 or arr[name][b, :n[b]].any()


@pytest.mark.gpu
def test_same_arguments_same_outputs(plain_runs):
    (_, a, _), (_, b, _) = plain_runs
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
