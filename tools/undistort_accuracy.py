#!/usr/bin/env python3
"""ATE and RPE against the synthetic ground truth for a camera with lens distortion (engine option
dist_coeffs; DESIGN 5i's accuracy table).  Per preset, the seeds of tools/seed_spread.py (0..7) as the
chains of one Engine (the same camera path, eight textures), stepped n frames after the bootstrap,
three times:

  pinhole      the ideal pinhole render, option off (what every other table of DESIGN measures)
  raw          the render through a barrel-distorted lens (k1 k2 p1 p2 k3 = -0.28 0.07 2e-4 2e-5 0),
               option off: the frames are taken for pinhole ones
  rectified    the same raw frames with dist_coeffs set

The distorted render only replaces the renderer's per-pixel rays by those of the raw pixels: the
inverse of the lens model at 100 iterations (vo_undistort_points), whose round trip through the
forward model is reported.  A chain that ends is scored over the poses it produced.
usage: python tools/undistort_accuracy.py [n_frames] [out.json] [preset ...]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monocular_visual_odometry_va4mr_amd import _lib as L  # noqa: E402
from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.ate import ate  # noqa: E402
from monocular_visual_odometry_va4mr_amd.engine import Engine  # noqa: E402
from monocular_visual_odometry_va4mr_amd.evaluation import poses_from_transforms, rpe  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import Renderer, poses  # noqa: E402

BARREL = [-0.28, 0.07, 2e-4, 2e-5, 0.0]
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


def lens_rays(K, W, H, dist):
    """Normalised rays of the raw pixels (vo_undistort_points, 100 iterations) and the largest error,
    in pixels, of their way back through the forward model."""
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    grid = torch.stack([u, v], -1).reshape(-1, 2).contiguous().cuda()
    out = torch.empty_like(grid)
    Kc = (C.c_double * 9)(*np.asarray(K, np.float64).ravel())
    dc = (C.c_double * len(dist))(*dist)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().vo_undistort_points(W * H, C.c_void_p(grid.data_ptr()), Kc, dc, len(dist), None, 100,
                                        C.c_void_p(out.data_ptr()), st), "vo_undistort_points")
    x, y = out[:, 0], out[:, 1]
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
    back = torch.stack([float(K[0, 0]) * xd + float(K[0, 2]), float(K[1, 1]) * yd + float(K[1, 2])], -1)
    err = float((back - grid).abs().max())
    return x.reshape(H, W).contiguous(), y.reshape(H, W).contiguous(), err


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    presets = sys.argv[3:] or ["parking", "kitti"]
    rows = []
    for preset in presets:
        opts, boot, _ = Op.get(preset)
        last = n + boot[1] + 1
        need = [boot[0]] + list(range(boot[1], last))
        frames = {}
        for lens in ("pinhole", "raw"):
            rends = [Renderer(preset, seed=s, device="cuda") for s in SEEDS]
            K, W, H = rends[0].K, rends[0].W, rends[0].H
            if lens == "raw":
                rx, ry, err = lens_rays(K, W, H, BARREL)
                print(json.dumps({"preset": preset, "lens_round_trip_px": err}), flush=True)
                assert np.isfinite(err) and err < 1e-6, err
                for r in rends:
                    r.rx, r.ry = rx, ry
            Rs, cs = poses(last, rends[0].p)
            fr = {}
            for c0 in range(0, len(need), 16):
                chunk = need[c0:c0 + 16]
                imgs = [r.render_batch(chunk, Rs[chunk], cs[chunk]) for r in rends]
                for j, i in enumerate(chunk):
                    fr[i] = torch.stack([im[j] for im in imgs]).contiguous()
            frames[lens] = fr
        gt = np.concatenate([Rs[need], cs[need][:, :, None]], 2)
        B = len(SEEDS)
        for run, lens, o in (("pinhole", "pinhole", dict(opts)), ("raw", "raw", dict(opts)),
                             ("rectified", "raw", dict(opts, dist_coeffs=BARREL))):
            fr = frames[lens]
            eng = Engine(K, o, W, H, batch=B, device="cuda", fcap=last + 8)
            eng.bootstrap(fr[boot[0]], fr[boot[1]])
            survived = np.zeros(B, np.int64)
            stopped = [None] * B
            for i in range(boot[1] + 1, last):
                eng.step(fr[i])
                st = eng.statuses()
                for b in range(B):
                    if stopped[b] is None:
                        if st[b] != 0:
                            stopped[b] = (i, L.STATUS_NAMES.get(int(st[b]), str(int(st[b]))))
                        else:
                            survived[b] += 1
                if all(s is not None for s in stopped):
                    break
            for b, seed in enumerate(SEEDS):
                est = poses_from_transforms(eng.export_chain(b)["transforms"])
                m = min(len(est), len(gt))
                row = {"preset": preset, "run": run, "seed": seed, "frames": n, "poses": m, "frames_survived": int(survived[b]),
                       "ate_rmse": None, "ate_rel": None, "rpe1_t": None, "rpe10_t": None}
                if m >= 3:
                    rmse, rel = ate(est[:m, :, 3], gt[:m, :, 3])
                    row.update(ate_rmse=rmse, ate_rel=rel, rpe1_t=rpe(est[:m], gt[:m], 1)[0])
                    if m > 11:
                        row["rpe10_t"] = rpe(est[:m], gt[:m], 10)[0]
                if stopped[b] is not None:
                    row["stopped_at_frame"], row["error"] = stopped[b]
                rows.append(row)
                print(json.dumps(row), flush=True)
            del eng
            torch.cuda.empty_cache()
            if out_path:
                os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
                with open(out_path, "w") as f:
                    json.dump(rows, f, indent=1)
    # median [min .. max] over the seeds
    print("\npreset run | survived | ATE rmse | ATE rel | RPE(1) t | RPE(10) t")
    for preset in presets:
        for run in ("pinhole", "raw", "rectified"):
            sel = [r for r in rows if r["preset"] == preset and r["run"] == run]

            def sp(k):
                v = np.array([r[k] for r in sel if r[k] is not None], np.float64)
                return "-" if v.size == 0 else f"{np.median(v):.4g} [{v.min():.4g} .. {v.max():.4g}] ({v.size})"
            print(f"{preset} {run} | {sp('frames_survived')} | {sp('ate_rmse')} | {sp('ate_rel')} | {sp('rpe1_t')} | {sp('rpe10_t')}")


if __name__ == "__main__":
    main()
