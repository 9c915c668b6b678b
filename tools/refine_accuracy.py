#!/usr/bin/env python3
"""ATE and RPE of one chain against the synthetic ground truth with the PnP pose refinement off
and on (option pnp_refine_iters; DESIGN 5d's accuracy table).  One chain through the drop-in
class per (preset, iterations); a chain that raises (PnP failed, too few keypoints) is scored
over the poses it produced, with the frame it stopped at.
usage: python tools/refine_accuracy.py [n_frames] [out.json]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.ate import ate  # noqa: E402
from monocular_visual_odometry_va4mr_amd.evaluation import poses_from_transforms, rpe  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import Renderer, poses  # noqa: E402
from monocular_visual_odometry_va4mr_amd.VisualOdometryPipeLine import VisualOdometryPipeLine  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rows = []
for preset in ("kitti", "malaga", "parking"):
    opts, boot, _ = Op.get(preset)
    last = n + boot[1] + 1
    rend = Renderer(preset, seed=1, device="cuda")
    Rs, cs = poses(last, rend.p)
    ids = [boot[0]] + list(range(boot[1], last))
    gt = np.concatenate([Rs[ids], cs[ids][:, :, None]], 2)
    frame = lambda i: rend.render_batch([i], Rs[i:i + 1], cs[i:i + 1])[0]
    for iters in (0, 5, 10):
        row = {"preset": preset, "frames": n, "pnp_refine_iters": iters}
        vo = VisualOdometryPipeLine(rend.K, dict(opts, pnp_refine_iters=iters), max_frames=last + 8)
        vo.initialization(frame(boot[0]), frame(boot[1]))
        costs = []
        for i in range(boot[1] + 1, last):
            try:
                vo.continuous_operation(frame(i))
            except Exception as e:
                row["stopped_at_frame"] = i
                row["error"] = f"{type(e).__name__}: {e}"
                break
            if iters:
                costs.append(vo._eng.refine_info()[0])
        est = poses_from_transforms(vo.transforms)
        m = min(len(est), len(gt))
        rmse, rel = ate(est[:m, :, 3], gt[:m, :, 3])
        t1, r1 = rpe(est[:m], gt[:m], 1)
        t10, r10 = rpe(est[:m], gt[:m], 10)
        row.update(poses=m, ate_rmse=rmse, ate_rel=rel, rpe1_t=t1, rpe1_deg=r1, rpe10_t=t10, rpe10_deg=r10)
        if costs:
            c = np.array(costs)
            ran = np.isfinite(c[:, 2])                # a start with a point at z <= 0 is left alone (+inf)
            row.update(median_iterations=float(np.median(c[:, 0])), max_iterations=float(c[:, 0].max()),
                       failed_starts=int((~ran).sum()),
                       median_cost_ratio=float(np.median(c[ran, 3] / c[ran, 2])) if ran.any() else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(rows, f, indent=1)
