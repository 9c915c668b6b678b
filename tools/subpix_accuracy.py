#!/usr/bin/env python3
"""ATE / path length of one chain against the synthetic ground truth with the sub-pixel corner
refinement off and on (option feature_subpix_win 3 and 5; DESIGN 5e's accuracy table), for the three
presets and seeds 0-7, so that the on/off difference can be set beside the seed-to-seed spread.
One chain through the drop-in class per (preset, seed, half-window); a chain that raises (PnP
failed, too few keypoints) is scored over the poses it produced, with the frame it stopped at.
usage: python tools/subpix_accuracy.py [out.json] [kitti/malaga frames] [parking frames]
Writes profiles/subpix/accuracy.json by default."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.ate import ate  # noqa: E402
from monocular_visual_odometry_va4mr_amd.evaluation import poses_from_transforms  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import Renderer, poses  # noqa: E402
from monocular_visual_odometry_va4mr_amd.VisualOdometryPipeLine import VisualOdometryPipeLine  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "subpix", "accuracy.json")
n_long = int(sys.argv[2]) if len(sys.argv) > 2 else 300
n_park = int(sys.argv[3]) if len(sys.argv) > 3 else 100
SEEDS = list(range(8))
WINS = (None, 3, 5)
rows = []
for preset in ("kitti", "malaga", "parking"):
    opts, boot, _ = Op.get(preset)
    n = n_park if preset == "parking" else n_long
    last = n + boot[1] + 1
    for seed in SEEDS:
        rend = Renderer(preset, seed=seed, device="cuda")
        Rs, cs = poses(last, rend.p)
        ids = [boot[0]] + list(range(boot[1], last))
        gt = np.concatenate([Rs[ids], cs[ids][:, :, None]], 2)
        fr = [rend.render_batch(list(range(a, min(last, a + 8))), Rs[a:a + 8], cs[a:a + 8]) for a in range(0, last, 8)]
        frame = lambda i: fr[i // 8][i % 8]
        for win in WINS:
            row = {"preset": preset, "seed": seed, "frames": n, "feature_subpix_win": win}
            o = dict(opts) if win is None else dict(opts, feature_subpix_win=win)
            vo = VisualOdometryPipeLine(rend.K, o, max_frames=last + 8)
            vo.initialization(frame(boot[0]), frame(boot[1]))
            for i in range(boot[1] + 1, last):
                try:
                    vo.continuous_operation(frame(i))
                except Exception as e:
                    row["stopped_at_frame"] = i
                    row["error"] = f"{type(e).__name__}: {e}"
                    break
            est = poses_from_transforms(vo.transforms)
            m = min(len(est), len(gt))
            rmse, rel = ate(est[:m, :, 3], gt[:m, :, 3])
            row.update(poses=m, ate_rmse=float(rmse), ate_rel=float(rel), landmarks=int(vo.num_pts[-1]) if vo.num_pts else 0)
            rows.append(row)
            print(json.dumps(row), flush=True)
summary = {}
for preset in ("kitti", "malaga", "parking"):
    off = np.array([r["ate_rel"] for r in rows if r["preset"] == preset and r["feature_subpix_win"] is None])
    s = {"seeds": len(off), "off": {"mean": float(off.mean()), "std": float(off.std()), "min": float(off.min()),
                                    "max": float(off.max())}}
    for win in WINS[1:]:
        on = np.array([r["ate_rel"] for r in rows if r["preset"] == preset and r["feature_subpix_win"] == win])
        d = on - off
        s[f"win{win}"] = {"mean": float(on.mean()), "std": float(on.std()), "mean_minus_off": float(d.mean()),
                          "std_of_difference": float(d.std()), "seeds_better": int((d < 0).sum()),
                          "seeds_worse": int((d > 0).sum()), "per_seed_minus_off": [float(v) for v in d]}
    summary[preset] = s
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"tool": "tools/subpix_accuracy.py", "metric": "Umeyama Sim(3) ATE RMSE / ground-truth path length",
               "runs": rows, "summary": summary}, f, indent=1)
print(json.dumps(summary, indent=1))
