#!/usr/bin/env python3
"""ATE, RPE, survival, PnP inlier ratio and the triangulation counters against the synthetic ground
truth with the reprojection-error gate on new landmarks off and on (option tri_max_reproj_error;
DESIGN 5g's accuracy table).  Per preset: seeds 0..3 as the chains of one Engine (the same camera
path, four textures), stepped n frames after the bootstrap, once with the gate off and once at the
preset's PnP threshold, at half of it and at 2 px.  A chain that ends (PnP failed, too few
keypoints) is scored over the poses it produced.
usage: python tools/tri_gate_accuracy.py [n_frames] [out.json] [preset ...]"""
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else None
presets = sys.argv[3:] or ["kitti", "malaga", "parking"]
SEEDS = (0, 1, 2, 3)
rows = []
for preset in presets:
    opts, boot, _ = Op.get(preset)
    last = n + boot[1] + 1
    rends = [Renderer(preset, seed=s, device="cuda") for s in SEEDS]
    Rs, cs = poses(last, rends[0].p)
    ids = [boot[0]] + list(range(boot[1], last))
    gt = np.concatenate([Rs[ids], cs[ids][:, :, None]], 2)
    need = [boot[0]] + list(range(boot[1], last))
    fr = {}
    for c0 in range(0, len(need), 32):
        chunk = need[c0:c0 + 32]
        imgs = [r.render_batch(chunk, Rs[chunk], cs[chunk]) for r in rends]
        for j, i in enumerate(chunk):
            fr[i] = torch.stack([im[j] for im in imgs]).contiguous()
    H, W = fr[boot[0]].shape[-2:]
    pnp_err = float(opts["PnP_error"])
    for gate in (None, pnp_err, pnp_err / 2, 2.0):
        o = dict(opts) if gate is None else dict(opts, tri_max_reproj_error=gate)
        eng = Engine(rends[0].K, o, W, H, batch=len(SEEDS), device="cuda", fcap=last + 8)
        eng.bootstrap(fr[boot[0]], fr[boot[1]])
        B = len(SEEDS)
        survived = np.zeros(B, np.int64)
        ratio_sum = np.zeros(B)
        totals = np.zeros((B, 4), np.int64)
        stopped = [None] * B
        for i in range(boot[1] + 1, last):
            eng.step(fr[i])
            st = eng.statuses()
            ninl = eng.t["nInl"].cpu().numpy().astype(np.float64)
            nout = eng.t["nOutl"].cpu().numpy().astype(np.float64)
            info = eng.tri_gate_info()
            for b in range(B):
                if stopped[b] is not None:
                    continue
                if st[b] != 0:
                    stopped[b] = (i, L.STATUS_NAMES.get(int(st[b]), str(int(st[b]))))
                    continue
                survived[b] += 1
                ratio_sum[b] += ninl[b] / max(ninl[b] + nout[b], 1.0)
                if info is not None:
                    totals[b] += info[b]
            if all(s is not None for s in stopped):
                break
        for b, seed in enumerate(SEEDS):
            est = poses_from_transforms(eng.export_chain(b)["transforms"])
            m = min(len(est), len(gt))
            rmse, rel = ate(est[:m, :, 3], gt[:m, :, 3])
            t1, r1 = rpe(est[:m], gt[:m], 1)
            t10, r10 = rpe(est[:m], gt[:m], 10)
            row = {"preset": preset, "seed": seed, "frames": n, "tri_max_reproj_error": gate, "poses": m,
                   "frames_survived": int(survived[b]), "ate_rmse": rmse, "ate_rel": rel, "rpe1_t": t1, "rpe1_deg": r1,
                   "rpe10_t": t10, "rpe10_deg": r10,
                   "mean_inlier_ratio": float(ratio_sum[b] / max(survived[b], 1)),
                   "reached": None, "depth_kept": None, "dropped": None, "appended": None}
            if gate is not None:
                row.update(zip(("reached", "depth_kept", "dropped", "appended"), (int(v) for v in totals[b])))
            if stopped[b] is not None:
                row["stopped_at_frame"], row["error"] = stopped[b]
            rows.append(row)
            print(json.dumps(row), flush=True)
        del eng
        torch.cuda.empty_cache()
        if out_path:
            with open(out_path, "w") as f:
                json.dump(rows, f, indent=1)
# median [min .. max] over the seeds
print("\npreset gate | survived | ATE rmse | RPE(1) t | RPE(10) t | inlier ratio | dropped / reached")
for preset in presets:
    for gate in sorted({r["tri_max_reproj_error"] for r in rows if r["preset"] == preset}, key=lambda g: -1e9 if g is None else -g):
        sel = [r for r in rows if r["preset"] == preset and r["tri_max_reproj_error"] == gate]

        def sp(k):
            v = np.array([r[k] for r in sel], np.float64)
            return f"{np.median(v):.4g} [{v.min():.4g} .. {v.max():.4g}]"
        frac = "-" if gate is None else f"{sum(r['dropped'] for r in sel)} / {sum(r['reached'] for r in sel)}"
        print(f"{preset} {gate} | {sp('frames_survived')} | {sp('ate_rmse')} | {sp('rpe1_t')} | {sp('rpe10_t')} | "
              f"{sp('mean_inlier_ratio')} | {frac}")
