#!/usr/bin/env python3
"""B copies of one KITTI chain in one engine, stepped eagerly with the sub-pixel corner refinement
on (option feature_subpix_win), for a kernel trace of k_corner_subpix at 1 chain and at 384 chains
per launch (DESIGN 5e's cost figures):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/subpix_prof.py 40 384
usage: python tools/subpix_prof.py [n_frames] [chains] [half-window]"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import torch  # noqa: E402

import bench  # noqa: E402
from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.engine import Engine  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import Renderer  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1
win = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda")
opts, (b0, b1), _ = Op.get("kitti")
gap = b1 - b0
rend = Renderer("kitti", seed=1, device=dev)
gt = bench.StagePoses(n + gap + 8, rend.p)
fr = bench.render_windows(rend, gt, [0], gap, n - 2, dev)[:, 0]
eng = Engine(rend.K, dict(opts, feature_subpix_win=win), fr.shape[-1], fr.shape[-2], batch=B, device=dev,
             ncap=16384 if B == 1 else 4096, pcap=16384 if B == 1 else 8192, fcap=n + 8)
eng.bootstrap(fr[0:1].expand(B, -1, -1), fr[1:2].expand(B, -1, -1))
corners = []
for i in range(2, n):
    eng.step(fr[i:i + 1].expand(B, -1, -1))
    torch.cuda.synchronize()
    corners.append(int(eng.t["nCorners"][0]))
print(f"{B} chains, {n - 2} steps, half-window {win}: corners per chain and step {min(corners)}..{max(corners)}, "
      f"statuses ok {int((eng.statuses() == 0).sum())}/{B}")
