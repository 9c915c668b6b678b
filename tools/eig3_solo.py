#!/usr/bin/env python3
"""The GFTT stage alone at the headline's per-group batch: vo_gftt on 384 kitti chains with nothing
else on the GPU, timed with device events.  Run it under `rocprofv3 --kernel-trace` and
tools/trace_by_grid.py for k_eig3's own time at this grid (3,244,032 threads).

usage: eig3_solo.py [chains] [reps]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monocular_visual_odometry_va4mr_amd import options as Op          # noqa: E402
from monocular_visual_odometry_va4mr_amd.engine import Engine          # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import make_sequence    # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 384
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
fr, K, _, _ = make_sequence("kitti", 6, seed=1)
opts, _, _ = Op.get("kitti")
H, W = fr[0].shape
eng = Engine(K, opts, W, H, batch=B, ncap=2048, pcap=2048, fcap=16)
eng.build_pyramid(np.stack([fr[b % len(fr)] for b in range(B)]), 0)
for _ in range(3):
    assert eng.lib.vo_gftt(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
ev[0].record()
for i in range(reps):
    assert eng.lib.vo_gftt(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
    ev[i + 1].record()
torch.cuda.synchronize()
ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
print(json.dumps({"chains": B, "reps": reps, "vo_gftt_ms_median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4),
                  "max": round(ms[-1], 4), "corners_chain0": int(eng.t["nCorners"][0]),
                  "lib": os.path.basename(os.path.dirname(os.path.dirname(os.path.dirname(eng.lib._name))))}))
