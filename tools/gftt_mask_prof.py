#!/usr/bin/env python3
"""vo_gftt against vo_gftt_masked on B copies of one KITTI-size frame, with the mask a KLT front end
passes (a disc of feature_min_dist around every second corner of the unmasked run): wall time per call
from HIP events, and, under a kernel trace, the eigen pass and the selection kernel by kernel (DESIGN
5f's cost figures):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/gftt_mask_prof.py 384
usage: python tools/gftt_mask_prof.py [chains] [repetitions]"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.engine import Engine  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import make_sequence  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
fr, K, _, _ = make_sequence("kitti", 1, seed=1)
img = fr[0]
H, W = img.shape
opts, _, _ = Op.get("kitti")
eng = Engine(K, opts, W, H, batch=B, ncap=64, pcap=64, fcap=4)
eng.build_pyramid(torch.from_numpy(img).cuda()[None].expand(B, -1, -1), 0)
lib, st = eng.lib, eng.stream


def plain():
    return lib.vo_gftt(eng._pd, eng._po, eng._ps, 0, st)


assert plain() == 0
torch.cuda.synchronize()
n0 = int(eng.t["nCorners"][0])
pts = eng.t["corners"][0, :n0].cpu().numpy()[::2]
r = float(opts["feature_min_dist"])
m = np.full((H, W), 255, np.uint8)
yy, xx = np.mgrid[0:H, 0:W]
for x, y in pts:
    x0, x1, y0, y1 = max(int(x - r), 0), min(int(x + r) + 1, W), max(int(y - r), 0), min(int(y + r) + 1, H)
    sub = (xx[y0:y1, x0:x1] - x) ** 2 + (yy[y0:y1, x0:x1] - y) ** 2 <= r * r
    m[y0:y1, x0:x1][sub] = 0
d_m = torch.from_numpy(m).cuda()[None].expand(B, -1, -1).contiguous()
mp = C.c_void_p(d_m.data_ptr())


def masked():
    return lib.vo_gftt_masked(eng._pd, eng._po, eng._ps, 0, mp, W * H, W, st)


def timed(fn):
    for _ in range(3):
        assert fn() == 0
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert fn() == 0
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms)), int(eng.t["nCorners"][0]), int(eng.t["gf_n"][0])


for name, fn in (("vo_gftt", plain), ("vo_gftt_masked", masked), ("vo_gftt", plain), ("vo_gftt_masked", masked)):
    med, lo, hi, n, keys = timed(fn)
    print(f"{B} chains  {name:15s} median {med:.4f} ms  (min {lo:.4f}, max {hi:.4f}; {reps} calls)  "
          f"corners {n}  keys past the quality gate {keys}  masked-out pixels {int((m == 0).sum())}", flush=True)
