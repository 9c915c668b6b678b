#!/usr/bin/env python3
"""Cost of the lens rectification (engine option dist_coeffs; DESIGN 5i's cost tables), in one process,
timed with HIP events, warm-up discarded, the things compared run alternately:

  remap   vo_remap_u8 alone on B frames through one map, beside vo_pyr_build on the same B frames
          (every kernel of the pyramid build: k_pyr01 / k_pyr_rows and the tail), at each shape; the
          bytes the remap must move (source + destination + map) over 8 TB/s is its floor
  step    the headline step (bench.Headline, KITTI, 2 groups, prefetch) with dist_coeffs = zeros (the
          identity map: one remap launch per step and group, the same frames downstream) against
          the option off, each from its own bootstrap, alternated `reps` times

usage: python tools/undistort_prof.py [out.jsonl] [remap|step ...] [--chains N] [--reps N]"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.engine import Engine  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import SIZES, intrinsics  # noqa: E402

BARREL = [-0.28, 0.07, 2e-4, 2e-5, 0.0]
SHAPES = [(768, "kitti"), (256, "hd1080"), (1, "kitti")]
HBM_BYTES_PER_S = 8e12


def arg(flag, default):
    return int(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def emit(out, row):
    print(json.dumps(row), flush=True)
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        fn(r)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def remap_leg(out, rounds=5):
    dev = torch.device("cuda", 0)
    for B, preset in SHAPES:
        W, H = SIZES[preset]
        opts, _, _ = Op.get(preset)
        eng = Engine(intrinsics(preset), dict(opts, dist_coeffs=BARREL), W, H, batch=B, device=dev, ncap=16, pcap=16, fcap=4)
        g = torch.Generator(device=dev).manual_seed(B)
        raw = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device=dev, generator=g)
        dst = torch.empty_like(raw)
        reps = 10 if B > 1 else 200
        remap = lambda r: eng._remap(raw, dst)
        pyr = lambda r: eng._build_pyramid(dst, r & 1)
        for _ in range(3):                                   # warm-up, discarded
            remap(0)
            pyr(0)
        torch.cuda.synchronize()
        t_remap, t_pyr = [], []
        for _ in range(rounds):
            t_remap.append(timed(remap, reps))
            t_pyr.append(timed(pyr, reps))
        need = 2 * B * W * H + 6 * W * H
        med = float(np.median(t_remap))
        emit(out, {"leg": "remap", "B": B, "W": W, "H": H, "reps": reps, "rounds": rounds,
                   "remap_ms": [round(t, 4) for t in t_remap], "remap_ms_median": round(med, 4),
                   "pyr_build_ms": [round(t, 4) for t in t_pyr], "pyr_build_ms_median": round(float(np.median(t_pyr)), 4),
                   "bytes_needed": need, "floor_ms_at_8TBps": round(need / HBM_BYTES_PER_S * 1e3, 4),
                   "share_of_8TBps": round(need / HBM_BYTES_PER_S * 1e3 / med, 3),
                   "GB_per_s": round(need / (med * 1e-3) / 1e9, 1)})
        del eng, raw, dst
        torch.cuda.empty_cache()


def step_leg(out, chains, reps, steps=30, warmup=5):
    dev = torch.device("cuda", 0)
    n_after = warmup + steps
    get = Op.get
    hls = {}
    for tag, extra in (("off", {}), ("zeros", {"dist_coeffs": [0.0] * 5})):
        def patched(name, extra=extra):
            o, boot, last = get(name)
            o.update(extra)
            return o, boot, last
        bench.Op.get = patched
        try:
            hl = bench.Headline(dev, "kitti", 1, chains, 2, 0, 1, n_after, reserve=False)
        finally:
            bench.Op.get = get
        if hls:
            hl.frames = hls["off"].frames                    # the same frames in HBM, once
        hls[tag] = hl
    assert hls["off"].engines[0].dist is None and hls["zeros"].engines[0].dist is not None
    for rep in range(reps):
        for tag in ("off", "zeros") if rep % 2 == 0 else ("zeros", "off"):
            hl = hls[tag]
            hl.bootstrap()
            torch.cuda.synchronize()
            for i in range(warmup):
                hl.step(2 + i, prefetch=i + 1 < warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                hl.step(2 + warmup + k, prefetch=k + 1 < steps)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            emit(out, {"leg": "step", "variant": tag, "rep": rep, "chains": chains, "steps": steps, "warmup": warmup,
                       "ms_per_step": round(ms, 4), "ok": int((hl.statuses() == 0).sum())})
    # the identity map leaves the chains what they are
    a, b = hls["off"].engines[0], hls["zeros"].engines[0]
    same = all(bool(torch.equal(a.t[k], b.t[k])) for k in ("pose_R", "pose_t", "nL", "nC", "lm_kp"))
    emit(out, {"leg": "step", "identical_state": same})


def main():
    args = [a for a in sys.argv[1:]]
    out = args[0] if args and not args[0].startswith("--") and args[0] not in ("remap", "step") else None
    legs = [a for a in args if a in ("remap", "step")] or ["remap", "step"]
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("undistort_prof.py needs a ROCm GPU")
    if "remap" in legs:
        remap_leg(out)
    if "step" in legs:
        step_leg(out, arg("--chains", 768), arg("--reps", 4))


if __name__ == "__main__":
    main()
