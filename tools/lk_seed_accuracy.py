#!/usr/bin/env python3
"""What the constant-velocity seeding of the landmark tracks (option lk_motion_model)
buys and costs.

accuracy: ATE, RPE, survival and the tracked / inlier counts against the synthetic ground truth with
the option off and on at maxLevel 3, 2 and 1, and the tracking stage's time per step beside them.
Per preset: seeds 0..3 as the chains of one Engine (the same camera path, four textures), stepped n
frames after the bootstrap.  A chain that ends is scored over the poses it produced.

cost: at the headline shape (384 kitti chains of one engine, 1241x376) and on one fixed state per
maxLevel (the state after 4 seeded steps, the next frame's pyramid built): vo_track_lk, the
vo_predict_seeds call and vo_track_seeded, alternating inside one process, device events around each
call; median [min .. max] over the rounds, one JSON row per (maxLevel, call) appended to out.jsonl.

usage: python tools/lk_seed_accuracy.py accuracy [n_frames] [out.json] [preset ...]
       python tools/lk_seed_accuracy.py cost [rounds] [out.jsonl] [chains]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monocular_visual_odometry_va4mr_amd import _lib as L  # noqa: E402
from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.ate import ate  # noqa: E402
from monocular_visual_odometry_va4mr_amd.engine import Engine  # noqa: E402
from monocular_visual_odometry_va4mr_amd.evaluation import poses_from_transforms, rpe  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import Renderer, poses  # noqa: E402

MODEL = "constant_velocity"
LEVELS = (3, 2, 1)


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.4g} [{v.min():.4g} .. {v.max():.4g}]"


def accuracy(argv):
    n = int(argv[0]) if argv else 300
    out_path = argv[1] if len(argv) > 1 else None
    presets = argv[2:] or ["kitti", "malaga", "parking"]
    SEEDS = (0, 1, 2, 3)
    B = len(SEEDS)
    rows = []
    for preset in presets:
        opts, boot, _ = Op.get(preset)
        last = n + boot[1] + 1
        rends = [Renderer(preset, seed=s, device="cuda") for s in SEEDS]
        Rs, cs = poses(last, rends[0].p)
        ids = [boot[0]] + list(range(boot[1], last))
        gt = np.concatenate([Rs[ids], cs[ids][:, :, None]], 2)
        fr = {}
        for c0 in range(0, len(ids), 32):
            chunk = ids[c0:c0 + 32]
            imgs = [r.render_batch(chunk, Rs[chunk], cs[chunk]) for r in rends]
            for j, i in enumerate(chunk):
                fr[i] = torch.stack([im[j] for im in imgs]).contiguous()
        H, W = fr[boot[0]].shape[-2:]
        for level in LEVELS:
            for model in (None, MODEL):
                o = dict(opts, maxLevel=level)
                if model is not None:
                    o["lk_motion_model"] = model
                eng = Engine(rends[0].K, o, W, H, batch=B, device="cuda", fcap=last + 8)
                eng.bootstrap(fr[boot[0]], fr[boot[1]])
                survived = np.zeros(B, np.int64)
                tracked, inliers = np.zeros(B), np.zeros(B)
                totals = np.zeros((B, 4), np.int64)
                stopped = [None] * B
                ev, lk_ms = {}, []

                def marks(i, end, strm):
                    if i == 1:                      # the tracking stage (with the option: seeds + LK)
                        ev[end] = torch.cuda.Event(enable_timing=True)
                        ev[end].record(strm)

                for i in range(boot[1] + 1, last):
                    eng.step(fr[i], marks=marks)
                    st = eng.statuses()
                    lk_ms.append(ev[False].elapsed_time(ev[True]))
                    ninl = eng.t["nInl"].cpu().numpy().astype(np.float64)
                    nout = eng.t["nOutl"].cpu().numpy().astype(np.float64)
                    info = eng.seed_info()
                    for b in range(B):
                        if stopped[b] is not None:
                            continue
                        if st[b] != 0:
                            stopped[b] = (i, L.STATUS_NAMES.get(int(st[b]), str(int(st[b]))))
                            continue
                        survived[b] += 1
                        tracked[b] += ninl[b] + nout[b]
                        inliers[b] += ninl[b]
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
                    k = max(int(survived[b]), 1)
                    row = {"preset": preset, "seed": seed, "frames": n, "maxLevel": level, "lk_motion_model": model,
                           "poses": m, "frames_survived": int(survived[b]), "ate_rmse": rmse, "ate_rel": rel,
                           "rpe1_t": t1, "rpe1_deg": r1, "rpe10_t": t10, "rpe10_deg": r10,
                           "mean_tracked": float(tracked[b] / k), "mean_inliers": float(inliers[b] / k),
                           "track_ms_median": float(np.median(lk_ms)), "track_ms_min": float(np.min(lk_ms)),
                           "track_ms_max": float(np.max(lk_ms)),
                           "seen": None, "seeded": None, "fell_back_depth": None, "fell_back_bounds": None}
                    if model is not None:
                        row.update(zip(("seen", "seeded", "fell_back_depth", "fell_back_bounds"), (int(v) for v in totals[b])))
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
    print("\npreset maxLevel model | survived | ATE rmse | RPE(1) t | RPE(10) t | tracked | inliers | track ms (4 chains)")
    for preset in presets:
        for level in LEVELS:
            for model in (None, MODEL):
                sel = [r for r in rows if r["preset"] == preset and r["maxLevel"] == level and r["lk_motion_model"] == model]
                sp = lambda k: spread([r[k] for r in sel])
                print(f"{preset} {level} {'on' if model else 'off'} | {sp('frames_survived')} | {sp('ate_rmse')} | {sp('rpe1_t')} | "
                      f"{sp('rpe10_t')} | {sp('mean_tracked')} | {sp('mean_inliers')} | {sel[0]['track_ms_median']:.3f} "
                      f"[{sel[0]['track_ms_min']:.3f} .. {sel[0]['track_ms_max']:.3f}]")


def cost(argv):
    import bench
    rounds = int(argv[0]) if argv else 20
    out_path = argv[1] if len(argv) > 1 else None
    B = int(argv[2]) if len(argv) > 2 else 384
    n_after = 5
    dev = torch.device("cuda")
    hl = bench.Headline(dev, "kitti", 1, B, 1, 0, 1, n_after, reserve=False)
    frames, K = hl.frames, hl.K
    hl.engines.clear()
    torch.cuda.empty_cache()
    opts, _, _ = Op.get("kitti")
    rows = []
    for level in LEVELS:
        eng = Engine(K, dict(opts, maxLevel=level, lk_motion_model=MODEL), hl.rend.W, hl.rend.H, batch=B, device=dev,
                     ncap=16384, pcap=16384, fcap=n_after + 16)
        eng.bootstrap(frames[0], frames[1])
        eng.release_bootstrap()
        for j in range(4):
            eng.step(frames[2 + j])
        eng.build_pyramid(frames[6], 1 - eng.prev)
        torch.cuda.synchronize()
        info = eng.seed_info().sum(0)
        lib, pd, po, ps, st = eng.lib, eng._pd, eng._po, eng._ps, eng.stream
        sd, si = C.c_void_p(eng._seeds.data_ptr()), C.c_void_p(eng._seed_info.data_ptr())
        zero = C.c_double(0.0)
        calls = {
            "vo_track_lk": lambda: lib.vo_track_lk(pd, po, ps, eng.prev, st),
            "vo_predict_seeds": lambda: lib.vo_predict_seeds(pd, po, ps, sd, si, st),
            "vo_track_seeded": lambda: lib.vo_track_seeded(pd, po, ps, eng.prev, sd, zero, None, 0, st),
        }
        t = {k: [] for k in calls}
        for r in range(rounds + 2):
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.check(call(), name)
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:                           # two rounds of warm-up
                    t[name].append(e0.elapsed_time(e1) * 1e3)
        n_pts = int(eng.t["nL"].sum()) + int(eng.t["nC"].sum())
        for name, v in t.items():
            row = {"chains": B, "maxLevel": level, "call": name, "rounds": rounds, "points": n_pts,
                   "landmarks": int(eng.t["nL"].sum()), "seed_info_sum": [int(x) for x in info],
                   "us_median": float(np.median(v)), "us_min": float(np.min(v)), "us_max": float(np.max(v))}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del eng
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "accuracy"
    {"accuracy": accuracy, "cost": cost}[mode](sys.argv[2:])
