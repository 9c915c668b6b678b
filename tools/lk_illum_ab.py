#!/usr/bin/env python3
"""What the LK tracker's illumination models (option lk_illumination) cost and buy.

cost: the headline step (bench.py's workload: 768 kitti chains of 1241x376 as 2 engines, 5 warm-up
and 30 timed steps, the next pyramid prefetched) with the option off, "bias" and "gain_bias", the
three alternating inside one process for `rounds` rounds; one JSON row per leg (ms per step, frames
per second, chains alive, per-stage event times of group 0) appended to out.jsonl.  With the option
off the launches are those of bench.py; bench.py itself is not touched: its Headline class is built
with the preset's options plus the key.

accuracy: ATE, survival and the tracked / inlier counts against the synthetic ground truth for the
plain tracker and both models, on the rendered frames as they are and under synth.apply_exposure's
schedule.  Seeds 0..3 as the chains of one Engine (the same camera path, four textures), stepped n
frames after the bootstrap; a chain that ends is scored over the poses it produced.

usage: python tools/lk_illum_ab.py cost [rounds] [out.jsonl] [chains] [steps]
       python tools/lk_illum_ab.py accuracy [n_frames] [out.json] [preset ...]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monocular_visual_odometry_va4mr_amd import _lib as L  # noqa: E402
from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: E402
from monocular_visual_odometry_va4mr_amd.ate import ate  # noqa: E402
from monocular_visual_odometry_va4mr_amd.engine import Engine  # noqa: E402
from monocular_visual_odometry_va4mr_amd.evaluation import poses_from_transforms  # noqa: E402
from monocular_visual_odometry_va4mr_amd.synth import Renderer, apply_exposure, poses  # noqa: E402

MODELS = (None, "bias", "gain_bias")


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.4g} [{v.min():.4g} .. {v.max():.4g}]"


def cost(argv):
    import bench
    rounds = int(argv[0]) if argv else 3
    out_path = argv[1] if len(argv) > 1 else None
    B = int(argv[2]) if len(argv) > 2 else 768
    K_steps = int(argv[3]) if len(argv) > 3 else 30
    W_steps, G = 5, 2
    dev = torch.device("cuda")
    get = Op.get
    rows = []
    for r in range(rounds):
        for model in MODELS:
            def patched(preset, model=model):
                opts, boot, last = get(preset)
                if model is not None:
                    opts["lk_illumination"] = model
                return opts, boot, last
            bench.Op.get = patched              # Headline reads the preset's options through bench.Op
            try:
                hl = bench.Headline(dev, "kitti", 1, B, G, 0, 1, W_steps + K_steps)
            finally:
                bench.Op.get = get
            assert all(e.lk_illumination == model for e in hl.engines)
            hl.bootstrap()
            torch.cuda.synchronize()
            hl.release()
            for i in range(W_steps):
                hl.step(2 + i, prefetch=i + 1 < W_steps)
            torch.cuda.synchronize()
            nst = len(Engine.STAGES)
            ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(nst)] for _ in range(K_steps)]
            t0 = time.perf_counter()
            for k in range(K_steps):
                e = ev[k]
                hl.step(2 + W_steps + k, marks=lambda i, end, strm, e=e: e[i][int(end)].record(strm), prefetch=k + 1 < K_steps)
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            n_ok = int((hl.statuses() == 0).sum())
            st_ms = np.zeros(nst)
            for k in range(K_steps):
                for i in range(nst):
                    st_ms[i] += ev[k][i][0].elapsed_time(ev[k][i][1])
            st_ms /= K_steps
            row = {"round": r, "lk_illumination": model, "chains": B, "steps": K_steps, "ms": round(elapsed / K_steps * 1e3, 4),
                   "value": round(n_ok * K_steps / elapsed, 2), "ok": n_ok,
                   "stages": {n: round(float(m), 4) for n, m in zip(Engine.STAGES, st_ms)}}
            rows.append(row)
            print(json.dumps(row), flush=True)
            if out_path:
                with open(out_path, "a") as f:
                    f.write(json.dumps(row) + "\n")
            hl.engines.clear()
            del hl
            torch.cuda.empty_cache()
    print("\nlk_illumination | ms per step | track stage ms (group 0) | chains alive")
    for model in MODELS:
        sel = [r for r in rows if r["lk_illumination"] == model]
        print(f"{model} | {spread([r['ms'] for r in sel])} | {spread([r['stages']['track'] for r in sel])} | "
              f"{spread([r['ok'] for r in sel])}")


def accuracy(argv):
    n = int(argv[0]) if argv else 120
    out_path = argv[1] if len(argv) > 1 else None
    presets = argv[2:] or ["kitti"]
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
        raw = {}
        for c0 in range(0, len(ids), 32):
            chunk = ids[c0:c0 + 32]
            imgs = [r.render_batch(chunk, Rs[chunk], cs[chunk]) for r in rends]
            for j, i in enumerate(chunk):
                raw[i] = torch.stack([im[j] for im in imgs]).contiguous()
        H, W = raw[boot[0]].shape[-2:]
        # frame i of every chain at the exposure of global frame index i
        exposed = {i: apply_exposure(f.reshape(1, B * H, W), start=i)[0].reshape(B, H, W).contiguous() for i, f in raw.items()}
        sat = float(np.mean([float(((f == 0) | (f == 255)).float().mean()) for f in exposed.values()]))
        for sched, fr in (("none", raw), ("exposure", exposed)):
            for model in MODELS:
                o = dict(opts)
                if model is not None:
                    o["lk_illumination"] = model
                eng = Engine(rends[0].K, o, W, H, batch=B, device="cuda", fcap=last + 8)
                eng.bootstrap(fr[boot[0]], fr[boot[1]])
                survived = np.zeros(B, np.int64)
                tracked, inliers = np.zeros(B), np.zeros(B)
                stopped = [None] * B
                for i in range(boot[1] + 1, last):
                    eng.step(fr[i])
                    st = eng.statuses()
                    ninl = eng.t["nInl"].cpu().numpy().astype(np.float64)
                    nout = eng.t["nOutl"].cpu().numpy().astype(np.float64)
                    for b in range(B):
                        if stopped[b] is not None:
                            continue
                        if st[b] != 0:
                            stopped[b] = (i, L.STATUS_NAMES.get(int(st[b]), str(int(st[b]))))
                            continue
                        survived[b] += 1
                        tracked[b] += ninl[b] + nout[b]
                        inliers[b] += ninl[b]
                    if all(s is not None for s in stopped):
                        break
                for b, seed in enumerate(SEEDS):
                    est = poses_from_transforms(eng.export_chain(b)["transforms"])
                    m = min(len(est), len(gt))
                    rmse, rel = ate(est[:m, :, 3], gt[:m, :, 3])
                    k = max(int(survived[b]), 1)
                    row = {"preset": preset, "seed": seed, "frames": n, "schedule": sched, "lk_illumination": model,
                           "saturated_fraction": sat if sched == "exposure" else None,
                           "poses": m, "frames_survived": int(survived[b]), "ate_rmse": rmse, "ate_rel": rel,
                           "mean_tracked": float(tracked[b] / k), "mean_inliers": float(inliers[b] / k)}
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
    print("\npreset schedule model | survived | ATE rmse | ATE rel | tracked | inliers")
    for preset in presets:
        for sched in ("none", "exposure"):
            for model in MODELS:
                sel = [r for r in rows if r["preset"] == preset and r["schedule"] == sched and r["lk_illumination"] == model]
                sp = lambda k: spread([r[k] for r in sel])
                print(f"{preset} {sched} {model} | {sp('frames_survived')} | {sp('ate_rmse')} | {sp('ate_rel')} | "
                      f"{sp('mean_tracked')} | {sp('mean_inliers')}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "accuracy"
    {"cost": cost, "accuracy": accuracy}[mode](sys.argv[2:])
