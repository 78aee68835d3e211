#!/usr/bin/env python3
"""Time be_mlp_rollout (BlockRollout / BlockTrainer with backend="fused") against the two-launch path it is an
alternative to, in one session, the arms of a leg taking turns window by window after a warm-up of each.

    python tools/mlp_rollout_time.py [--out profiles/mlp_rollout.json]

(a) us per step of BlockRollout(record_obs=True).run(): fused (be_mlp_rollout launches of min(T, 100) steps)
    against backend="hip" captured into HIP graphs (run()) and eager (run_eager()), at the given (T, N) with
    the 3-layer supervised weights, plus one row with the 2-layer REINFORCE weights.  Wall clock over a window
    of whole horizons closed by one synchronise; every arm has its own env from the same seed.  Beside each
    row the MFMA floor of the fused kernel: tiles x MFMAs per tile x 32 cycles / SIMDs in use at 2.4 GHz.
(b) BlockTrainer.train per iteration, backend="fused" against "hip" (eager and captured), update half
    captured where the rollout is.
(c) The fused kernel's instances against each other through BALLENV_MLP_ROLLOUT_WAVES, one process per arm
    (this tool with --arm), each with its own warm-up and windows; the parent only collects.
Medians over WINDOWS windows, with every window's value.  An arm counts as faster than another only if its
slowest window is below the other's fastest.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVES_ENV = "BALLENV_MLP_ROLLOUT_WAVES"
CLOCK_HZ = 2.4e9
MFMAS_PER_TILE = {3: 64 + 256 + 32, 2: 64 + 32}      # 16-env tile: layer 1, [layer 2,] the last layer


def wall(run, n, dev):
    """Wall seconds of n calls of run(), closed by one synchronise."""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def interleaved(arms, measure, windows):
    out = {k: [] for k in arms}
    for _ in range(windows):
        for k, fn in arms.items():
            out[k].append(measure(fn))
    return out


def summary(ws):
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": v} for k, v in ws.items()}


def faster(s, a, b):
    """arm a's slowest window is below arm b's fastest"""
    return s[a]["max"] < s[b]["min"]


def policy(gb, kind, dev):
    return gb.BlockPolicy.from_npz(gb.reference_block_weights(kind)).to(dev)


def mfma_floor_us(N, layers, name, cus):
    """The matrix pipe's time per step for the instance `name` (mlp_rollout_kernel<L, NW>): one workgroup per
    compute unit (the staged image leaves room for one), a wave's two tiles back to back on its SIMD."""
    nw = int(name.split(",")[1].strip(" >"))
    waves = (N + 31) // 32
    wgs = (waves + nw - 1) // nw
    simds = min(wgs, cus) * min(nw, 4)
    tiles = (N + 15) // 16
    return {"tiles": tiles, "simds_in_use": simds, "instance": name,
            "mfma_floor_us": tiles * MFMAS_PER_TILE[layers] * 32 / simds / CLOCK_HZ * 1e6}


def rollout_row(gb, dev, T, N, kind, args):
    arms, closers, name = {}, [], None
    for which in ("fused", "hip_captured", "hip_eager"):
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        ro = gb.BlockRollout(env, policy(gb, kind, dev), horizon=T, record_obs=True, seed=2,
                             backend="fused" if which == "fused" else "hip", chunk=min(T, 100))
        if which == "fused":
            name = ro.hp.rollout_kernel
            assert name is not None, "no fused instance for this shape"
        if which == "hip_captured":
            ro.capture(chunk=min(T, 250))
        arms[which] = ro.run_eager if which == "hip_eager" else ro.run
        closers.append((ro, env))
    reps = max(3, args.steps_per_window // T)
    for fn in arms.values():
        wall(fn, 2, dev)
    ws = interleaved(arms, lambda fn: wall(fn, reps, dev) / (reps * T) * 1e6, args.windows)
    layers = closers[0][0].hp.layers
    row = {"T": T, "N": N, "weights": kind, "layers": layers, "horizons_per_window": reps, "us_per_step": summary(ws)}
    row.update(mfma_floor_us(N, layers, name, torch.cuda.get_device_properties(dev).multi_processor_count))
    s = row["us_per_step"]
    row["fused_faster_than_hip_captured"] = faster(s, "fused", "hip_captured")
    row["fused_faster_than_hip_eager"] = faster(s, "fused", "hip_eager")
    row["hip_captured_over_fused"] = s["hip_captured"]["median"] / s["fused"]["median"]
    for ro, env in closers:
        ro.close()
        env.close()
    return row


def trainer_row(gb, dev, T, N, args):
    arms, closers = {}, []
    for which in ("fused", "hip_captured", "hip_eager"):
        torch.manual_seed(0)
        pol = gb.BlockPolicy(3, 128, 9, final_relu=True).to(dev)
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        tr = gb.BlockTrainer(env, pol, horizon=T, lr=1e-2, seed=2, log_rows=args.iters, chunk=min(T, 100),
                             backend="fused" if which == "fused" else "hip")
        if which != "hip_eager":
            tr.capture()            # (fused: the update half only)
        arms[which] = lambda tr=tr: tr.train(1)
        closers.append((tr, env))
    for fn in arms.values():
        wall(fn, 3, dev)
    ws = interleaved(arms, lambda fn: wall(fn, args.iters, dev) / args.iters * 1e3, args.windows)
    s = summary(ws)
    row = {"T": T, "N": N, "iterations_per_window": args.iters, "ms_per_iteration": s,
           "fused_faster_than_hip_captured": faster(s, "fused", "hip_captured"),
           "fused_faster_than_hip_eager": faster(s, "fused", "hip_eager"),
           "hip_captured_over_fused": s["hip_captured"]["median"] / s["fused"]["median"]}
    for tr, env in closers:
        tr.close()
        env.close()
    return row


def arm(gb, dev, T, N, args):
    """One instance (this process's BALLENV_MLP_ROLLOUT_WAVES), its own warm-up and windows."""
    env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
    env.reset()
    ro = gb.BlockRollout(env, policy(gb, "supervised3", dev), horizon=T, record_obs=True, seed=2, backend="fused",
                         chunk=min(T, 100))
    reps = max(3, args.steps_per_window // T)
    wall(ro.run, 2, dev)
    ws = [wall(ro.run, reps, dev) / (reps * T) * 1e6 for _ in range(args.windows)]
    row = {"T": T, "N": N, "waves_env": os.environ.get(WAVES_ENV), "instance": ro.hp.rollout_kernel,
           "us_per_step": summary({"fused": ws})["fused"]}
    ro.close()
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32x512,100x4096,100x16384,100x65536", help="TxN,... of leg (a)")
    ap.add_argument("--two-layer-size", default="100x4096", help="TxN of leg (a)'s 2-layer row")
    ap.add_argument("--trainer-sizes", default="32x512,100x4096", help="TxN,... of leg (b)")
    ap.add_argument("--instance-sizes", default="100x4096,100x65536", help="TxN,... of leg (c)")
    ap.add_argument("--steps-per-window", type=int, default=12000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--arm", default=None, help="TxN: run leg (c)'s arm for this process's " + WAVES_ENV + " and print it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_rollout.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_rollout_time needs a GPU"
    import gym_ballenv_amd as gb
    dev = torch.device("cuda:0")
    size = lambda s: tuple(int(v) for v in s.split("x"))  # noqa: E731
    if args.arm:
        print("ARM " + json.dumps(arm(gb, dev, *size(args.arm), args)), flush=True)
        return
    res = {"tool": "tools/mlp_rollout_time.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "clock_hz_assumed": CLOCK_HZ,
           "windows": args.windows, "steps_per_window": args.steps_per_window, "rollout": [], "trainer": [],
           "instances": []}
    for s in args.sizes.split(","):
        res["rollout"].append(rollout_row(gb, dev, *size(s), "supervised3", args))
        print(json.dumps(res["rollout"][-1]), flush=True)
    res["rollout"].append(rollout_row(gb, dev, *size(args.two_layer_size), "reinforce2", args))
    print(json.dumps(res["rollout"][-1]), flush=True)
    for s in args.trainer_sizes.split(","):
        res["trainer"].append(trainer_row(gb, dev, *size(s), args))
        print(json.dumps(res["trainer"][-1]), flush=True)
    for s in args.instance_sizes.split(","):
        for waves in ("1", "2", "4", "8"):
            env = dict(os.environ, **{WAVES_ENV: waves})
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", s, "--windows", str(args.windows),
                   "--steps-per-window", str(args.steps_per_window)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ARM ")]
            if r.returncode != 0 or not lines:
                raise RuntimeError(f"arm {waves} at {s} failed ({r.returncode}): {r.stderr[-2000:]}")
            res["instances"].append(json.loads(lines[-1][4:]))
            print(json.dumps(res["instances"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
