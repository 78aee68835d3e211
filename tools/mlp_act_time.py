#!/usr/bin/env python3
"""Time be_mlp_act (HipBlockPolicy) and BlockRollout against the path a user had before them, in
one session.

    python tools/mlp_act_time.py [--out profiles/mlp_act.json]

(a) select_action per call, the 3-layer reference shape (29 -> 128 -> 128 -> 9, the supervised weights),
    at each N: ``be_mlp_act`` with blocks_in = NULL (prep_state2 computed in the kernel) against
    ``env.observe_blocks(f32=True)`` + the BlockPolicy forward in torch fp32 + the cumsum draw on
    ``torch.rand`` uniforms (torch_block_select_action), under no_grad.  HIP events around WINDOWS
    windows of LAUNCHES back-to-back calls after a warm-up (device span per call: it includes the
    gaps the host leaves); the median window is reported, with the host's wall time to enqueue.
    The kernel's rate is set against the 157 TFLOP/s f32 MFMA peak DESIGN 3.12 uses, at the
    2 * (29*128 + 128*128 + 128*9) = 42 496 FLOP of the unpadded shape per env.
(b) A BlockRollout of T steps at N envs, captured into HIP graphs, against the same loop with the
    torch policy (observe_blocks + torch_block_select_action + env.step per step, eager: the path has
    no graph form a user could reach without this module).  Wall clock per horizon with one closing
    synchronise, the median of WINDOWS windows after a warm-up.
Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.0
FLOP_PER_ENV = 2 * (29 * 128 + 128 * 128 + 128 * 9)


def window(fn, launches, dev):
    """(device ms per call between two events, host ms per call to enqueue)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    host = time.perf_counter() - t0
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches, host * 1e3 / launches


def stats(ws):
    return {"device_ms_per_call_median": statistics.median(w[0] for w in ws), "device_ms_windows": [w[0] for w in ws],
            "host_ms_per_call_median": statistics.median(w[1] for w in ws), "host_ms_windows": [w[1] for w in ws]}


def policy(dev):
    from gym_ballenv_amd.block_policy import BlockPolicy, reference_block_weights
    return BlockPolicy.from_npz(reference_block_weights("supervised3")).to(dev)


def act(gb, dev, N, args):
    from gym_ballenv_amd.block_policy import HipBlockPolicy, torch_block_select_action
    env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
    env.reset()
    acts = env.sample_actions(20, seed=3)
    for t in range(20):
        env.step(acts[t])
    pol = policy(dev)
    hp = HipBlockPolicy(env, pol)

    def torch_path():
        with torch.no_grad():
            x = env.observe_blocks(f32=True)
            return torch_block_select_action(pol, x, torch.rand(N, device=dev))

    out = {"N": N}
    for name, fn in (("be_mlp_act", hp.act), ("torch_path", torch_path), ("be_mlp_act_again", hp.act)):
        window(fn, 5, dev)
        out[name] = stats([window(fn, args.launches, dev) for _ in range(args.windows)])
    ms = out["be_mlp_act"]["device_ms_per_call_median"]
    out["tflops"] = N * FLOP_PER_ENV / (ms * 1e-3) / 1e12
    out["fraction_of_f32_mfma_peak"] = out["tflops"] / PEAK_TFLOPS
    out["torch_over_hip_device"] = out["torch_path"]["device_ms_per_call_median"] / ms
    hp.close(); env.close()
    return out


def rollout(gb, dev, T, N, args):
    from gym_ballenv_amd.block_policy import BlockRollout, torch_block_select_action
    out = {"T": T, "N": N}
    for which in ("block_rollout_captured", "torch_loop"):
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        pol = policy(dev)
        if which == "block_rollout_captured":
            ro = BlockRollout(env, pol, horizon=T, seed=2)
            ro.capture(chunk=T)
            run = ro.run
        else:
            ro = None

            def run():
                with torch.no_grad():
                    for _ in range(T):
                        a, _, _ = torch_block_select_action(pol, env.observe_blocks(f32=True), torch.rand(N, device=dev))
                        env.step(a.to(torch.uint8))
        run()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            ms.append((time.perf_counter() - t0) * 1e3)
        out[which] = {"ms_per_horizon_median": statistics.median(ms), "ms_windows": ms}
        if ro is not None:
            ro.close()
        env.close()
    out["torch_over_hip"] = out["torch_loop"]["ms_per_horizon_median"] / out["block_rollout_captured"]["ms_per_horizon_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--rollout", default="100x65536", help="TxN of part (b)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_act.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_act_time needs a GPU"
    import gym_ballenv_amd as gb
    dev = torch.device("cuda:0")
    res = {"tool": "tools/mlp_act_time.py", "device": torch.cuda.get_device_name(0), "shape": "29-128-128-9 (supervised3)",
           "launches_per_window": args.launches, "windows": args.windows, "flop_per_env": FLOP_PER_ENV,
           "f32_mfma_peak_tflops": PEAK_TFLOPS, "library": os.environ.get("BALLENV_LIB", "in-tree"), "act": [],
           "rollout": []}
    for N in (int(v) for v in args.sizes.split(",")):
        row = act(gb, dev, N, args)
        print(json.dumps(row), flush=True)
        res["act"].append(row)
    if args.rollout:                       # --rollout "": part (a) alone (A/B runs of a BALLENV_LIB build)
        T, N = (int(v) for v in args.rollout.split("x"))
        row = rollout(gb, dev, T, N, args)
        print(json.dumps(row), flush=True)
        res["rollout"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
