#!/usr/bin/env python3
"""Time be_a2c_grad (A2CGrad) against a2c_losses + backward() on the same tensors.

    python tools/a2c_grad_time.py [--out profiles/a2c_grad.json]

Per (T, N, W): a real backend="fused" rollout with record_obs=True and be_a2c_targets of it give the
observations, actions, returns_norm and valid.  The two launches of be_a2c_grad are timed over
WINDOWS windows of LAUNCHES back-to-back calls between two HIP events (after a warm-up); the
torch path -- a2c_losses(targets=...) + backward(), what a2c_update(grads="torch") runs -- warm,
as the median of three runs between events with a synchronise.  torch.cuda.max_memory_allocated
is recorded for each side on top of what the rollout and the targets hold.  FLOPs are 2 per
multiply-add of the four matrix products per row (fc1 and gW1: 2 F H each; the heads forward,
dh and their gradients: 3 * 2 (A + 1) H).  Needs a GPU: there is no fallback.
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100x65536x10,1000x4096x5,32x512x10", help="TxNxW,...")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3, help="0: kernel only")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "a2c_grad.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a2c_grad_time needs a GPU"
    import gym_ballenv_amd as gb
    from gym_ballenv_amd.rollout import A2CGrad, Rollout, a2c_losses
    dev = torch.device("cuda:0")
    rows_out = []
    for size in args.sizes.split(","):
        T, N, W = (int(v) for v in size.split("x"))
        torch.manual_seed(0)
        pol = gb.Policy(W).to(dev)
        env = gb.BatchedBallEnv(N, W, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        ro = Rollout(env, pol, horizon=T, backend="fused", record_obs=True, seed=2)
        ro.run()
        tg = ro.targets(args.gamma, with_returns=False)
        obs, actions, rn, valid = ro.obs[:-1], ro.actions, tg.returns_norm, tg.valid
        ag = A2CGrad(env, pol)
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        k = lambda: ag(obs, actions, rn, valid)
        events_ms(k, 3)
        ms = [events_ms(k, args.launches) for _ in range(args.windows)]
        pl, vl, count = ag.losses()
        mem_k = torch.cuda.max_memory_allocated(dev) - base
        ms_t, mem_t, rel, loss_rel = [float("nan")], None, None, None
        if args.torch_reps > 0:
            def tt():
                pol.zero_grad(set_to_none=True)
                a, b = a2c_losses(pol, obs, actions, ro.rewards, ro.dones, args.gamma, targets=(rn, valid))
                (a + b).backward()
                return a, b
            torch.cuda.reset_peak_memory_stats(dev)
            a, b = tt()                          # warm-up, and the comparison below
            torch.cuda.synchronize(dev)
            rel = {kk: float((ag.grads[kk] - p.grad).abs().max() / p.grad.abs().max())
                   for kk, p in pol.named_parameters()}
            loss_rel = abs(pl + vl - float(a + b)) / abs(float(a + b))
            del a, b
            ms_t = [events_ms(tt, 1) for _ in range(args.torch_reps)]
            mem_t = torch.cuda.max_memory_allocated(dev) - base
            pol.zero_grad(set_to_none=True)
        F, H, A = env.obs_dim, pol.hidden_layer, pol.action_head.out_features
        flop_row = 2 * (2 * F * H) + 3 * 2 * (A + 1) * H
        n = T * N
        med = statistics.median(ms)
        row = {"T": T, "N": N, "W": W, "rows": n, "F": F, "hidden": H, "active_rows": count,
               "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_windows": ms,
               "torch_ms_median": statistics.median(ms_t), "torch_ms_min": min(ms_t), "torch_ms_runs": ms_t,
               "torch_over_kernel": statistics.median(ms_t) / med,
               "kernel_peak_bytes_beyond_inputs": mem_k, "torch_peak_bytes_beyond_inputs": mem_t,
               "workspace_bytes": ag.workspace.numel() * 8,
               "flop_per_row": flop_row, "kernel_TFLOPs": n * flop_row / (med * 1e-3) / 1e12,
               "obs_bytes_per_row": F, "kernel_obs_GBps": n * (F + 6) / (med * 1e-3) / 1e9,
               "ns_per_row": med * 1e6 / n,
               "max_rel_diff_vs_torch_f32": rel, "loss_rel_diff_vs_torch_f32": loss_rel,
               "launches_per_window": args.launches, "windows": args.windows}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        ro.close()
        env.close()
        del ro, env, ag, tg, obs, actions, rn, valid, pol
        gc.collect()
        torch.cuda.empty_cache()
    res = {"tool": "tools/a2c_grad_time.py", "device": torch.cuda.get_device_name(0), "gamma": args.gamma,
           "lib": os.environ.get("BALLENV_LIB", "in-tree"), "sizes": rows_out}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
