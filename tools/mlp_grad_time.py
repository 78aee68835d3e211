#!/usr/bin/env python3
"""Time be_mlp_grad (BlockGrad) against reinforce_losses + backward() on the same tensors.

    python tools/mlp_grad_time.py [--out profiles/mlp_grad.json]

Per (T, N, layers): an eager BlockRollout with record_obs=True (the reference's trained weights:
`supervised3` for 3 layers, `reinforce2` for 2) and be_a2c_targets of it give the block counts, actions,
returns_norm and valid.  The two launches of be_mlp_grad are timed over WINDOWS windows of LAUNCHES
back-to-back calls between two HIP events (after a warm-up); the torch path --
reinforce_losses(targets=...) + backward(), what reinforce_update(grads="torch") runs -- warm, as the
median of its runs between events with a synchronise.  torch.cuda.max_memory_allocated is recorded for
each side on top of what the rollout and the targets hold.  FLOPs are 2 per multiply-add of the
matrix products per row (affine1 and gW1: 2 * 29 H1 each; every later layer forward, dh and its gradient:
3 * 2 * in * out).  Needs a GPU: there is no fallback.
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
    ap.add_argument("--sizes", default="100x65536x3,100x65536x2,1000x4096x3,1000x4096x2,32x512x3,32x512x2",
                    help="TxNxlayers,...")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3, help="0: kernel only")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_grad.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_grad_time needs a GPU"
    import gym_ballenv_amd as gb
    from gym_ballenv_amd.block_policy import (BlockGrad, BlockPolicy, BlockRollout, reference_block_weights,
                                              reinforce_losses)
    dev = torch.device("cuda:0")
    rows_out = []
    for size in args.sizes.split(","):
        T, N, layers = (int(v) for v in size.split("x"))
        pol = BlockPolicy.from_npz(reference_block_weights("supervised3" if layers == 3 else "reinforce2")).to(dev)
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        ro = BlockRollout(env, pol, horizon=T, record_obs=True, seed=2)
        ro.run_eager()
        tg = gb.a2c_targets(env, ro.rewards, ro.dones, None, args.gamma, with_returns=False)
        blocks, actions, rn, valid = ro.blocks, ro.actions, tg.returns_norm, tg.valid
        bg = BlockGrad(env, pol)
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        k = lambda: bg(blocks, actions, rn, valid, loss="reinforce")
        events_ms(k, 3)
        ms = [events_ms(k, args.launches) for _ in range(args.windows)]
        loss, count = bg.losses.tolist()
        mem_k = torch.cuda.max_memory_allocated(dev) - base
        ms_t, mem_t, rel, loss_rel = [float("nan")], None, None, None
        if args.torch_reps > 0:
            def tt():
                pol.zero_grad(set_to_none=True)
                a = reinforce_losses(pol, blocks, actions, ro.rewards, ro.dones, args.gamma, targets=(rn, valid))
                a.backward()
                return a
            torch.cuda.reset_peak_memory_stats(dev)
            a = tt()                             # warm-up, and the comparison below
            torch.cuda.synchronize(dev)
            rel = {kk: float((bg.grads[kk] - p.grad).abs().max() / p.grad.abs().max())
                   for kk, p in pol.named_parameters()}
            loss_rel = abs(loss - float(a)) / abs(float(a))
            del a
            ms_t = [events_ms(tt, 1) for _ in range(args.torch_reps)]
            mem_t = torch.cuda.max_memory_allocated(dev) - base
            pol.zero_grad(set_to_none=True)
        H1, H2, A = pol.hidden1, pol.hidden2, pol.num_actions
        flop_row = 2 * (2 * 29 * H1) + (3 * 2 * (H1 * H2 + H2 * A) if layers == 3 else 3 * 2 * H1 * A)
        n = T * N
        med = statistics.median(ms)
        row = {"T": T, "N": N, "layers": layers, "rows": n, "hidden1": H1, "hidden2": H2, "active_rows": count,
               "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_windows": ms,
               "torch_ms_median": statistics.median(ms_t), "torch_ms_min": min(ms_t), "torch_ms_runs": ms_t,
               "torch_over_kernel": statistics.median(ms_t) / med,
               "kernel_peak_bytes_beyond_inputs": mem_k, "torch_peak_bytes_beyond_inputs": mem_t,
               "workspace_bytes": bg.workspace.numel() * 8,
               "flop_per_row": flop_row, "kernel_TFLOPs": n * flop_row / (med * 1e-3) / 1e12,
               "ns_per_row": med * 1e6 / n,
               "max_rel_diff_vs_torch_f32": rel, "loss_rel_diff_vs_torch_f32": loss_rel,
               "launches_per_window": args.launches, "windows": args.windows}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        ro.close()
        env.close()
        del ro, env, bg, tg, blocks, actions, rn, valid, pol
        gc.collect()
        torch.cuda.empty_cache()
    res = {"tool": "tools/mlp_grad_time.py", "command": " ".join(["python"] + sys.argv),
           "device": torch.cuda.get_device_name(0), "gamma": args.gamma,
           "lib": os.environ.get("BALLENV_LIB", "in-tree"), "sizes": rows_out}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
