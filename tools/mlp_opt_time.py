#!/usr/bin/env python3
"""Time be_mlp_opt (HipBlockOptim) and the two block-MLP trainers against the paths they replace, in one
session, the variants of a leg interleaved window by window after a warm-up of each.

    python tools/mlp_opt_time.py [--out profiles/mlp_opt.json]

(a) The update tail, per call, for Adam and SGD on the 29 -> 128 -> 128 -> 9 network: the new path is
    HipBlockOptim.step (the update + pack kernel, the state kernel); the path it replaces is what
    reinforce_update / supervised_update(grads="hip") run with a torch optimizer behind BlockGrad:
    BlockGrad.assign() (six .grad.copy_()), torch.optim.Adam / SGD.step() and HipBlockPolicy.load().
    Windows of LAUNCHES back-to-back calls between two HIP events (device span per call: it includes the
    gaps the host leaves), with the host's wall time to enqueue the window alongside (no synchronise inside).
(b) The REINFORCE iteration at the given (T, N): BlockTrainer.train eager and captured against
    BlockRollout.run() + reinforce_update(grads="hip") with torch.optim.Adam (which returns the loss as a
    float, i.e. synchronises every iteration).  Wall clock per iteration over ITERS iterations with one
    closing synchronise; every variant has its own env and policy from the same seeds.
(c) The supervised epoch on the reference's recorded trial (3186 rows, 16 minibatches of 200):
    SupervisedTrainer eager and captured against a supervised_update(grads="hip") loop with torch.optim.SGD.
    Wall clock per epoch over EPOCHS epochs with one closing synchronise.
Medians over WINDOWS windows.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def wall(run, n, dev):
    """Wall ms per unit of run(n), closed by one synchronise."""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run(n)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / n


def med(xs):
    return statistics.median(xs)


def interleaved(variants, measure, windows):
    """{name: [measure(fn) per window]}, the variants taking turns inside every window."""
    out = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            out[k].append(measure(fn))
    return out


def tail(gb, dev, kind, args):
    torch.manual_seed(0)
    env = gb.BatchedBallEnv(512, 5, gb.EnvConfig(), device=dev, seed=1)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(1)
    fns, keep = {}, []
    for which in ("hip_optim", "torch_tail"):
        pol = gb.BlockPolicy(3, 128, 9, final_relu=False).to(dev)
        hp = gb.HipBlockPolicy(env, pol)
        bg = gb.BlockGrad(env, pol)
        for k in bg.grads:
            bg.grads[k].copy_(torch.randn(bg.grads[k].shape, device=dev, generator=gen) * 1e-3)
        if which == "hip_optim":
            opt = gb.HipBlockOptim(hp, pol, kind, lr=1e-2, log_rows=64)
            fns[which] = lambda opt=opt, bg=bg: opt.step(bg.grads, bg.losses)
        else:
            opt = (torch.optim.Adam if kind == "adam" else torch.optim.SGD)(pol.parameters(), lr=1e-2)

            def fn(opt=opt, bg=bg, hp=hp, pol=pol):
                bg.assign()
                opt.step()
                hp.load(pol)
            fns[which] = fn
        keep.append((pol, hp, bg, opt))
    for fn in fns.values():
        window(fn, 5, dev)
    ws = interleaved(fns, lambda fn: window(fn, args.launches, dev), args.windows)
    out = {"kind": kind, "elements": sum(p.numel() for p in keep[0][0].parameters())}
    for k, w in ws.items():
        out[k] = {"device_ms_per_call_median": med([x[0] for x in w]), "device_ms_windows": [x[0] for x in w],
                  "host_ms_per_call_median": med([x[1] for x in w]), "host_ms_windows": [x[1] for x in w]}
    for _, hp, _, _ in keep:
        hp.close()
    env.close()
    out["torch_over_hip_device"] = out["torch_tail"]["device_ms_per_call_median"] / out["hip_optim"]["device_ms_per_call_median"]
    out["torch_over_hip_host"] = out["torch_tail"]["host_ms_per_call_median"] / out["hip_optim"]["host_ms_per_call_median"]
    return out


def _summary(out, ws, unit, base):
    for k, ms in ws.items():
        out[k] = {f"ms_per_{unit}_median": med(ms), f"ms_per_{unit}_min": min(ms), "ms_windows": ms}
    p = out[base][f"ms_per_{unit}_median"]
    for k in ws:
        if k != base:
            out[f"{base}_over_{k}"] = p / out[k][f"ms_per_{unit}_median"]
    return out


def iteration(gb, dev, T, N, args):
    runs, closers = {}, []
    for which in ("parent_loop", "trainer_eager", "trainer_captured"):
        torch.manual_seed(0)
        pol = gb.BlockPolicy(3, 128, 9, final_relu=True).to(dev)
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        if which == "parent_loop":
            ro = gb.BlockRollout(env, pol, horizon=T, record_obs=True, seed=2)
            ro.capture(chunk=min(T, 250))
            opt = torch.optim.Adam(pol.parameters(), lr=1e-2)

            def run(iters, ro=ro, opt=opt):
                for _ in range(iters):
                    ro.run()
                    gb.reinforce_update(ro, opt, gamma=args.gamma, targets="hip", grads="hip")
            runs[which] = run
            closers.append((ro, env))
        else:
            tr = gb.BlockTrainer(env, pol, horizon=T, gamma=args.gamma, lr=1e-2, seed=2, log_rows=args.iters,
                                 chunk=min(T, 250))
            if which == "trainer_captured":
                tr.capture()
            runs[which] = tr.train
            closers.append((tr, env))
    for run in runs.values():
        run(3)
    torch.cuda.synchronize(dev)
    ws = interleaved(runs, lambda run: wall(run, args.iters, dev), args.windows)
    out = _summary({"T": T, "N": N}, ws, "iteration", "parent_loop")
    for c, env in closers:
        c.close()
        env.close()
    return out


def epoch(gb, dev, args):
    d = np.load(gb.reference_supervise_data(), allow_pickle=False)
    blocks, labels = torch.from_numpy(d["blocks"]).to(dev), torch.from_numpy(d["labels"]).to(dev)
    env = gb.BatchedBallEnv(64, 5, gb.EnvConfig(), device=dev, seed=1)
    env.reset()
    runs, closers = {}, []
    for which in ("parent_loop", "trainer_eager", "trainer_captured"):
        torch.manual_seed(0)
        pol = gb.BlockPolicy(3, 128, 9, final_relu=False).to(dev)
        if which == "parent_loop":
            bg = gb.BlockGrad(env, pol)
            opt = torch.optim.SGD(pol.parameters(), lr=1e-2)

            def run(epochs, pol=pol, bg=bg, opt=opt):
                for _ in range(epochs):
                    for i in range(0, blocks.shape[0], 200):
                        gb.supervised_update(pol, blocks[i:i + 200], labels[i:i + 200], opt, grads="hip", grad=bg)
            runs[which] = run
        else:
            tr = gb.SupervisedTrainer(env, pol, blocks, labels, batch_size=200, lr=1e-2, log_rows=16)
            if which == "trainer_captured":
                tr.capture()
            runs[which] = tr.train
            closers.append(tr)
    for run in runs.values():
        run(2)
    torch.cuda.synchronize(dev)
    ws = interleaved(runs, lambda run: wall(run, args.epochs, dev), args.windows)
    out = _summary({"rows": int(blocks.shape[0]), "batch": 200, "minibatches": 16}, ws, "epoch", "parent_loop")
    for c in closers:
        c.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32x512,100x4096", help="TxN,... of part (b)")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_opt.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_opt_time needs a GPU"
    import gym_ballenv_amd as gb
    dev = torch.device("cuda:0")
    res = {"tool": "tools/mlp_opt_time.py", "device": torch.cuda.get_device_name(0), "gamma": args.gamma,
           "launches_per_window": args.launches, "windows": args.windows, "iterations_per_window": args.iters,
           "epochs_per_window": args.epochs, "tail": [], "iteration": [], "epoch": None}
    for kind in ("adam", "sgd"):
        row = tail(gb, dev, kind, args)
        print(json.dumps(row), flush=True)
        res["tail"].append(row)
    for size in args.sizes.split(","):
        T, N = (int(v) for v in size.split("x"))
        row = iteration(gb, dev, T, N, args)
        print(json.dumps(row), flush=True)
        res["iteration"].append(row)
    res["epoch"] = epoch(gb, dev, args)
    print(json.dumps(res["epoch"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
