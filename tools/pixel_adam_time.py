#!/usr/bin/env python3
"""Time be_cnn_adam (HipPixelAdam) and PixelTrainer against the paths they replace, in one session, the
variants of a leg interleaved window by window after a warm-up of each.

    python tools/pixel_adam_time.py [--out profiles/pixel_adam.json]

(a) The update tail, per call, on the pixel agent's 14 parameters (A = 9): the new path is HipPixelAdam.step
    (the update + pack kernel, the state kernel); the path it replaces is what
    pixel_reinforce_update(grads="hip") runs with a torch optimizer behind PixelGrad: PixelGrad.assign()
    (14 .grad.copy_()), torch.optim.Adam.step() and HipPixelPolicy.load().  Windows of LAUNCHES back-to-back
    calls between two HIP events (device span per call: it includes the gaps the host leaves), with the
    host's wall time to enqueue the window alongside (no synchronise inside).
(b) The REINFORCE iteration at the given (T, N): PixelTrainer.train eager and captured against
    PixelRollout.run() + pixel_reinforce_update(grads="hip") with torch.optim.Adam (which returns the loss as
    a float, i.e. synchronises every iteration).  Wall clock per iteration over ITERS iterations with one
    closing synchronise; every variant has its own env and policy from the same seeds.
Medians over WINDOWS windows.  Needs a GPU: there is no fallback.
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


def tail(gb, dev, args):
    env = gb.BatchedBallEnv(64, 5, gb.EnvConfig(), device=dev, seed=1)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(1)
    fns, keep = {}, []
    for which in ("hip_optim", "torch_tail"):
        torch.manual_seed(0)
        pol = gb.PixelPolicy(9).to(dev)
        hp = gb.HipPixelPolicy(env, pol)
        pg = gb.PixelGrad(env, pol)
        for k in pg.grads:
            pg.grads[k].copy_(torch.randn(pg.grads[k].shape, device=dev, generator=gen) * 1e-3)
        for k in ("conv1.bias", "conv2.bias", "conv3.bias"):      # as be_cnn_grad writes them
            pg.grads[k].zero_()
        if which == "hip_optim":
            opt = gb.HipPixelAdam(hp, pol, lr=1e-3, log_rows=64)
            fns[which] = lambda opt=opt, pg=pg: opt.step(pg.grads, pg.losses)
        else:
            opt = torch.optim.Adam(pol.parameters(), lr=1e-3)

            def fn(opt=opt, pg=pg, hp=hp, pol=pol):
                pg.assign()
                opt.step()
                hp.load(pol)
            fns[which] = fn
        keep.append((pol, hp, pg, opt))
    for fn in fns.values():
        window(fn, 5, dev)
    ws = interleaved(fns, lambda fn: window(fn, args.launches, dev), args.windows)
    out = {"kind": "adam", "elements": sum(p.numel() for p in keep[0][0].parameters())}
    for k, w in ws.items():
        out[k] = {"device_ms_per_call_median": med([x[0] for x in w]), "device_ms_windows": [x[0] for x in w],
                  "host_ms_per_call_median": med([x[1] for x in w]), "host_ms_windows": [x[1] for x in w]}
    for _, hp, _, _ in keep:
        hp.close()
    env.close()
    out["torch_over_hip_device"] = out["torch_tail"]["device_ms_per_call_median"] / out["hip_optim"]["device_ms_per_call_median"]
    out["torch_over_hip_host"] = out["torch_tail"]["host_ms_per_call_median"] / out["hip_optim"]["host_ms_per_call_median"]
    return out


def iteration(gb, dev, T, N, args):
    runs, closers = {}, []
    for which in ("parent_loop", "trainer_eager", "trainer_captured"):
        torch.manual_seed(0)
        pol = gb.PixelPolicy(9).to(dev)
        env = gb.BatchedBallEnv(N, 5, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        if which == "parent_loop":
            ro = gb.PixelRollout(env, pol, horizon=T, seed=2, record_images=True)
            ro.capture(chunk=min(T, 250))
            opt = torch.optim.Adam(pol.parameters(), lr=1e-3)

            def run(iters, ro=ro, opt=opt):
                for _ in range(iters):
                    ro.run()
                    gb.pixel_reinforce_update(ro, opt, gamma=args.gamma, targets="hip", grads="hip")
            runs[which] = run
            closers.append((ro, env))
        else:
            tr = gb.PixelTrainer(env, pol, horizon=T, gamma=args.gamma, lr=1e-3, seed=2, log_rows=args.iters,
                                 chunk=min(T, 250))
            if which == "trainer_captured":
                tr.capture()
            runs[which] = tr.train
            closers.append((tr, env))
    for run in runs.values():
        run(3)
    torch.cuda.synchronize(dev)
    ws = interleaved(runs, lambda run: wall(run, args.iters, dev), args.windows)
    out = {"T": T, "N": N}
    for k, ms in ws.items():
        out[k] = {"ms_per_iteration_median": med(ms), "ms_per_iteration_min": min(ms), "ms_windows": ms}
    p = out["parent_loop"]["ms_per_iteration_median"]
    for k in ("trainer_eager", "trainer_captured"):
        out[f"parent_loop_over_{k}"] = p / out[k]["ms_per_iteration_median"]
    for c, env in closers:
        c.close()
        env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16x64,32x512", help="TxN,... of part (b)")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_adam.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pixel_adam_time needs a GPU"
    import gym_ballenv_amd as gb
    dev = torch.device("cuda:0")
    res = {"tool": "tools/pixel_adam_time.py", "device": torch.cuda.get_device_name(0), "gamma": args.gamma,
           "launches_per_window": args.launches, "windows": args.windows, "iterations_per_window": args.iters,
           "tail": None, "iteration": []}
    res["tail"] = tail(gb, dev, args)
    print(json.dumps(res["tail"]), flush=True)
    for size in args.sizes.split(","):
        T, N = (int(v) for v in size.split("x"))
        row = iteration(gb, dev, T, N, args)
        print(json.dumps(row), flush=True)
        res["iteration"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
