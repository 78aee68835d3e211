#!/usr/bin/env python3
"""Time be_observe_pixels against a batched torch composition of the same function and against a bare
fill of its output, in one session.

    python tools/pixels_time.py [--out profiles/pixels.json]

At each N (4 096 and 65 536 envs, the default config after 20 Philox steps) and for u8-only and f32-only
output, three legs:
  kernel  ``env.observe_pixels(out=...)``: one launch of pixels_kernel;
  torch   the same function as a user could batch it in torch on the same GPU: the patch by broadcasting
          the doubled-pixel-centre rule over (envs, 100, 100), one object after the other in render.draw's
          order, then PIL's two passes as two einsums with the integer coefficients (be_pixels_coeffs) --
          in f64, since torch has no integer matmul on the GPU; every sum is an integer below 2^31, so f64
          is exact -- each followed by the +2^21, >> 22, clip.  In chunks of --chunk envs.  Its bytes are
          checked equal to the kernel's before anything is timed;
  fill    ``out.fill_(1)``: the write floor of the same output bytes (4.8 KB per env u8, 19.2 KB f32).
Method: each leg is captured into a HIP graph (--launches back-to-back calls for kernel and fill, one pass
for torch), warmed up, and the three graphs are replayed in turn --reps times, each replay between two HIP
events.  Reported per call: min / median / max over the repetitions.  Needs a GPU: there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def coeff_matrix(lib, dev):
    """(40, 100) f64: row xx holds output xx's integer taps at their input positions."""
    kk, bounds = (C.c_int32 * 400)(), (C.c_int32 * 80)()
    assert lib.be_pixels_coeffs(kk, bounds) == 0
    kk, bounds = np.array(kk).reshape(40, 10), np.array(bounds).reshape(40, 2)
    m = np.zeros((40, 100))
    for xx in range(40):
        m[xx, bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = kk[xx, :bounds[xx, 1]]
    return torch.from_numpy(m).to(dev)


def constants(lib, dev):
    """The composition's constant tensors, made once (a capture admits no host-to-device copy): the
    coefficient matrix, the colour table, the patch's index range, ToTensor's divisor."""
    lut = torch.tensor([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0]], dtype=torch.uint8, device=dev)
    ar = torch.arange(100, device=dev, dtype=torch.int64)   # int64: a far obstacle's squared distance passes 2^31
    return coeff_matrix(lib, dev), lut, ar, torch.tensor(255.0, device=dev)


def torch_pixels(env, consts, f32, out, chunk):
    cfg, dev = env.cfg, env.device
    K, lut, ar, div = consts
    for s in range(0, env.num_envs, chunk):
        e = min(s + chunk, env.num_envs)
        a = env.agent[s:e].to(torch.int64)
        x = a[:, 0, None] - 50 + ar                      # (n, 100) world x of column j
        y = a[:, 1, None] + 49 - ar                      # (n, 100) world y of row i
        inside = ((y >= 0) & (y < cfg.screen_height))[:, :, None] & ((x >= 0) & (x < cfg.screen_width))[:, None, :]
        X, Y = 2 * x + 1, 2 * y + 1
        col = torch.zeros((e - s, 100, 100), dtype=torch.int64, device=dev)

        def disk(c, r, colour):
            c = c.to(torch.int64)
            u, v = X - 2 * c[:, 0, None], Y - 2 * c[:, 1, None]
            cover = ((u * u)[:, None, :] + (v * v)[:, :, None] <= 4 * r * r) & inside
            col.masked_fill_(cover, colour)

        disk(env.agent[s:e], cfg.radius_agent, 1)
        g = env.goal[s:e].to(torch.int64)
        u, v = (X - 2 * g[:, 0, None])[:, None, :], (Y - 2 * g[:, 1, None])[:, :, None]
        fan = ((u <= 10) & (v <= 10) & (u + v >= 0)) | ((v <= 10) & (u >= -10) & (v >= u))
        col.masked_fill_(fan & inside, 1)
        for k in range(cfg.num_static):
            disk(env.static_obs[k, s:e], cfg.radius_obstacle, 2)
        for k in range(cfg.num_dynamic):
            disk(env.dyn_obs[k, s:e], cfg.radius_obstacle, 3)
        patch = lut[col].to(torch.float64)               # (n, 100 i, 100 j, 3)
        h = torch.einsum("xj,nijc->nixc", K, patch)
        h = torch.floor((h + 2.0 ** 21) / 2.0 ** 22).clamp_(0, 255)
        w = torch.einsum("yi,nixc->ncyx", K, h)
        w = torch.floor((w + 2.0 ** 21) / 2.0 ** 22).clamp_(0, 255)
        if f32:
            out[s:e] = w.to(torch.float32) / div
        else:
            out[s:e] = w.to(torch.uint8)
    return out


def capture(fn, calls, dev, side):
    g = torch.cuda.CUDAGraph()
    fn()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(g, stream=side):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize(dev)
    return g


def timed(g, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(ms):
    return {"ms_min": min(ms), "ms_median": statistics.median(ms), "ms_max": max(ms), "ms_reps": ms}


def case(gb, dev, N, f32, args, K, side):
    env = gb.BatchedBallEnv(N, 10, gb.EnvConfig(), device=dev, seed=1)
    env.reset()
    acts = env.sample_actions(20, seed=3)
    for t in range(20):
        env.step(acts[t])
    dt = torch.float32 if f32 else torch.uint8
    out_k, out_t, out_f = (torch.zeros((N, 3, 40, 40), dtype=dt, device=dev) for _ in range(3))
    env.observe_pixels(f32=f32, out=out_k)
    with torch.no_grad():
        torch_pixels(env, K, f32, out_t, args.chunk)
    torch.cuda.synchronize(dev)
    assert torch.equal(out_k, out_t), "the torch composition and the kernel disagree"
    legs = {"kernel": (lambda: env.observe_pixels(f32=f32, out=out_k), args.launches),
            "torch": (lambda: torch_pixels(env, K, f32, out_t, args.chunk), 1),
            "fill": (lambda: out_f.fill_(1), args.launches)}
    with torch.no_grad():
        graphs = {name: (capture(fn, calls, dev, side), calls) for name, (fn, calls) in legs.items()}
        ms = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, (g, calls) in graphs.items():
                ms[name].append(timed(g, calls))
    out_bytes = N * 4800 * (4 if f32 else 1)
    row = {"N": N, "output": "f32" if f32 else "u8", "output_bytes": out_bytes, "state_bytes_read": N * 80,
           **{name: summary(v) for name, v in ms.items()}}
    k, t, f = (row[n]["ms_median"] for n in ("kernel", "torch", "fill"))
    row["torch_over_kernel"] = t / k
    row["kernel_over_fill"] = k / f
    row["kernel_output_GBps"] = out_bytes / (k * 1e-3) / 1e9
    row["fill_GBps"] = out_bytes / (f * 1e-3) / 1e9
    row["kernel_us_per_1000_envs"] = k * 1e3 / (N / 1000)
    del graphs
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixels.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pixels_time needs a GPU"
    import gym_ballenv_amd as gb
    from gym_ballenv_amd import _abi
    dev = torch.device("cuda:0")
    K = constants(_abi.lib(), dev)
    side = torch.cuda.Stream(dev)
    res = {"tool": "tools/pixels_time.py", "device": torch.cuda.get_device_name(0), "launches_per_graph": args.launches,
           "reps": args.reps, "torch_chunk": args.chunk, "cases": []}
    for N in (int(v) for v in args.sizes.split(",")):
        for f32 in (False, True):
            row = case(gb, dev, N, f32, args, K, side)
            print(json.dumps({k: v for k, v in row.items() if not isinstance(v, dict)} |
                             {n: row[n]["ms_median"] for n in ("kernel", "torch", "fill")}), flush=True)
            res["cases"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
