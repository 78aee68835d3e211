#!/usr/bin/env python3
"""Time be_cnn_act (the pixel agent's select_action in HIP) against the torch path a user has without it,
on the same GPU in one session.

    python tools/pixel_act_time.py [--out profiles/pixel_act.json]

At each N (4 096 and 65 536 envs, the default config after 20 Philox steps) and for both BatchNorm modes
(norm = sample, the reference's per-env statistics; running, the stored ones), three legs:
  act          ``HipPixelPolicy.act(image=...)``: be_cnn_act alone on a given u8 image;
  observe_act  ``HipPixelPolicy.act()``: be_observe_pixels + be_cnn_act, the per-step policy path;
  torch        ``pixel_inputs(env)`` (the f32 image from be_observe_pixels, the quadrant from
               be_observe_blocks) + ``torch_pixel_forward`` in fp32 under no_grad + the inverse-CDF draw on
               ``torch.rand`` and the log of the drawn probability.
Before anything is timed the two paths' probabilities are compared on the same state by the rule of
tests/test_gpu_pixel_policy.py: |hip - torch32| <= 2e-5 on every env, and on the first --check envs the HIP
error against a float64 torch forward is at most 4x torch fp32's + 1e-6.
Then one rollout case: ``PixelRollout`` of --steps steps at the first N against the same loop with the torch
policy (``pixel_inputs`` + forward + draw + ``env.step``).
Method: each leg is captured into a HIP graph (--launches back-to-back calls for the HIP legs, one pass for
torch; a leg whose capture fails is timed eagerly between events and marked so), warmed up, and the legs'
graphs are replayed in turn --reps times, each replay between two HIP events.  Reported per call: min /
median / max over the repetitions, and be_cnn_act's share of the 157.3 TFLOP/s f32 MFMA peak on the unpadded
network's FLOPs.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# multiply-adds of the unpadded network per env: the three convolutions and the head
MACS = 16 * 324 * 75 + 32 * 49 * 400 + 32 * 4 * 800 + 9 * 132
PEAK_F32_MFMA = 157.3e12
TOL = 2e-5


def torch_act(env, pol, norm, gb):
    img, quad = gb.pixel_inputs(env)
    probs = gb.torch_pixel_forward(pol, img, quad, norm)
    u = torch.rand(probs.shape[0], device=probs.device)
    a = (probs.cumsum(-1) <= u.unsqueeze(-1)).sum(-1).clamp_(max=probs.shape[1] - 1)
    return a.to(torch.uint8), torch.log(probs.gather(-1, a.unsqueeze(-1))).squeeze(-1), probs


def capture(fn, calls, dev, side):
    """(graph or None, calls): None when the leg cannot be captured."""
    fn()
    torch.cuda.synchronize(dev)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(calls):
                fn()
        g.replay()
        torch.cuda.synchronize(dev)
        return g
    except Exception as e:      # noqa: BLE001  (reported in the result, the leg is then timed eagerly)
        print(f"capture failed, timing eagerly: {type(e).__name__}: {e}", flush=True)
        torch.cuda.synchronize(dev)
        return None


def timed(g, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if g is not None:
        g.replay()
    else:
        for _ in range(calls):
            fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(ms, captured):
    return {"ms_min": min(ms), "ms_median": statistics.median(ms), "ms_max": max(ms), "ms_reps": ms, "captured": captured}


def run_legs(legs, dev, side, reps):
    graphs = {name: capture(fn, calls, dev, side) for name, (fn, calls) in legs.items()}
    ms = {name: [] for name in legs}
    for _ in range(reps):
        for name, (fn, calls) in legs.items():
            ms[name].append(timed(graphs[name], fn, calls))
    return {name: summary(v, graphs[name] is not None) for name, v in ms.items()}


def agreement(env, hp, pol, norm, gb, check):
    """The tolerance rule on the current state; returns the figures."""
    _, _, probs = hp.act()
    img, quad = gb.pixel_inputs(env)
    t32 = gb.torch_pixel_forward(pol, img, quad, norm)
    d = (probs - t32).abs().max().item()
    n = min(check, env.num_envs)
    pol.double()
    p64 = gb.torch_pixel_forward(pol, img[:n].double(), quad[:n].double(), norm)
    pol.float()
    err_hip = (probs[:n].double() - p64).abs().max().item()
    err_t32 = (t32[:n].double() - p64).abs().max().item()
    fig = {"max_abs_probs_hip_minus_torch32": d, "err_hip_vs_f64": err_hip, "err_torch32_vs_f64": err_t32, "f64_rows": n}
    print(json.dumps(fig), flush=True)
    assert d <= TOL and err_hip <= 4 * err_t32 + 1e-6, fig
    return fig


def make_env(gb, dev, N):
    env = gb.BatchedBallEnv(N, 10, gb.EnvConfig(), device=dev, seed=1)
    env.reset()
    acts = env.sample_actions(20, seed=3)
    for t in range(20):
        env.step(acts[t])
    return env


def act_case(gb, dev, N, norm, pol, args, side):
    env = make_env(gb, dev, N)
    hp = gb.HipPixelPolicy(env, pol, norm=norm, probs=True, seed=5)
    with torch.no_grad():
        fig = agreement(env, hp, pol, norm, gb, args.check)
        image = env.observe_pixels()
        legs = {"act": (lambda: hp.act(image=image), args.launches),
                "observe_act": (lambda: hp.act(), args.launches),
                "torch": (lambda: torch_act(env, pol, norm, gb), 1)}
        row = {"N": N, "norm": norm, "agreement": fig, **run_legs(legs, dev, side, args.reps)}
    k, o, t = (row[n]["ms_median"] for n in ("act", "observe_act", "torch"))
    row["torch_over_observe_act"] = t / o
    row["act_us_per_1000_envs"] = k * 1e3 / (N / 1000)
    row["act_TFLOPs"] = 2 * MACS * N / (k * 1e-3) / 1e12
    row["act_share_of_f32_mfma_peak"] = 2 * MACS * N / (k * 1e-3) / PEAK_F32_MFMA
    hp.close()
    env.close()
    return row


def rollout_case(gb, dev, N, pol, args, side):
    """PixelRollout of --steps steps, captured, against the same loop with the torch policy."""
    T = args.steps
    env = make_env(gb, dev, N)
    ro = gb.PixelRollout(env, pol, horizon=T, norm="sample", seed=5)
    env_t = make_env(gb, dev, N)

    def torch_loop():
        for _ in range(T):
            a, _, _ = torch_act(env_t, pol, "sample", gb)
            env_t.step(a)

    with torch.no_grad():
        legs = {"pixel_rollout": (ro.run_eager, 1), "torch_loop": (torch_loop, 1)}
        row = {"N": N, "steps": T, "norm": "sample", **run_legs(legs, dev, side, args.reps)}
    row["torch_over_pixel_rollout"] = row["torch_loop"]["ms_median"] / row["pixel_rollout"]["ms_median"]
    row["pixel_rollout_env_steps_per_s"] = N * T / (row["pixel_rollout"]["ms_median"] * 1e-3)
    ro.close()
    env.close()
    env_t.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_act.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pixel_act_time needs a GPU"
    import gym_ballenv_amd as gb
    dev = torch.device("cuda:0")
    pol = gb.PixelPolicy()
    pol.load_state_dict(gb.reference_pixel_weights(), strict=True)
    pol = pol.to(dev).eval()        # the forward's mode is torch_pixel_forward's norm, not the module's flag
    side = torch.cuda.Stream(dev)
    sizes = [int(v) for v in args.sizes.split(",")]
    res = {"tool": "tools/pixel_act_time.py", "device": torch.cuda.get_device_name(0), "launches_per_graph": args.launches,
           "reps": args.reps, "macs_per_env": MACS, "peak_f32_mfma_flops": PEAK_F32_MFMA, "cases": [], "rollout": None}

    def flat(row):
        return {k: (v["ms_median"] if isinstance(v, dict) and "ms_median" in v else v) for k, v in row.items()
                if k != "agreement"}

    for N in sizes:
        for norm in ("sample", "running"):
            row = act_case(gb, dev, N, norm, pol, args, side)
            print(json.dumps(flat(row)), flush=True)
            res["cases"].append(row)
    res["rollout"] = rollout_case(gb, dev, sizes[0], pol, args, side)
    print(json.dumps(flat(res["rollout"])), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
