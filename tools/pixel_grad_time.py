#!/usr/bin/env python3
"""Time be_cnn_grad (the pixel agent's REINFORCE loss and gradients in HIP) against the torch path a user has
without it, on the same GPU in one session.

    python tools/pixel_grad_time.py [--out profiles/pixel_grad.json]

At each row count (4 096 and 65 536): the rows are ``PixelRollout(record_images=True)``'s own images, quadrants
and actions of the reference's trained policy (N = 4 096 envs, 1 resp. 16 steps, the default config after 20
Philox steps), coef standard normal, every row valid.  Two legs:
  hip    ``PixelGrad(...)``: be_cnn_grad's three kernels (pack, gradients, reduce);
  torch  what the parent commit offers: the f32 copy of the u8 images / 255, the quadrant one-hot,
         ``torch_pixel_forward(norm="sample")`` in fp32, ``Categorical.log_prob``, the loss sum and
         ``backward()``, in chunks of --chunk rows (the gradients accumulate in ``.grad`` across the chunks).
         The default chunk is all 65 536 rows at once: their saved activations, about 90 KB per row, fit the
         device's memory next to the record.
Before anything is timed the two paths' gradients are compared on the first --check rows by the rule of
tests/test_gpu_pixel_grad.py: per tensor err_hip <= 4 * err_torch32 + 1e-6 against the float64 restatement
(tests/cnn_grad_ref.py), the conv biases exact zeros.
Method (tools/pixel_act_time.py's): the hip leg is captured into a HIP graph of --launches back-to-back calls;
the torch leg runs eagerly after warm-up (autograd allocates); the legs are timed in turn --reps times, each
between two HIP events.  Reported per call: min / median / max over the repetitions.  Needs a GPU: there is no
fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_grad(gb, pol, images, quadrants, actions, coef, chunk):
    pol.zero_grad(set_to_none=True)
    total = 0.0
    for i in range(0, images.shape[0], chunk):
        s = slice(i, i + chunk)
        x = images[s].to(torch.float32) / 255.0
        q = torch.nn.functional.one_hot(quadrants[s].long(), 4).to(torch.float32)
        probs = gb.torch_pixel_forward(pol, x, q, "sample")
        logp = torch.distributions.Categorical(probs=probs).log_prob(actions[s].long())
        loss = -(logp * coef[s]).sum()
        loss.backward()
        total = total + loss.detach()
    return total


def timed(fn, calls, graph=None):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if graph is not None:
        graph.replay()
    else:
        for _ in range(calls):
            fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(ms, captured):
    return {"ms_min": min(ms), "ms_median": statistics.median(ms), "ms_max": max(ms), "ms_reps": ms, "captured": captured}


def agreement(gb, pol, pg, images, quadrants, actions, coef, n):
    import cnn_grad_ref as R
    ins = tuple(x[:n].contiguous() for x in (images, quadrants, actions, coef))
    pg(*ins)
    torch.cuda.synchronize()
    got = {k: v.cpu().clone() for k, v in pg.grads.items()}
    loss = float(pg.losses[0])
    cpu = tuple(x.cpu() for x in ins)
    ref = R.restatement(pol, *cpu)
    t32 = R.torch_reference(pol, *cpu, dtype=torch.float32, device=images.device)
    eh, et = R.errors(got, ref.grads), R.errors(t32.grads, ref.grads)
    fig = {"rows": n, "err_hip_vs_f64": eh, "err_torch32_vs_f64": et,
           "loss_err_hip": abs(loss - ref.loss) / ref.abs_loss, "loss_err_torch32": abs(t32.loss - ref.loss) / ref.abs_loss}
    print(json.dumps(fig), flush=True)
    R.check_rule((got, loss), t32, ref)
    assert all(torch.count_nonzero(got[k]) == 0 for k in R.CONV_BIASES)
    return fig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_grad.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pixel_grad_time needs a GPU"
    import gym_ballenv_amd as gb
    dev = torch.device("cuda:0")
    pol = gb.PixelPolicy()
    pol.load_state_dict(gb.reference_pixel_weights(), strict=True)
    pol = pol.to(dev)
    side = torch.cuda.Stream(dev)
    res = {"tool": "tools/pixel_grad_time.py", "device": torch.cuda.get_device_name(0), "launches_per_graph": args.launches,
           "reps": args.reps, "torch_chunk_rows": args.chunk, "cases": []}
    for rows in (int(v) for v in args.sizes.split(",")):
        N = min(args.envs, rows)
        T = rows // N
        env = gb.BatchedBallEnv(N, 10, gb.EnvConfig(), device=dev, seed=1)
        env.reset()
        acts = env.sample_actions(20, seed=3)
        for t in range(20):
            env.step(acts[t])
        ro = gb.PixelRollout(env, pol, T, seed=5, record_images=True)
        ro.run_eager()
        torch.cuda.synchronize(dev)
        images, quadrants, actions = ro.images.reshape(rows, 3, 40, 40), ro.quadrants.reshape(-1), ro.actions.reshape(-1)
        coef = torch.randn(rows, device=dev)
        pg = gb.PixelGrad(env, pol)
        fig = agreement(gb, pol, pg, images, quadrants, actions, coef, min(args.check, rows))
        hip = lambda: pg(images, quadrants, actions, coef)
        tor = lambda: torch_grad(gb, pol, images, quadrants, actions, coef, args.chunk)
        hip()
        tor()
        tor()
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(args.launches):
                hip()
        g.replay()
        torch.cuda.synchronize(dev)
        ms = {"hip": [], "torch": []}
        for _ in range(args.reps):
            ms["hip"].append(timed(hip, args.launches, g))
            ms["torch"].append(timed(tor, 1))
        row = {"rows": rows, "envs": N, "steps": T, "agreement": fig, "hip": summary(ms["hip"], True),
               "torch": summary(ms["torch"], False)}
        row["torch_over_hip"] = row["torch"]["ms_median"] / row["hip"]["ms_median"]
        row["hip_us_per_1000_rows"] = row["hip"]["ms_median"] * 1e3 / (rows / 1000)
        print(json.dumps({k: (v["ms_median"] if isinstance(v, dict) and "ms_median" in v else v)
                          for k, v in row.items() if k != "agreement"}), flush=True)
        res["cases"].append(row)
        del g
        ro.close()
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
