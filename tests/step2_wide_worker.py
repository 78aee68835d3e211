"""Child process of tests/test_gpu_step2_wide.py: BALLENV_STEP2_WIDE is read at be_create, so each
side of the comparison runs in a process started with its value.

    python step2_wide_worker.py OUT.npz

Runs every case of CASES (default config, Philox mode, autoreset on) with the pool on and off and
writes, per case, every per-step output stacked over the steps, the final state blob (save_state),
the stats slots and which instance the steps took."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# (N, steps, env_offset): one wave; two waves, through the TimeLimit; 9 waves, the last block partial
# in waves; three waves at an offset into the global env ids
CASES = ((32, 300, 0), (64, 1100, 0), (288, 300, 0), (96, 300, 12345))
OUTPUTS = ("obs", "reward", "done", "truncated", "final_return", "final_len", "terminal_obs")


def run_case(torch, N, steps, offset, pool):
    from gym_ballenv_amd import BatchedBallEnv
    from gym_ballenv_amd.config import EnvConfig
    os.environ["BALLENV_POOL"] = "1" if pool else "0"
    env = BatchedBallEnv(N, 10, EnvConfig(), device="cuda:0", seed=0x51DE, env_offset=offset, terminal_obs=True)
    assert env.kernel_name("step") == f"step2_kernel<10, 13, 5, {'true' if pool else 'false'}>", env.kernel_name("step")
    assert (env.pool_bytes() > 0) == pool
    env.reset()
    acts = env.sample_actions(steps, seed=7)
    rec = {k: torch.zeros((steps,) + tuple(getattr(env, k).shape), dtype=getattr(env, k).dtype, device=env.device)
           for k in OUTPUTS}
    for t in range(steps):
        env.step(acts[t])
        for k in OUTPUTS:
            rec[k][t].copy_(getattr(env, k))
    res = {k: v.cpu().numpy() for k, v in rec.items()}
    res["state"] = env.save_state("cpu").numpy().copy()
    res["stats"] = env.stats_buf.cpu().numpy()
    res["instance"] = np.array(env.step_instance())
    env.status()
    env.close()
    return res


def main(out_path):
    import torch
    out = {}
    for N, steps, offset in CASES:
        for pool in (True, False):
            for k, v in run_case(torch, N, steps, offset, pool).items():
                out[f"{N}_{int(pool)}_{k}"] = v
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
