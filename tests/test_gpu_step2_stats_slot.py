"""GPU: step2_kernel reads a wave's statistics slot in the finishing path, not in the prologue.

The three 16-byte loads of the wave's 48-byte slot used to be the prologue's last loads, issued by
every wave; they now sit at the head of the finishing path, in the launch that folds into the slot,
and the prev_dist load is unconditional ("exact waits").  TimeLimit 2 makes every env
finish at least every second step, so every wave takes the finishing path (slot read, fold, slot
write) again and again, with the lean path (no slot access) in between wherever none of its envs
finishes, and a fold adds to what an earlier launch wrote.

Everything is compared bit for bit, no tolerances:
  * obs, reward, done, truncated, final_* and the full state after every step against the generic
    kernel (BALLENV_GENERIC_KERNELS=1) on the same seed and actions;
  * the statistics slots against a host model of the fold: per 32-env slot and per launch the sums
    of the finished envs taken in env order from zero (wave_stats), then added to the slot; min and
    max folded the same way.  The model's inputs are the generic kernel's done / final_* rows, its
    f64 operations are the kernel's (no FMA), so the slots are equal to the last bit;
  * stats_record() / episode_stats() against the same reduction of the model's slots.
Variants: the pool on and off, no statistics buffer at all (nothing is read or written and nothing
else changes), BALLENV_PREV_READ=0, and two clear_stats() windows.
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import KEYS, make_env, np_state

pytestmark = pytest.mark.gpu

W, STEPS, SEED = 10, 8, 0x51A7
POOL, NOPOOL = "step2_kernel<10, 13, 5, true>", "step2_kernel<10, 13, 5, false>"
# a lone env, a partial wave, an exact wave, a wave plus one, a block boundary (64 envs) plus one, three waves
SIZES = (1, 31, 32, 33, 65, 96)
OUT_KEYS = ("obs", "reward", "done", "truncated", "final_return", "final_len")

_REF = {}   # N -> (actions, the generic kernel's trace): computed once, shared, never modified


def _cfg():
    from gym_ballenv_amd.config import EnvConfig
    return EnvConfig(time_limit=2)


def _snapshot(env, res):
    obs, reward, done, info = res
    d = {"obs": obs, "reward": reward, "done": done, "truncated": info["truncated"],
         "final_return": info["final_return"], "final_len": info["final_len"]}
    d = {k: v.cpu().numpy().copy() for k, v in d.items()}
    d["state"] = np_state(env)
    return d


def _reference(gpu, N):
    if N not in _REF:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("BALLENV_GENERIC_KERNELS", "1")
            env = make_env(_cfg(), N, W, gpu, seed=SEED)
        assert env.kernel_name("step").endswith(", 0, 0, false>"), env.kernel_name("step")
        acts = env.sample_actions(STEPS, seed=SEED + 1)
        env.reset()
        trace = [_snapshot(env, env.step(acts[t])) for t in range(STEPS)]
        env.status()
        env.close()
        for s in trace:
            for v in (*[s[k] for k in OUT_KEYS], *s["state"].values()):
                v.setflags(write=False)
        _REF[N] = (acts, trace)
    return _REF[N]


def _cleared(slots):
    b = np.zeros((slots, 8), np.float64)
    b[:, 4], b[:, 5] = math.inf, -math.inf
    return b


def _fold(buf, step):
    """One launch's fold into the (slots, 8) buffer: wave_stats over each slot's 32 envs in env
    order, then the finishing path's read-modify-write of the slot (only when the wave counted one)."""
    done, ret, length = step["done"], step["final_return"], step["final_len"]
    for s in range(buf.shape[0]):
        n = s1 = s2 = sl = 0.0
        mn, mx = math.inf, -math.inf
        for e in range(32 * s, min(32 * s + 32, len(done))):
            if done[e]:
                r = float(ret[e])
                n += 1.0; s1 += r; s2 += r * r; sl += float(length[e])
                mn, mx = min(mn, r), max(mx, r)
        if n > 0.0:
            buf[s, 0] += n; buf[s, 1] += s1; buf[s, 2] += s2; buf[s, 3] += sl
            buf[s, 4], buf[s, 5] = min(buf[s, 4], mn), max(buf[s, 5], mx)


def _check_step(t, got, ref):
    for k in OUT_KEYS:
        rows = ref["done"] if k.startswith("final_") else slice(None)   # final_* are written on done rows
        np.testing.assert_array_equal(got[k][rows], ref[k][rows], err_msg=f"t={t} {k}")
    for k in KEYS:
        np.testing.assert_array_equal(got["state"][k], ref["state"][k], err_msg=f"t={t} state[{k}]")


def _check_stats(env, model, gpu, what):
    np.testing.assert_array_equal(env.stats_buf.cpu().numpy(), model, err_msg=f"{what}: the slots")
    m = torch.from_numpy(model).to(gpu)
    want = m.sum(0)
    want[4], want[5] = m[:, 4].min(), m[:, 5].max()
    rec = env.stats_record()
    assert torch.equal(rec, want), f"{what}: stats_record {rec.tolist()} != {want.tolist()}"
    es, w = env.episode_stats(), want.cpu().tolist()
    assert es["episodes"] == int(model[:, 0].sum()) and es["sum_return"] == w[1] and es["sum_return_sq"] == w[2]
    assert es["min_return"] == model[:, 4].min() and es["max_return"] == model[:, 5].max()
    assert es["mean_length"] == w[3] / w[0] and w[3] == model[:, 3].sum()


@pytest.mark.parametrize("variant", ["pool", "nopool", "nostats", "prev_read0", "two_windows"])
@pytest.mark.parametrize("N", SIZES)
def test_stats_slot_read_in_the_finishing_path(gpu, N, variant, monkeypatch):
    acts, ref = _reference(gpu, N)
    # TimeLimit 2: an env finishes at least every second step, so every wave takes the finishing
    # path at least four times in the eight steps.  Envs that collide early fall out of step with
    # the others, so a wave of many envs finishes one on most launches (a fold of a few lanes); the
    # lone env's wave is the one that certainly alternates with the lean path, which must leave the
    # slot alone
    assert sum(int(r["done"].sum()) for r in ref) >= STEPS // 2 * N
    if N == 1:
        assert sum(not r["done"].any() for r in ref) >= 2
    if variant == "nopool":
        monkeypatch.setenv("BALLENV_POOL", "0")
    if variant == "prev_read0":
        monkeypatch.setenv("BALLENV_PREV_READ", "0")
    env = make_env(_cfg(), N, W, gpu, seed=SEED, track_stats=variant != "nostats")
    assert env.kernel_name("step") == (NOPOOL if variant == "nopool" else POOL)
    assert (env.pool_bytes() > 0) == (variant != "nopool")
    slots = env.stats_buf.shape[0]
    assert slots >= (N + 31) // 32, "one statistics slot per wave of 32 envs"
    env.reset()
    model = _cleared(slots)
    for t in range(STEPS):
        if variant == "two_windows" and t == STEPS // 2:
            _check_stats(env, model, gpu, "the first window")
            assert model[:, 0].sum() >= STEPS // 4 * N
            env.clear_stats()
            model = _cleared(slots)
        got = _snapshot(env, env.step(acts[t]))
        _check_step(t, got, ref[t])
        _fold(model, ref[t])
        if variant == "nostats":   # no buffer handed to the kernel: ours stays as clear_stats() left it
            np.testing.assert_array_equal(env.stats_buf.cpu().numpy(), _cleared(slots), err_msg=f"t={t}")
        else:                      # after every launch: a lean step leaves the slots alone
            np.testing.assert_array_equal(env.stats_buf.cpu().numpy(), model, err_msg=f"t={t} slots")
    if variant != "nostats":
        _check_stats(env, model, gpu, "the last window")
        assert model[:, 0].sum() >= (STEPS // 4 if variant == "two_windows" else STEPS // 2) * N
    env.status()
    env.close()
