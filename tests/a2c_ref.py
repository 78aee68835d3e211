"""Scalar restatement of be_a2c_targets (include/ballenv.h, the six pinned steps) in numpy f64.

Vectorised over envs only: every sum runs over t in the pinned order, one IEEE operation at a
time (numpy's +, *, /, sqrt and astype on f64 / f32 arrays are correctly rounded and never
fused), so the kernel is expected to agree with it bit for bit.  Also the input generator the
CPU and GPU tests share.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)


def a2c_targets_ref(rewards, dones, values=None, bootstrap=None, gamma=0.99, eps=EPS):
    """rewards (T, N) f64, dones (T, N) bool, values (T, N) f32 or None, bootstrap (N) f64 or None.
    Returns dict(returns f64, returns_norm f32, advantage f32 or None, valid u8), each (T, N)."""
    rewards = np.asarray(rewards, np.float64)
    dones = np.asarray(dones).astype(bool)
    T, N = rewards.shape
    gamma, eps = np.float64(gamma), np.float64(eps)
    # 1. the return, t = T-1 .. 0
    R = np.empty((T, N), np.float64)
    acc = np.zeros(N, np.float64) if bootstrap is None else np.asarray(bootstrap, np.float64).copy()
    for t in range(T - 1, -1, -1):
        acc = np.where(dones[t], 0.0, acc)
        acc = rewards[t] + gamma * acc
        R[t] = acc
    # 2. its f32 rounding
    r32 = R.astype(np.float32)
    x = r32.astype(np.float64)
    end = dones.copy()
    end[T - 1] = True
    # 3. per-episode sum in decreasing t; at an episode's first step it is complete
    run_sum = np.empty((T, N), np.float64)
    run_len = np.empty((T, N), np.int64)
    s, L = np.zeros(N, np.float64), np.zeros(N, np.int64)
    for t in range(T - 1, -1, -1):
        s = np.where(end[t], 0.0, s)
        L = np.where(end[t], 0, L)
        s = s + x[t]
        L = L + 1
        run_sum[t], run_len[t] = s, L
    # 4. squared deviations in increasing t, from the episode's mean
    mean = np.empty((T, N), np.float64)
    length = np.empty((T, N), np.int64)
    run_ss = np.empty((T, N), np.float64)
    m, Lc, ss = np.zeros(N, np.float64), np.ones(N, np.int64), np.zeros(N, np.float64)
    for t in range(T):
        start = np.ones(N, bool) if t == 0 else end[t - 1]
        m = np.where(start, run_sum[t] / run_len[t].astype(np.float64), m)
        Lc = np.where(start, run_len[t], Lc)
        ss = np.where(start, 0.0, ss)
        d = x[t] - m
        ss = ss + d * d
        mean[t], length[t], run_ss[t] = m, Lc, ss
    # 5. / 6. normalisation with the episode's complete ss (carried back from its last step)
    rn = np.zeros((T, N), np.float32)
    valid = np.zeros((T, N), np.uint8)
    tot = np.zeros(N, np.float64)
    for t in range(T - 1, -1, -1):
        tot = np.where(end[t], run_ss[t], tot)
        ok = length[t] >= 2
        dof = np.where(ok, length[t] - 1, 1).astype(np.float64)
        den = np.sqrt(tot / dof) + eps
        with np.errstate(divide="ignore", invalid="ignore"):
            z = ((x[t] - mean[t]) / den).astype(np.float32)
        rn[t] = np.where(ok, z, np.float32(0))
        valid[t] = ok
    adv = None
    if values is not None:
        v = np.asarray(values, np.float32)
        adv = np.where(valid.astype(bool), rn - v, np.float32(0)).astype(np.float32)
    return {"returns": R, "returns_norm": rn, "advantage": adv, "valid": valid}


def make_case(rng, T, N, p_done, sigma, spikes):
    """rewards N(0, sigma) (+ 1 % entries of -8000, the env's collision penalty, when spikes),
    dones Bernoulli(p_done), drawn from rng in that order."""
    rewards = rng.normal(0, sigma, (T, N))
    dones = rng.random((T, N)) < p_done
    if spikes:
        rewards[rng.random((T, N)) < 0.01] = -8000.0
    return rewards, dones


def episodes(dones_col):
    """[(s, e)] of one env's (T,) dones: the cut of a2c_losses."""
    T, out, s = len(dones_col), [], 0
    for t in range(T):
        if dones_col[t] or t == T - 1:
            out.append((s, t))
            s = t + 1
    return out
