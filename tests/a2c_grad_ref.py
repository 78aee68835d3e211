"""The computation include/ballenv.h pins for be_a2c_grad, restated in numpy f64 without autograd,
the inputs of its tests, and the torch references (a2c_losses + autograd in f64 / f32) the GPU
test measures it against."""
import numpy as np
import torch

PARAMS = ("fc1.weight", "fc1.bias", "action_head.weight", "action_head.bias", "value_head.weight", "value_head.bias")


HIDDEN = {10: 208, 5: 128, 7: 72, 11: 256}      # the hidden size of a case that names none

# Cases (W, hidden, num_actions, rows) of tests/test_gpu_a2c_grad.py that the host test checks too
# (tests/test_a2c_grad_host.py::test_new_cases_kink_share).
# Shapes: A and hidden off the multiples the kernel pads to, each W, both sides of the instance
# bounds (hidden 128 / 129 at W = 5, 208 / 209 at W = 10), hidden tiles 14 .. 16.
SHAPE_CASES = [(5, 1, 1, 130), (7, 17, 15, 200), (10, 100, 5, 333), (5, 129, 9, 300), (5, 127, 9, 301),
               (5, 256, 4, 300), (1, 16, 3, 200), (2, 33, 2, 129), (3, 16, 1, 70), (4, 64, 9, 192),
               (6, 65, 7, 260), (8, 240, 9, 321), (9, 200, 14, 500), (10, 256, 9, 257), (10, 209, 9, 257)]
TILE_EDGE_CASES = [(10, 208, 9, 64), (10, 208, 9, 65), (5, 128, 9, 128)]


def multi_tile_cases(slots):
    """{name: (W, hidden, num_actions, rows, fixture)} with more than one 64-row tile per workgroup of
    a persistent grid of `slots` workgroups (workgroup b takes the tiles b, b + slots, ...)."""
    return {"w10": (10, 208, 9, 64 * (2 * slots + 5) + 37, False),      # 3 tiles or 2; the partial tile in round 3
            "w10-fixture": (10, 208, 9, 64 * (2 * slots + 5) + 37, True),
            "w5": (5, 128, 9, 64 * 3 * slots, False),                   # exactly 3 rounds
            "w11": (11, 256, 15, 64 * (slots + 3) + 1, False),          # 3 second tiles, the last of one row
            "w7": (7, 72, 9, 64 * (2 * slots + 1), False)}


def case_policy(W, hidden=None, num_actions=9, fixture=False):
    """The Policy of a case: the committed fixture, or torch.manual_seed(0)'s initialisation."""
    from gym_ballenv_amd.policy import Policy, reference_weights
    if fixture:
        pol = Policy.from_npz(reference_weights(W), W)
        assert (pol.hidden_layer, pol.action_head.out_features) == (hidden or HIDDEN[W], num_actions)
        return pol
    torch.manual_seed(0)
    return Policy(W, hidden=hidden or HIDDEN[W], num_actions=num_actions)


def case_inputs(pol, W, rows, num_actions=9):
    """make_inputs with seed 1000 + rows, and the relu-kink rows of `pol` among them."""
    obs, actions, rn, valid = make_inputs(np.random.default_rng(1000 + rows), rows, W, num_actions)
    return obs, actions, rn, valid, kink_rows(weights64(pol), obs)


def weights64(policy):
    """The six arrays of a Policy as numpy f64, keyed like state_dict()."""
    return {k: v.detach().cpu().double().numpy() for k, v in policy.state_dict().items()}


def make_inputs(rng, rows, W, num_actions=9):
    """obs: a one-hot quadrant and Bernoulli(0.15) window cells; uniform actions; Rn ~ N(0, 1) with every
    17th value tripled (both smooth-L1 branches occur); 90 % valid."""
    F = 4 + W * W
    obs = np.zeros((rows, F), np.uint8)
    obs[np.arange(rows), rng.integers(0, 4, rows)] = 1
    obs[:, 4:] = rng.random((rows, W * W)) < 0.15
    actions = rng.integers(0, num_actions, rows).astype(np.uint8)
    rn = rng.normal(0, 1, rows)
    rn[::17] *= 3
    rn = rn.astype(np.float32)
    valid = (rng.random(rows) < 0.9).astype(np.uint8)
    return obs, actions, rn, valid


def kink_rows(w, obs):
    """Rows with a hidden unit whose f64 pre-activation is within rounding of 0: in f32 such a row may
    take the other relu branch, which changes its whole contribution."""
    x = obs.astype(np.float64)
    W1, b1 = w["fc1.weight"], w["fc1.bias"]
    pre = x @ W1.T + b1
    mag = 1.0 + x @ np.abs(W1).T + np.abs(b1)
    return (np.abs(pre) < 1e-6 * mag).any(axis=1)


def a2c_grad_ref(w, obs, actions, rn, valid):
    """Gradients (keyed like state_dict()), losses (policy, value, count) and the sums of the absolute
    loss terms, all f64."""
    W1, b1, Wa, ba, Wv, bv = (w[k] for k in PARAMS)
    A = Wa.shape[0]
    actions = actions.astype(np.int64)
    act = (valid != 0) & (actions < A)
    x = obs[act].astype(np.float64)
    a, Rn = actions[act], rn[act].astype(np.float64)
    n = len(a)
    pre = x @ W1.T + b1
    h = np.maximum(pre, 0.0)
    z = h @ Wa.T + ba
    v = h @ Wv[0] + bv[0]
    m = z.max(axis=1, keepdims=True) if n else z
    lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0] if n else np.zeros(0)
    logp = z[np.arange(n), a] - lse
    adv = Rn - v
    pterm = -logp * adv
    d = v - Rn
    vterm = np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
    dv = np.where(np.abs(d) < 1, d, np.sign(d))
    dz = np.exp(z - lse[:, None])
    dz[np.arange(n), a] -= 1.0
    dz *= adv[:, None]
    dh = dz @ Wa + dv[:, None] * Wv[0][None, :]
    dpre = np.where(pre > 0, dh, 0.0)
    grads = {"fc1.weight": dpre.T @ x, "fc1.bias": dpre.sum(0), "action_head.weight": dz.T @ h,
             "action_head.bias": dz.sum(0), "value_head.weight": (dv @ h)[None, :], "value_head.bias": dv.sum(keepdims=True)}
    return {"grads": grads, "losses": (float(pterm.sum()), float(vterm.sum()), n),
            "abs_terms": (float(np.abs(pterm).sum()), float(np.abs(vterm).sum()))}


def torch_reference(policy, obs, actions, rn, valid, dtype, device="cpu"):
    """a2c_losses(targets=(Rn, valid)) + autograd of pl + vl on a copy of `policy` in `dtype` on `device`:
    ({name: grad}, (policy_loss, value_loss)) as f64 numpy / floats.  The arrays are (rows, ...)."""
    import copy
    from gym_ballenv_amd.rollout import a2c_losses
    pol = copy.deepcopy(policy).to(device=device, dtype=dtype)
    rows = obs.shape[0]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    fwd = pol if dtype == torch.float32 else (lambda x: pol(x.to(dtype)))
    dummy = torch.zeros(rows, 1, dtype=torch.float64, device=device)
    pl, vl = a2c_losses(fwd, t(obs).reshape(rows, 1, -1), t(actions).reshape(rows, 1), dummy, dummy.bool(),
                        targets=(t(rn).to(dtype).reshape(rows, 1), t(valid).reshape(rows, 1)))
    (pl + vl).backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().double().numpy()
             for k, p in pol.named_parameters()}
    return grads, (float(pl.detach().double()), float(vl.detach().double()))
