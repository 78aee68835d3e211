"""On-GPU policy rollouts of a BatchedBallEnv (BASELINE config 5).

The reference's A2C driver (examples/ball_cnn_ac3.py:573-600) runs one env on
the host: per step ``prep_state4`` -> ``.to(device)`` -> ``select_action`` ->
``.item()`` -> ``env.step``, and keeps ``policy.saved_actions`` /
``policy.rewards`` lists for ``finish_episode`` (:222-246).  Here a step of all
N envs is two launches that never leave the GPU:

    be_policy_act   obs (N, 4+W*W) u8  ->  action, log_prob, value   (HipPolicy)
    be_step         action             ->  obs, reward, done          (BatchedBallEnv)

and each launch writes straight into row t of the (T, N) trajectory buffers
(per-step ``be_out`` / ``be_act_out`` structs point into them: no copy
kernels).  ``capture()`` records the T-step loop into HIP graphs, so
``run()`` is one graph replay per chunk with no host work per step.  That loop
is ``StepRollout``, the base of ``Rollout`` here, ``BlockRollout``
(block_policy.py) and ``PixelRollout`` (pixel_policy.py): a subclass supplies
the policy launches of one step and, where it has one, the fused launch.

``backend="fused"`` runs the same T steps as ``be_policy_rollout`` launches of ``chunk``
steps each: select_action and the env step in one kernel, each env's state in
registers and the packed policy in LDS (bit-identical to ``"hip"``); ``step(t)``
raises there, as it does for every fused rollout.

``backend="torch"`` runs select_action as plain PyTorch fp32 (``Policy`` +
``torch_select_action`` on ``torch.rand`` uniforms) -- the PyTorch-ROCm policy
the BASELINE config names, kept as the comparison point.

``discounted_returns`` is the batched form of finish_episode's return
recursion (:224-227) with episode boundaries (done) cutting the sum
(``discounted``; with ``episode_ids`` the shared part of the two plain-torch
target functions, ``_torch_targets`` here and block_policy's ``_episode_targets``);
``a2c_losses`` / ``a2c_update`` are the whole finish_episode (per-episode
return normalisation, policy + value losses) over all envs at once, so a
training loop is rollout (HIP) -> update (torch autograd) -> re-pack (HIP).
``A2CGrad`` (``a2c_update(grads="hip")``) is the losses and ``loss.backward()``
of that update in one HIP entry (``be_a2c_grad``), straight from the u8 record
(optim.py's ``RowGrad`` is what it shares with ``BlockGrad``).
``HipAdam`` is ``optimizer.step()`` and the re-pack in one HIP entry (``be_a2c_adam``; optim.py's
``HipOptim`` is what it shares with the block policy's ``HipBlockOptim``), and
``A2CTrainer`` the loop rollout -> targets -> gradients -> Adam -> re-packed policy with no host
round trip between two rollouts, its update half replayed as one HIP graph.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _abi
from ._bind import want
from .optim import HipOptim, RowGrad, _beta_powers      # noqa: F401  (_beta_powers stays importable from here)
from .policy import HipPolicy, Policy, torch_select_action


class A2CTargets(NamedTuple):
    """What ``a2c_targets`` returns, each (T, N) on the env's device."""
    returns_norm: torch.Tensor              # f32 per-episode normalised return R^
    advantage: Optional[torch.Tensor]       # f32 R^ - values (None without values)
    valid: torch.Tensor                     # u8 1: the element's episode has >= 2 steps
    returns: Optional[torch.Tensor]         # f64 discounted return R


def a2c_targets(env, rewards: torch.Tensor, dones: torch.Tensor, values: Optional[torch.Tensor] = None,
                gamma: float = 0.99, eps: Optional[float] = None, bootstrap: Optional[torch.Tensor] = None,
                with_returns: bool = True) -> A2CTargets:
    """The targets of the batched ``finish_episode`` in one HIP kernel (``be_a2c_targets``).

    rewards (T, N) f64, dones (T, N) bool or u8 0/1, values (T, N) f32 or None, bootstrap (N) f64
    or None, all contiguous on ``env``'s device (N = env.num_envs).  The arithmetic is the one
    include/ballenv.h pins, so two calls on the same inputs agree bit for bit and ``returns``
    equals ``Rollout.discounted_returns``.  eps=None: fp32 eps, as in ``a2c_losses``.
    Asynchronous on the caller's current stream; with_returns=False skips the f64 output."""
    import numpy as np
    eps = float(np.finfo(np.float32).eps) if eps is None else float(eps)
    dev, N = env.device, env.num_envs
    T = want(rewards, "rewards", torch.float64, (None, N), dev).shape[0]
    if T < 1:
        raise ValueError("rewards must have at least one row")
    want(dones, "dones", (torch.bool, torch.uint8), (T, N), dev)
    want(values, "values", torch.float32, (T, N), dev, optional=True)
    want(bootstrap, "bootstrap", torch.float64, (N,), dev, optional=True)
    rn = torch.empty(T, N, dtype=torch.float32, device=dev)
    adv = torch.empty(T, N, dtype=torch.float32, device=dev) if values is not None else None
    valid = torch.empty(T, N, dtype=torch.uint8, device=dev)
    ret = torch.empty(T, N, dtype=torch.float64, device=dev) if with_returns else None
    return a2c_targets_into(env, rewards, dones, values, gamma, eps, bootstrap, A2CTargets(rn, adv, valid, ret))


def a2c_targets_into(env, rewards, dones, values, gamma: float, eps: float, bootstrap, out: A2CTargets) -> A2CTargets:
    """``a2c_targets`` into tensors the caller allocated (no allocation: usable under graph capture).
    The caller vouches for dtypes, shapes, contiguity and devices."""
    ptr = lambda x: None if x is None else x.data_ptr()
    o = _abi.BeA2COut(ptr(out.returns), ptr(out.returns_norm), ptr(out.advantage), ptr(out.valid))
    rc = _abi.lib().be_a2c_targets(env._ctx, rewards.data_ptr(), dones.data_ptr(), ptr(values), ptr(bootstrap),
                                   int(rewards.shape[0]), float(gamma), float(eps), C.byref(o), env._stream())
    if rc:
        _abi.check(rc, env._ctx)
    return out


_PARAMS = ("fc1.weight", "fc1.bias", "action_head.weight", "action_head.bias", "value_head.weight",
           "value_head.bias")


class A2CGrad(RowGrad):
    """``be_a2c_grad`` bound to one BatchedBallEnv and one Policy: the policy and value loss sums of
    ``a2c_losses`` and what ``loss.backward()`` leaves in the six ``.grad``, from the recorded u8
    observations in two launches.  The workspace, the six gradient tensors (``.grads``), the f64 ``_losses``,
    the checks and ``assign()``: ``RowGrad`` (optim.py)."""

    LOSS_WIDTH = 3
    WEIGHTS, GRADS = _abi.BeA2CWeights, _abi.BeA2CGrads

    def __init__(self, env, policy: Policy):
        self.hidden, self.num_actions = int(policy.hidden_layer), int(policy.action_head.out_features)
        if policy.fc1.in_features != env.obs_dim:
            raise ValueError("policy input size does not match the env's observation")
        sizes = (self.hidden, self.num_actions)
        super().__init__(env, policy, _PARAMS, "be_a2c_grad_workspace_bytes", sizes, sizes)

    def __call__(self, obs: torch.Tensor, actions: torch.Tensor, returns_norm: torch.Tensor, valid: torch.Tensor):
        """obs (T, N, F) or (rows, F) u8; actions u8, returns_norm f32, valid u8 or bool, each (T, N) or
        (rows,): contiguous, on the env's device.  Asynchronous on the caller's current stream.
        Returns ``.grads``."""
        rows = self._rows(obs, "obs", self.env.obs_dim,
                          ((actions, "actions", torch.uint8, False), (returns_norm, "returns_norm", torch.float32, False),
                           (valid, "valid", (torch.bool, torch.uint8), False)))
        ws, w = self._params()
        rc = self._lib.be_a2c_grad(self.env._ctx, obs.data_ptr(), actions.data_ptr(), returns_norm.data_ptr(),
                                   valid.data_ptr(), rows, C.byref(w), self.workspace.data_ptr(),
                                   self.workspace.numel() * 8, C.byref(self._g), self.env._stream())
        return self._ran(rc, ws)

    def losses(self):
        """(policy_loss, value_loss, count) of the last call as Python numbers (synchronises)."""
        pl, vl, n = self._losses.tolist()
        return pl, vl, int(n)


class HipAdam(HipOptim):
    """``be_a2c_adam`` bound to one ``HipPolicy`` and its ``Policy`` module: ``torch.optim.Adam``
    (weight_decay=0, amsgrad=False, maximize=False) on the six parameters in place *and* the re-pack of
    the new weights into ``hip_policy``, in one asynchronous entry (include/ballenv.h pins the
    arithmetic; reproducible bit for bit).  After ``step()`` ``policy.state_dict()`` is current and
    the policy kernels run the new weights: no ``HipPolicy.load`` is needed.

    Owns the moments (``exp_avg`` / ``exp_avg_sq``, keyed like ``policy.state_dict()``), the device
    ``state`` [t, beta1^t, beta2^t, lr] and, with ``log_rows`` > 0, a (log_rows, 3) f64 ``loss_log``
    ring: the step that starts at count t copies the ``losses`` it is given (the 3 f64 of ``A2CGrad``)
    into row t % log_rows.  Nothing is allocated per call and nothing synchronises, so a step can be
    graph-captured; the learning rate lives on the device, so a captured step follows ``opt.lr = ...``.
    ``step``, ``state_dict`` and the rest: ``HipOptim`` (optim.py)."""

    KINDS = {"adam": ()}
    LOSS_WIDTH = 3
    STRUCT = _abi.BeA2CTensors
    ON, MODULE = "HipPolicy", "a Policy module (fc1, action_head, value_head)"

    def __init__(self, hip_policy: HipPolicy, policy: Policy, lr: float = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-8, log_rows: int = 0):
        H, A, F = hip_policy.hidden, hip_policy.num_actions, hip_policy.env.obs_dim
        super().__init__(hip_policy, policy, _abi.lib().be_a2c_adam, _PARAMS,
                         ((H, F), (H,), (A, H), (A,), (1, H), (1,)), "adam", lr, betas, eps, log_rows)


def capture_graph(fn, dev, stream: Optional[torch.cuda.Stream] = None) -> torch.cuda.CUDAGraph:
    """One call of ``fn`` recorded into one HIP graph: synchronise, capture on ``stream`` (default a new
    one from torch's pool), synchronise."""
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev) if stream is None else stream):
        fn()
    torch.cuda.synchronize(dev)
    return g


def capture_steps(step, T: int, chunk: int, dev, stream: Optional[torch.cuda.Stream] = None) -> list:
    """``step(t, stream_ptr)`` for t = 0 .. T - 1 recorded into HIP graphs of ``chunk`` steps each, all on
    one stream: what ``StepRollout.capture`` keeps in ``_graphs``."""
    cap = torch.cuda.Stream(dev) if stream is None else stream
    chunk = max(1, int(chunk))

    def steps(c0):
        sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for t in range(c0, min(T, c0 + chunk)):
            step(t, sp)
    return [capture_graph(lambda: steps(c0), dev, cap) for c0 in range(0, T, chunk)]


class StepRollout:
    """The T-step loop of the three policies: per step the subclass's policy launches (``_act``), then
    ``be_step``, each writing straight into row t of the (T, N) ``actions`` u8 / ``log_probs`` f32 /
    ``values`` f32 (None without a value head) / ``rewards`` f64 / ``dones`` bool through the per-step
    ``_act_outs`` / ``_step_outs`` structs (no copy kernels).  ``capture()`` records the loop into HIP
    graphs (a linear chain on one stream) and ``run()`` replays them.

    ``backend="fused"``, where the subclass has one: the same T steps as launches of ``chunk`` steps each
    (``_launch``); nothing to capture then, ``run()`` and ``run_eager()`` both issue them, ``step(t)`` raises.

    obs_rows: a tensor whose row t receives the window obs step t writes (default: the env's obs buffer).
    ``begin()`` / ``end()`` bracket a horizon (nothing here)."""

    def __init__(self, env, policy, hp, horizon: int, seed: int, backend: str = "hip", chunk: int = 100,
                 values: bool = False, obs_rows: Optional[torch.Tensor] = None):
        self.env, self.policy, self.hp, self.T, self.seed = env, policy, hp, int(horizon), int(seed)
        self.backend, self.chunk = backend, max(1, int(chunk))
        dev, N, T = env.device, env.num_envs, self.T
        self.actions = torch.zeros(T, N, dtype=torch.uint8, device=dev)
        self.log_probs = torch.zeros(T, N, dtype=torch.float32, device=dev)
        self.values = torch.zeros(T, N, dtype=torch.float32, device=dev) if values else None
        self.rewards = torch.zeros(T, N, dtype=torch.float64, device=dev)
        self.dones = torch.zeros(T, N, dtype=torch.bool, device=dev)
        self._graphs = []
        self._lib = _abi.lib()
        self._act_outs = [self._act_out(t) for t in range(T)]
        o = env._out
        self._step_outs = [_abi.BeOut(o.obs if obs_rows is None else obs_rows[t].data_ptr(), o.obs_f32,
                                      self.rewards[t].data_ptr(), self.dones[t].data_ptr(), o.truncated,
                                      o.terminal_obs, o.final_return, o.final_len, o.stats) for t in range(T)]

    def _act_out(self, t: int):
        """The be_act_out whose outputs start at row t."""
        return _abi.BeActOut(self.actions[t].data_ptr(), self.log_probs[t].data_ptr(),
                             None if self.values is None else self.values[t].data_ptr(), None)

    def _chunk_out(self, c0: int, obs_ptr):
        """The be_out of a fused launch whose rewards and dones start at row c0."""
        return _abi.BeOut(obs_ptr, None, self.rewards[c0].data_ptr(), self.dones[c0].data_ptr(), None, None,
                          None, None, self.env._out.stats)

    def run_fused(self, stream_ptr=None) -> None:
        """The horizon as fused launches of ``chunk`` steps (backend="fused")."""
        env = self.env
        s = env._stream() if stream_ptr is None else stream_ptr
        self.begin()
        for c0 in range(0, self.T, self.chunk):
            rc = self._launch(c0, min(self.chunk, self.T - c0), self._act_out(c0), s)
            if rc:
                _abi.check(rc, env._ctx)

    def step(self, t: int, stream_ptr=None) -> None:
        """The policy's select_action + env step of every env, results into row t."""
        if self.backend == "fused":
            raise RuntimeError("backend='fused' has no single step: run() / run_eager() issue the fused launches")
        env = self.env
        s = env._stream() if stream_ptr is None else stream_ptr
        self._act(t, s)
        rc = self._lib.be_step(env._ctx, C.byref(env._st), C.c_void_p(self.actions[t].data_ptr()), None, None,
                               C.byref(self._step_outs[t]), s)
        if rc:
            _abi.check(rc, env._ctx)

    def begin(self) -> None:
        pass

    def end(self) -> None:
        pass

    def _warm(self) -> None:
        """What must run eagerly once before a capture (nothing here)."""

    def run_eager(self) -> None:
        if self.backend == "fused":
            return self.run_fused()
        self.begin()
        for t in range(self.T):
            self.step(t)
        self.end()

    def capture(self, chunk: int = 250, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Record the T steps into HIP graphs of ``chunk`` steps each (stream: the stream to capture
        on; default a new one from torch's pool)."""
        if self.backend == "fused":     # a few launches per horizon: nothing to capture
            self._graphs = []
            return
        self._warm()
        self._graphs = capture_steps(self.step, self.T, chunk, self.env.device, stream)

    def run(self) -> None:
        """Replay the captured horizon (capture() first)."""
        if self.backend == "fused":
            return self.run_fused()
        if not self._graphs:
            raise RuntimeError("capture() first")
        self.begin()
        for g in self._graphs:
            g.replay()
        self.end()

    def close(self) -> None:
        self._graphs = []
        if self.hp is not None:
            self.hp.close()


class Rollout(StepRollout):
    """``StepRollout`` with the A2C ``Policy``: ``be_policy_act`` + ``be_step`` per step ("hip"),
    ``be_policy_rollout`` launches ("fused") or select_action in plain PyTorch ("torch": ``hp`` is None).
    record_obs: ``obs`` (T + 1, N, F) u8, row t the obs action t was chosen from."""

    def __init__(self, env, policy: Policy, horizon: int, backend: str = "hip", record_obs: bool = False,
                 seed: int = 0x5E1EC7, chunk: int = 100):
        if backend not in ("hip", "fused", "torch"):
            raise ValueError("backend must be 'hip', 'fused' or 'torch'")
        dev = env.device
        self.obs = torch.zeros(int(horizon) + 1, env.num_envs, env.obs_dim, dtype=torch.uint8, device=dev) \
            if record_obs else None
        hp = HipPolicy(env, policy, seed=int(seed)) if backend != "torch" else None
        super().__init__(env, policy, hp, horizon, seed, backend, chunk, values=True,
                         obs_rows=None if self.obs is None else self.obs[1:])
        if hp is None:
            self.policy = policy.to(dev)     # draws: torch.rand on the default (graph-safe) generator

    def _launch(self, c0: int, k: int, act, s) -> int:
        env = self.env
        out = self._chunk_out(c0, self.obs[c0 + 1].data_ptr() if self.obs is not None else None)
        return self._lib.be_policy_rollout(self.hp._h, C.byref(env._st), env.obs.data_ptr(), env.obs.data_ptr(), k,
                                           C.byref(out), C.byref(act), self.seed & (2**64 - 1), s)

    def _act(self, t: int, s) -> None:
        env = self.env
        obs = self.obs[t] if self.obs is not None else env.obs
        if self.hp is not None:
            rc = self._lib.be_policy_act(self.hp._h, C.byref(env._st), obs.data_ptr(), C.byref(self._act_outs[t]),
                                         self.seed & (2**64 - 1), s)
            if rc:
                _abi.check(rc, env._ctx)
        else:
            with torch.no_grad():
                u = torch.rand(env.num_envs, device=env.device)
                a, lp, v, _ = torch_select_action(self.policy, obs, u)
                self.actions[t].copy_(a)
                self.log_probs[t].copy_(lp)
                self.values[t].copy_(v)

    def begin(self) -> None:
        """Make row 0 of the obs record the env's current obs (call after reset)."""
        if self.obs is not None:
            self.obs[0].copy_(self.env.obs)

    def end(self) -> None:
        """With record_obs the steps write obs into the record: leave the last one in env.obs."""
        if self.obs is not None:
            self.env.obs.copy_(self.obs[self.T])

    def _warm(self) -> None:
        if self.hp is None:
            # initialise the BLAS handles eagerly: hipBLASLt set-up is not capturable
            with torch.no_grad():
                self.policy(self.env.obs[:64].float())
            torch.cuda.synchronize(self.env.device)

    def discounted_returns(self, gamma: float = 0.99, bootstrap: Optional[torch.Tensor] = None) -> torch.Tensor:
        """R_t = r_t + gamma * R_{t+1} * (1 - done_t), per env (finish_episode, ball_cnn_ac3.py:224-227)."""
        return discounted(self.rewards, self.dones, gamma, bootstrap)

    def targets(self, gamma: float = 0.99, bootstrap: Optional[torch.Tensor] = None,
                with_returns: bool = True) -> A2CTargets:
        """``a2c_targets`` of this rollout's rewards, dones and values (one HIP kernel)."""
        return a2c_targets(self.env, self.rewards, self.dones, self.values, gamma, None, bootstrap, with_returns)


def discounted(rewards: torch.Tensor, dones: torch.Tensor, gamma: float,
               bootstrap: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The return recursion R_t = r_t + gamma R_{t+1} (1 - done_t) per env in f64, (T, N); R_T = bootstrap (N)
    or 0.  The one loop of ``_torch_targets``, block_policy's ``_episode_targets`` and
    ``Rollout.discounted_returns``."""
    T, N = rewards.shape
    keep = 1.0 - dones.to(torch.float64)
    acc = torch.zeros(N, dtype=torch.float64, device=rewards.device) if bootstrap is None \
        else bootstrap.to(torch.float64).clone()
    R = torch.empty(T, N, dtype=torch.float64, device=rewards.device)
    for t in range(T - 1, -1, -1):
        acc = rewards[t].to(torch.float64) + gamma * acc * keep[t]
        R[t] = acc
    return R


def episode_ids(dones: torch.Tensor):
    """(sid, S): the episode id 0 .. S - 1 of every (t, env), flat (T*N) -- dones strictly before t in that
    env, then env -- and the number of episodes."""
    N = dones.shape[1]
    d = dones.to(torch.int64)
    seg = (torch.cumsum(d, 0) - d) * N + torch.arange(N, device=dones.device)
    _, sid = torch.unique(seg.reshape(-1), return_inverse=True)
    return sid, int(sid.max()) + 1


def _torch_targets(rewards: torch.Tensor, dones: torch.Tensor, gamma: float = 0.99, eps: Optional[float] = None):
    """The per-episode normalised returns of ``a2c_losses`` in plain torch: (Rn, valid), flat (T*N).
    The episode statistics are taken in f32."""
    import numpy as np
    eps = float(np.finfo(np.float32).eps) if eps is None else eps
    dev = rewards.device
    flat = discounted(rewards, dones, gamma).to(torch.float32).reshape(-1)
    sid, S = episode_ids(dones)
    cnt = torch.bincount(sid, minlength=S).to(torch.float32)
    mean = torch.zeros(S, device=dev).index_add_(0, sid, flat) / cnt
    dev2 = (flat - mean[sid]) ** 2
    var = torch.zeros(S, device=dev).index_add_(0, sid, dev2) / (cnt - 1).clamp(min=1)
    valid = (cnt > 1)[sid]
    Rn = (flat - mean[sid]) / (var.sqrt()[sid] + eps)
    return Rn, valid


def a2c_losses(policy: Policy, obs: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor,
               dones: torch.Tensor, gamma: float = 0.99, eps: Optional[float] = None, targets=None):
    """Batched ``finish_episode`` (examples/ball_cnn_ac3.py:222-246) over a recorded rollout.

    obs (T, N, F) u8 -- the obs each action was chosen from; actions (T, N); rewards (T, N)
    f64; dones (T, N) bool.  Every maximal run of an env's steps that ends at a done (or at
    the horizon) is one episode, as ``policy.rewards`` / ``policy.saved_actions`` are in the
    reference.  Per episode, exactly as there:
      R_t = r_t + gamma R_{t+1} (python floats), then torch.tensor(R) (fp32),
      R^ = (R - R.mean()) / (R.std() + eps)          (unbiased std, eps = fp32 eps),
      policy loss  sum_t -log pi(a_t|s_t) * (R^_t - v_t.item()),
      value loss   sum_t smooth_l1(v_t, R^_t).
    Episodes of one step are skipped (the driver only trains when t > 0, :614).
    log pi and v are recomputed from ``obs`` with autograd (the rollout's own values are
    the same forward, taken without a graph).  Returns (policy_loss, value_loss) sums.

    targets: ``(returns_norm, valid)``, both (T, N) -- R^ and the "episode has >= 2 steps" mask
    computed elsewhere (``a2c_targets`` / ``Rollout.targets``: one HIP kernel); the return
    recursion and the per-episode statistics below are then skipped, the rest is the same.
    """
    T, N = rewards.shape
    if targets is None:
        Rn, valid = _torch_targets(rewards, dones, gamma, eps)
    else:
        Rn, valid = targets[0], targets[1]
        if tuple(Rn.shape) != (T, N) or tuple(valid.shape) != (T, N):
            raise ValueError("targets must be (returns_norm, valid), both (T, N)")
        Rn, valid = Rn.reshape(-1), valid.reshape(-1).to(torch.bool)
    probs, v = policy(obs.reshape(T * N, -1).float())
    v = v.squeeze(-1)
    logp = torch.log(probs.gather(-1, actions.reshape(-1, 1).long()).squeeze(-1))
    adv = Rn - v.detach()
    pl = -(logp * adv)[valid].sum()
    vl = torch.nn.functional.smooth_l1_loss(v[valid], Rn[valid], reduction="sum")
    return pl, vl


def _a2c_update_hip_grads(rollout: "Rollout", optimizer, gamma: float, targets: str) -> float:
    """a2c_update(grads="hip"): the losses and gradients from ``A2CGrad`` (cached on the rollout)."""
    T, N = rollout.rewards.shape
    if targets == "hip":
        t = rollout.targets(gamma, with_returns=False)
        Rn, valid = t.returns_norm, t.valid
    else:
        Rn, valid = _torch_targets(rollout.rewards, rollout.dones, gamma)
        Rn, valid = Rn.reshape(T, N).contiguous(), valid.reshape(T, N).contiguous()
    ag = getattr(rollout, "_a2c_grad", None)
    if ag is None or ag.policy is not rollout.policy:
        ag = rollout._a2c_grad = A2CGrad(rollout.env, rollout.policy)
    grads = ag(rollout.obs[:-1], rollout.actions, Rn, valid)
    if isinstance(optimizer, HipAdam):      # straight from A2CGrad's tensors: no .grad copies, no second load
        optimizer.step(grads, ag._losses)
        pl, vl, _ = ag.losses()
        return pl + vl
    ag.assign()
    pl, vl, _ = ag.losses()
    optimizer.step()
    if rollout.hp is not None:
        rollout.hp.load(rollout.policy)
    return pl + vl


def a2c_update(rollout: "Rollout", optimizer, gamma: float = 0.99, targets: str = "torch", grads: str = "torch"):
    """One A2C step on a recorded rollout (record_obs=True): loss.backward(), optimizer.step(),
    then re-pack the new weights for the HIP policy kernel.  Returns the loss value.
    targets: "torch" (a2c_losses' own recursion and statistics) or "hip" (``Rollout.targets``).
    grads: "torch" (a2c_losses + autograd) or "hip" (``A2CGrad``: the losses and every .grad from
    ``be_a2c_grad``, no autograd graph and no f32 copy of the observations)."""
    if rollout.obs is None:
        raise ValueError("a2c_update needs Rollout(record_obs=True)")
    if targets not in ("torch", "hip"):
        raise ValueError("targets must be 'torch' or 'hip'")
    if grads not in ("torch", "hip"):
        raise ValueError("grads must be 'torch' or 'hip'")
    hip_adam = isinstance(optimizer, HipAdam)
    if hip_adam and (optimizer.hp is not rollout.hp or optimizer.policy is not rollout.policy):
        raise ValueError("the HipAdam must be bound to rollout.hp and rollout.policy")
    if grads == "hip":
        return _a2c_update_hip_grads(rollout, optimizer, gamma, targets)
    tg = None
    if targets == "hip":
        t = rollout.targets(gamma, with_returns=False)
        tg = (t.returns_norm, t.valid)
    pl, vl = a2c_losses(rollout.policy, rollout.obs[:-1], rollout.actions, rollout.rewards, rollout.dones, gamma,
                        targets=tg)
    loss = pl + vl
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    if rollout.hp is not None and not hip_adam:      # a HipAdam step has re-packed rollout.hp
        rollout.hp.load(rollout.policy)
    return float(loss.detach())


class GraphLoop:
    """The loop of the three trainers: ``train(n)`` enqueues n passes on the caller's current stream without
    a synchronise -- per pass ``_rollout()`` (nothing here), then ``_pass()``, or the one HIP graph ``capture()``
    recorded of it.  A subclass sets ``env``, ``opt`` (the optimiser whose loss log ``losses()`` reads) and
    ``_closes`` (what ``close()`` closes) and defines ``_pass``."""

    _graph = None

    def _rollout(self) -> None:
        pass

    def capture(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Record one pass into one HIP graph, a linear chain.  stream: the stream to capture on; default
        a new one from torch's pool."""
        self._graph = capture_graph(self._pass, self.env.device, stream)

    def train(self, iterations: int) -> None:
        """``iterations`` passes, enqueued without a synchronise."""
        for _ in range(int(iterations)):
            self._rollout()
            if self._graph is not None:
                self._graph.replay()
            else:
                self._pass()

    def losses(self) -> torch.Tensor:
        """The optimiser's loss log on the host, one row per step in step order (synchronises)."""
        return self.opt.losses()

    def close(self) -> None:
        self._graph = None
        self._closes.close()


class RolloutTrainer(GraphLoop):
    """What ``A2CTrainer`` and ``BlockTrainer`` share: per iteration the rollout (replayed if it was captured),
    then ``update()``: ``a2c_targets_into`` (no values) into the preallocated ``.targets``, the gradients
    (``_grads``: the subclass's one call of ``.grad``; returns its grads and device losses) and ``opt.step``,
    which re-packs the policy.  A subclass makes ``.grad`` and ``.opt`` once this ``__init__`` has run."""

    GRAPH_CHUNK = 250               # rollout steps per captured graph

    def __init__(self, env, policy, rollout, gamma: float):
        import numpy as np
        self.env, self.policy, self.gamma = env, policy, float(gamma)
        self.rollout = self._closes = rollout
        T, N, dev = rollout.T, env.num_envs, env.device
        self.targets = A2CTargets(torch.zeros(T, N, dtype=torch.float32, device=dev), None,
                                  torch.zeros(T, N, dtype=torch.uint8, device=dev), None)
        self._eps = float(np.finfo(np.float32).eps)

    def update(self) -> None:
        """The update half on the recorded rollout: targets, gradients, Adam step + re-pack."""
        ro = self.rollout
        a2c_targets_into(self.env, ro.rewards, ro.dones, None, self.gamma, self._eps, None, self.targets)
        self.opt.step(*self._grads(ro, self.targets))

    _pass = update

    def _rollout(self) -> None:
        ro = self.rollout
        if ro._graphs:
            ro.run()
        else:
            ro.run_eager()

    def capture(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Record the rollout (its own ``capture``, ``GRAPH_CHUNK`` steps per graph) and ``update()`` (one
        graph) into HIP graphs, linear chains on one stream, which ``train()`` then replays.  stream: the
        stream to capture on; default a new one from torch's pool."""
        cap = torch.cuda.Stream(self.env.device) if stream is None else stream
        self.rollout.capture(chunk=self.GRAPH_CHUNK, stream=cap)
        super().capture(cap)


class A2CTrainer(RolloutTrainer):
    """The A2C training loop with no host round trip between two rollouts: per iteration
    rollout -> ``a2c_targets_into`` -> ``A2CGrad`` -> ``HipAdam.step`` (which re-packs the policy), all
    enqueued on the caller's current stream with nothing allocated and no synchronise.

    Owns a ``Rollout(record_obs=True)`` (``backend="fused"``: ``be_policy_rollout`` launches, nothing to
    capture; ``"hip"``: the policy and step kernels, graph-replayed after ``capture()``), preallocated
    ``A2CTargets``, an ``A2CGrad`` and a ``HipAdam`` (``.opt``; ``log_rows`` sizes its loss log).
    ``capture()`` records the update half (targets, gradients, Adam + re-pack, loss log) into one HIP
    graph, a linear chain on one stream, which ``train()`` then replays after each rollout.
    ``losses()``: the loss log as (iterations, 3) f64 on the host -- policy loss, value loss, active rows of
    each iteration, the last ``log_rows`` of them once the ring has wrapped (synchronises)."""

    def __init__(self, env, policy: Policy, horizon: int, gamma: float = 0.99, backend: str = "fused",
                 lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, seed: int = 0x5E1EC7, log_rows: int = 0,
                 chunk: int = 100):
        if backend not in ("fused", "hip"):
            raise ValueError("backend must be 'fused' or 'hip'")
        super().__init__(env, policy, Rollout(env, policy, horizon, backend=backend, record_obs=True, seed=seed,
                                              chunk=chunk), gamma)
        self.grad = A2CGrad(env, policy)
        self.opt = HipAdam(self.rollout.hp, policy, lr=lr, betas=betas, eps=eps, log_rows=log_rows)

    def _grads(self, ro, tg):
        return self.grad(ro.obs[:-1], ro.actions, tg.returns_norm, tg.valid), self.grad._losses
