"""The reference's REINFORCE / supervised block-count policy and its batched, on-GPU select_action.

Reference:
* ``Policy``          examples/ball_env_reinforce.py:57-73 (and examples/test_model.py:57-85)
                      affine1 (29 -> 128) -> relu -> affine2 (128 -> 128) -> relu -> affine3 (-> 9)
                      -> relu -> softmax, on the ``prep_state2`` block counts (:130-172)
* ``Model``           examples/train_supervise.py:11-28: the same layers, no relu on the last
* ``select_action``   ball_env_reinforce.py:76-85   a ~ Categorical(probs); saved log_prob(a)
* ``finish_episode``  ball_env_reinforce.py:88-108  R^ = (R - mean) / (std + eps); loss = sum -log_prob * R^
* the stored weights  2 layers (affine2 is 9 x 128): ``with obs``, ``without obs_1``, ``without_obs_rand``;
                      3 layers: ``supervised``

``HipBlockPolicy`` runs that select_action for every env of a ``BatchedBallEnv`` in one launch of the
kernel in csrc/mlp_policy.hip (``be_mlp_act``), which computes ``prep_state2`` of each env's state
itself: the 29-byte row makes no round trip.  ``BlockRollout`` is the T-step loop of
``be_mlp_act`` + ``be_step`` writing straight into (T, N) buffers, capturable into HIP graphs, or with
backend="fused" the same steps as ``be_mlp_rollout`` launches (policy and env step in one kernel);
``reinforce_losses`` / ``reinforce_update`` are the batched ``finish_episode`` over such a record
(targets from ``be_a2c_targets``; gradients from torch autograd over the recorded rows, or with
grads="hip" from ``BlockGrad``: ``be_mlp_grad``, csrc/mlp_grad.hip, straight from the u8 rows).
``supervised_losses`` / ``supervised_update`` are one minibatch of examples/train_supervise.py:66-101 on the
same network (mean cross-entropy; ``reference_supervise_data`` is the reference's own training set).
``HipBlockOptim`` is the optimiser step of both loops (Adam / SGD) fused with the re-pack of the kernel's
weight image (``be_mlp_opt``); ``BlockTrainer`` and ``SupervisedTrainer`` are the two training loops with no
host round trip, replayable as HIP graphs.
``torch_block_select_action`` is the same computation in plain PyTorch fp32 -- the numerics
reference of the tests.
What these classes share with the other two policies lives in their bases: ``_bind.HipHandle`` (the handle),
``rollout.StepRollout`` (the T-step loop), ``optim.RowGrad`` (the gradient binding) and ``optim.HipOptim``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi
from ._bind import HipHandle, categorical_pick, golden, want
from .optim import HipOptim, RowGrad
from .rollout import GraphLoop, RolloutTrainer, StepRollout, a2c_targets, discounted, episode_ids

BLOCKS = 29                      # prep_state2's row: 4 quadrant + 5 x 5 blocks
# be_mlp_act's work split (csrc/mlp_policy.hip): a persistent grid of one workgroup per compute unit,
# WAVES waves each, a wave taking TILE envs per round (tile t of G workgroups: workgroup t % G, wave t // G % WAVES)
TILE, WAVES = 16, 8
# be_mlp_grad's (csrc/mlp_grad.hip): a persistent grid of one workgroup per compute unit (at most
# GRAD_MAX_SLOTS), GRAD_WAVES waves each, a workgroup taking GRAD_TILE rows per round (tile t of G workgroups:
# workgroup t % G, round t // G)
GRAD_TILE, GRAD_WAVES, GRAD_MAX_SLOTS = 64, 4, 1024
_KINDS = ("supervised3", "reinforce2")


def _names(layers: int) -> list:
    """The parameters of a BlockPolicy of this many layers, in the C structs' order."""
    return [f"affine{i + 1}.{w}" for i in range(layers) for w in ("weight", "bias")]


class BlockPolicy(nn.Module):
    """ball_env_reinforce.py:57-73 (the same parameter names, so the reference's state_dicts load).
    layers=2: affine1 -> relu -> affine2 (-> actions); hidden: an int, or (hidden1, hidden2)."""

    def __init__(self, layers: int = 3, hidden=128, num_actions: int = 9, final_relu: bool = True):
        super().__init__()
        if layers not in (2, 3):
            raise ValueError("layers must be 2 or 3")
        h1, h2 = (hidden, hidden) if isinstance(hidden, int) else (int(hidden[0]), int(hidden[1]))
        self.layers, self.final_relu, self.num_actions = int(layers), bool(final_relu), int(num_actions)
        self.hidden1, self.hidden2 = int(h1), int(h2) if layers == 3 else 0
        self.affine1 = nn.Linear(BLOCKS, self.hidden1)
        if layers == 3:
            self.affine2 = nn.Linear(self.hidden1, self.hidden2)
            self.affine3 = nn.Linear(self.hidden2, self.num_actions)
        else:
            self.affine2 = nn.Linear(self.hidden1, self.num_actions)

    def logits(self, x):
        x = F.relu(self.affine1(x))
        if self.layers == 3:
            x = self.affine3(F.relu(self.affine2(x)))
        else:
            x = self.affine2(x)
        return F.relu(x) if self.final_relu else x

    def forward(self, x):
        return F.softmax(self.logits(x), dim=-1)

    def linears(self):
        return [self.affine1, self.affine2] + ([self.affine3] if self.layers == 3 else [])

    @classmethod
    def from_npz(cls, path: str) -> "BlockPolicy":
        """Weights from a fixture written by tests/golden/make_block_policy_fixture.py."""
        d = np.load(path, allow_pickle=False)
        layers = int(d["layers"])
        w1, wl = d["affine1_weight"], d[f"affine{layers}_weight"]
        hidden = (w1.shape[0], d["affine2_weight"].shape[0] if layers == 3 else 0)
        pol = cls(layers, hidden, num_actions=wl.shape[0], final_relu=bool(int(d["final_relu"])))
        pol.load_state_dict({k: torch.from_numpy(d[k.replace(".", "_")]) for k in pol.state_dict()})
        return pol


def reference_block_weights(kind: str) -> Optional[str]:
    """Path of the committed fixture of one of the reference's trained block policies
    ("supervised3": 3 layers, no final relu; "reinforce2": 2 layers), if present."""
    if kind not in _KINDS:
        raise ValueError(f"kind must be one of {_KINDS}")
    return golden(f"block_policy_{kind}.npz")


def torch_block_select_action(policy: BlockPolicy, blocks: torch.Tensor, u: torch.Tensor):
    """select_action (ball_env_reinforce.py:76-85) for a batch, fp32, with the draw
    ``a = #{j : cdf_j <= u}`` (clamped to the last action with p > 0) from given uniforms ``u`` (N,)
    -- the rule the HIP kernel uses.  Returns (action int64, log_prob, probs)."""
    probs = policy(blocks.float())
    return (*categorical_pick(probs, u), probs)


class HipBlockPolicy(HipHandle):
    """``be_mlp_act`` bound to one BatchedBallEnv.

    ``load(policy)`` packs the module's current fp32 weights on the device (one small kernel,
    stream-ordered, graph-capturable) -- call it again after an optimiser step.  ``act()`` writes
    ``action`` (N,) u8, ``log_prob`` (N,) f32 and, if ``probs=True``, ``probs`` (N, A) f32.
    """

    ENTRIES = ("be_mlp_create", "be_mlp_destroy", "be_mlp_bytes")

    def __init__(self, env, policy: BlockPolicy, probs: bool = False, seed: Optional[int] = None):
        self.layers, self.hidden1, self.hidden2 = policy.layers, policy.hidden1, policy.hidden2
        self.final_relu = policy.final_relu
        super().__init__(env, (self.layers, self.hidden1, self.hidden2, policy.num_actions, int(self.final_relu)),
                         policy.num_actions, probs, seed)
        self.load(policy)

    def load(self, policy: BlockPolicy) -> None:
        if (policy.layers, policy.hidden1, policy.hidden2, policy.num_actions, policy.final_relu) != \
                (self.layers, self.hidden1, self.hidden2, self.num_actions, self.final_relu):
            raise ValueError("policy shape does not match this HipBlockPolicy")
        dev = self.env.device
        ws = []
        for lin in policy.linears():
            ws += [lin.weight.detach().to(device=dev, dtype=torch.float32).contiguous(),
                   lin.bias.detach().to(device=dev, dtype=torch.float32).contiguous()]
        ptrs = [w.data_ptr() for w in ws] + [None] * (6 - len(ws))
        _abi.check(self._lib.be_mlp_load(self._h, *ptrs, self.env._stream()), self.env._ctx)
        self._weights = ws          # keep alive until the packing kernel has run

    @property
    def rollout_kernel(self) -> Optional[str]:
        """The fused kernel instance ``be_mlp_rollout`` launches for this env and network
        (``be_mlp_rollout_kernel``), or None where it loops ``be_mlp_act`` + ``be_step``."""
        r = self._lib.be_mlp_rollout_kernel(self._h)
        return r.decode() if r else None

    def act(self, blocks: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None,
            seed: Optional[int] = None):
        """select_action for every env.  blocks: the (N, 29) u8 rows to run the forward on (default:
        ``prep_state2`` of the env's current state, computed in the kernel); record: an (N, 29) u8
        tensor that receives the rows ``env.observe_blocks()`` would return.
        Returns (action, log_prob, probs)."""
        env = self.env
        want(blocks, "blocks", torch.uint8, (env.num_envs, BLOCKS), env.device, optional=True)
        want(record, "record", torch.uint8, (env.num_envs, BLOCKS), env.device, optional=True)
        _abi.check(self._lib.be_mlp_act(self._h, C.byref(env._st), None if blocks is None else blocks.data_ptr(),
                                        None if record is None else record.data_ptr(), C.byref(self._out),
                                        self._seed(seed), env._stream()), env._ctx)
        return self.action, self.log_prob, self.probs


class BlockRollout(StepRollout):
    """T steps of every env with the block policy in the loop (ball_env_reinforce.py's episode loop,
    batched): per step ``be_mlp_act`` writes action and log_prob into row t (and, with ``record_obs``,
    the block counts the action was drawn from into row t of ``blocks`` (T, N, 29) u8), then ``be_step``
    writes rewards and dones into row t.  The loop, its (T, N) buffers, ``capture()`` and ``run()`` are
    ``StepRollout``'s (rollout.py).

    ``backend="fused"`` runs the same T steps as ``be_mlp_rollout`` launches of ``chunk`` steps each into the
    same buffers: the policy and the env step in one kernel, each env's state in registers and the packed
    weights in LDS (csrc/ballenv.hip's ``mlp_rollout_kernel``; bit-identical to ``"hip"``).  There is then
    nothing to capture: ``run()`` and ``run_eager()`` both issue the launches, and ``step(t)`` raises."""

    def __init__(self, env, policy: BlockPolicy, horizon: int, record_obs: bool = False, seed: int = 0x5E1EC7,
                 backend: str = "hip", chunk: int = 100):
        if backend not in ("hip", "fused"):
            raise ValueError("backend must be 'hip' or 'fused'")
        super().__init__(env, policy, HipBlockPolicy(env, policy, seed=int(seed)), horizon, seed, backend, chunk)
        self.blocks = torch.zeros(self.T, env.num_envs, BLOCKS, dtype=torch.uint8, device=env.device) \
            if record_obs else None

    def _launch(self, c0: int, k: int, act, s) -> int:
        env = self.env
        out = self._chunk_out(c0, None)
        rec = None if self.blocks is None else self.blocks[c0].data_ptr()
        return self._lib.be_mlp_rollout(self.hp._h, C.byref(env._st), env.obs.data_ptr(), rec, k, C.byref(out),
                                        C.byref(act), self.seed & (2**64 - 1), s)

    def _act(self, t: int, s) -> None:
        env = self.env
        rec = None if self.blocks is None else self.blocks[t].data_ptr()
        rc = self._lib.be_mlp_act(self.hp._h, C.byref(env._st), None, rec, C.byref(self._act_outs[t]),
                                  self.seed & (2**64 - 1), s)
        if rc:
            _abi.check(rc, env._ctx)


def _episode_targets(rewards: torch.Tensor, dones: torch.Tensor, gamma: float, eps: float):
    """(R^, valid), flat (T*N), by be_a2c_targets' rule in plain torch: the return recursion in f64,
    R rounded to fp32 (the reference's torch.tensor(R)), then each episode's mean and unbiased std of
    those fp32 values taken in f64 and R^ rounded once to fp32."""
    dev = rewards.device
    flat = discounted(rewards, dones, gamma).to(torch.float32).to(torch.float64).reshape(-1)
    sid, S = episode_ids(dones)
    cnt = torch.bincount(sid, minlength=S).to(torch.float64)
    mean = torch.zeros(S, dtype=torch.float64, device=dev).index_add_(0, sid, flat) / cnt
    var = torch.zeros(S, dtype=torch.float64, device=dev).index_add_(0, sid, (flat - mean[sid]) ** 2) / \
        (cnt - 1).clamp(min=1)
    Rn = ((flat - mean[sid]) / (var.sqrt()[sid] + eps)).to(torch.float32)
    return Rn, (cnt > 1)[sid]


def reinforce_losses(policy: BlockPolicy, blocks: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor,
                     dones: torch.Tensor, gamma: float = 0.99, targets=None) -> torch.Tensor:
    """Batched ``finish_episode`` (examples/ball_env_reinforce.py:88-108) over a recorded rollout.

    blocks (T, N, 29) u8 -- the rows each action was drawn from; actions (T, N); rewards (T, N) f64;
    dones (T, N) bool.  Every maximal run of an env's steps that ends at a done (or at the horizon)
    is one episode, as ``policy.rewards`` / ``policy.saved_log_probs`` are in the reference.  Per
    episode, as there: R_t = r_t + gamma R_{t+1}, then torch.tensor(R) (fp32),
    R^ = (R - R.mean()) / (R.std() + eps) (unbiased std, eps = fp32 eps), loss = sum_t -log pi(a_t|s_t) R^_t.
    Episodes of one step are left out (the reference's std() of one element is NaN).  log pi is
    recomputed from ``blocks`` with autograd, as ``Categorical(probs).log_prob``.  Returns the loss summed over all episodes (f64).

    targets: ``(returns_norm, valid)``, both (T, N) -- R^ and the "episode has >= 2 steps" mask from
    ``a2c_targets(env, rewards, dones, None, gamma)`` (one HIP kernel, the same normalisation)."""
    T, N = rewards.shape
    if targets is None:
        Rn, valid = _episode_targets(rewards, dones, gamma, float(np.finfo(np.float32).eps))
    else:
        Rn, valid = targets[0], targets[1]
        if tuple(Rn.shape) != (T, N) or tuple(valid.shape) != (T, N):
            raise ValueError("targets must be (returns_norm, valid), both (T, N)")
        Rn, valid = Rn.reshape(-1), valid.reshape(-1).to(torch.bool)
    probs = policy(blocks.reshape(T * N, BLOCKS).float())
    # the reference's m.log_prob(action): Categorical renormalises the probabilities and clamps them to
    # [eps, 1 - eps] before the log, so an action of probability ~0 has a finite loss and no gradient
    logp = torch.distributions.Categorical(probs=probs).log_prob(actions.reshape(-1).long())
    return -(logp.double() * Rn.double())[valid].sum()      # products and sum in f64: no rounding of its own


class BlockGrad(RowGrad):
    """``be_mlp_grad`` bound to one BatchedBallEnv and one BlockPolicy: the loss sum of ``reinforce_losses``
    (loss="reinforce") or of ``supervised_losses`` (loss="xent", with scale = 1 / batch for its mean) and
    what ``loss.backward()`` leaves in each ``.grad``, from the recorded u8 block counts in two launches.
    The workspace, the gradient tensors (``.grads``), the checks and ``assign()``: ``RowGrad`` (optim.py);
    ``.losses`` is its f64 pair (scale * the sum of the row losses, the number of active rows)."""

    LOSSES = {"reinforce": _abi.MLP_LOSS_REINFORCE, "xent": _abi.MLP_LOSS_XENT}
    LOSS_WIDTH = 2
    WEIGHTS, GRADS = _abi.BeMlpWeights, _abi.BeMlpGrads

    def __init__(self, env, policy: BlockPolicy):
        self.layers, self.hidden1, self.hidden2 = policy.layers, policy.hidden1, policy.hidden2
        self.num_actions, self.final_relu = policy.num_actions, policy.final_relu
        sizes = (self.layers, self.hidden1, self.hidden2, self.num_actions)
        super().__init__(env, policy, _names(self.layers), "be_mlp_grad_workspace_bytes", sizes,
                         (*sizes, int(self.final_relu)))
        self.losses = self._losses

    def __call__(self, blocks: torch.Tensor, actions: torch.Tensor, coef: Optional[torch.Tensor] = None,
                 valid: Optional[torch.Tensor] = None, loss: str = "reinforce", scale: float = 1.0):
        """blocks (T, N, 29) or (rows, 29) u8; actions u8 (the labels with loss="xent"), coef f32 or None
        (= 1), valid u8 / bool or None (= every row), each (T, N) or (rows,): contiguous, on the env's
        device.  Asynchronous on the caller's current stream.  Returns ``.grads``."""
        if loss not in self.LOSSES:
            raise ValueError("loss must be 'reinforce' or 'xent'")
        rows = self._rows(blocks, "blocks", BLOCKS,
                          ((actions, "actions", torch.uint8, False), (coef, "coef", torch.float32, True),
                           (valid, "valid", (torch.bool, torch.uint8), True)))
        ws, w = self._params()
        rc = self._lib.be_mlp_grad(self.env._ctx, blocks.data_ptr(), actions.data_ptr(),
                                   None if coef is None else coef.data_ptr(),
                                   None if valid is None else valid.data_ptr(), rows, self.LOSSES[loss], float(scale),
                                   C.byref(w), self.workspace.data_ptr(), self.workspace.numel() * 8,
                                   C.byref(self._g), self.env._stream())
        return self._ran(rc, ws)


class HipBlockOptim(HipOptim):
    """``be_mlp_opt`` bound to one ``HipBlockPolicy`` and its ``BlockPolicy`` module: ``torch.optim.Adam``
    (kind="adam": weight_decay=0, amsgrad=False, maximize=False -- ball_env_reinforce.py:196) or
    ``torch.optim.SGD`` (kind="sgd": momentum=0, weight_decay=0, no Nesterov -- train_supervise.py:75) on the
    four or six parameters in place *and* the re-pack of the new weights into ``hip_block_policy``, in one
    asynchronous entry (include/ballenv.h pins the arithmetic; reproducible bit for bit).  After ``step()``
    ``policy.state_dict()`` is current and ``be_mlp_act`` runs the new weights: no ``HipBlockPolicy.load``
    is needed.

    Owns the moments (adam: ``exp_avg`` / ``exp_avg_sq``, keyed like ``policy.state_dict()``), the device
    ``state`` [t, beta1^t, beta2^t, lr] and, with ``log_rows`` > 0, a (log_rows, 2) f64 ``loss_log``
    ring: the step that starts at count t copies the ``losses`` it is given (the 2 f64 of
    ``BlockGrad.losses``) into row t % log_rows.  Nothing is allocated per call and nothing synchronises,
    so a step can be graph-captured; the learning rate lives on the device, so a captured step follows
    ``opt.lr = ...``.  ``step``, ``state_dict`` and the rest: ``HipOptim`` (optim.py)."""

    KINDS = {"adam": (_abi.MLP_OPT_ADAM,), "sgd": (_abi.MLP_OPT_SGD,)}
    LOSS_WIDTH = 2
    STRUCT = _abi.BeMlpTensors
    ON, MODULE = "HipBlockPolicy", "a BlockPolicy module of the HipBlockPolicy's layer count"

    def __init__(self, hip_block_policy: HipBlockPolicy, policy: BlockPolicy, kind: str = "adam", lr: float = 1e-2,
                 betas=(0.9, 0.999), eps: float = 1e-8, log_rows: int = 0):
        hp = hip_block_policy
        h1, h2, A = hp.hidden1, hp.hidden2, hp.num_actions
        shapes = [(h1, BLOCKS), (h1,)] + ([(h2, h1), (h2,), (A, h2), (A,)] if hp.layers == 3 else [(A, h1), (A,)])
        super().__init__(hp, policy, _abi.lib().be_mlp_opt, _names(hp.layers), shapes, kind, lr, betas, eps, log_rows)


def _check_block_optim(optimizer, hp, policy) -> bool:
    """True for a HipBlockOptim (which must then be bound to this HipBlockPolicy and module)."""
    if not isinstance(optimizer, HipBlockOptim):
        return False
    if (hp is not None and optimizer.hp is not hp) or optimizer.policy is not policy:
        raise ValueError("the HipBlockOptim must be bound to this HipBlockPolicy and BlockPolicy")
    return True


def reinforce_update(rollout: BlockRollout, optimizer, gamma: float = 0.99, targets: str = "hip",
                     grads: str = "torch") -> float:
    """One REINFORCE step on a recorded rollout (record_obs=True): the targets (targets="hip":
    ``be_a2c_targets`` with no values; "torch": ``reinforce_losses``' own), loss.backward(),
    optimizer.step(), then the new weights re-packed for the HIP kernel.  Returns the loss value.
    grads: "torch" (``reinforce_losses`` + autograd) or "hip" (``BlockGrad``, cached on the rollout: the
    loss and every .grad from ``be_mlp_grad``, no autograd graph and no f32 copy of the rows; needs
    targets="hip").  optimizer: a torch optimiser, or with grads="hip" a ``HipBlockOptim`` bound to
    ``rollout.hp`` (the step reads ``BlockGrad.grads`` directly and re-packs: no .grad copies, no load)."""
    if rollout.blocks is None:
        raise ValueError("reinforce_update needs BlockRollout(record_obs=True)")
    if targets not in ("torch", "hip"):
        raise ValueError("targets must be 'torch' or 'hip'")
    if grads not in ("torch", "hip"):
        raise ValueError("grads must be 'torch' or 'hip'")
    hip_optim = _check_block_optim(optimizer, rollout.hp, rollout.policy)
    if hip_optim and grads != "hip":
        raise ValueError("a HipBlockOptim needs grads='hip'")
    if grads == "hip":
        if targets != "hip":
            raise ValueError("grads='hip' needs targets='hip'")
        t = a2c_targets(rollout.env, rollout.rewards, rollout.dones, None, gamma, with_returns=False)
        bg = getattr(rollout, "_block_grad", None)
        if bg is None or bg.policy is not rollout.policy:
            bg = rollout._block_grad = BlockGrad(rollout.env, rollout.policy)
        g = bg(rollout.blocks, rollout.actions, t.returns_norm, t.valid, loss="reinforce", scale=1.0)
        if hip_optim:
            optimizer.step(g, bg.losses)
            return float(bg.losses[0])
        bg.assign()
        loss = float(bg.losses[0])
        optimizer.step()
        rollout.hp.load(rollout.policy)
        return loss
    tg = None
    if targets == "hip":
        t = a2c_targets(rollout.env, rollout.rewards, rollout.dones, None, gamma, with_returns=False)
        tg = (t.returns_norm, t.valid)
    loss = reinforce_losses(rollout.policy, rollout.blocks, rollout.actions, rollout.rewards, rollout.dones, gamma,
                            targets=tg)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    rollout.hp.load(rollout.policy)
    return float(loss.detach())


def reference_supervise_data() -> Optional[str]:
    """Path of the committed fixture of the reference's supervised training data (one recorded trial:
    ``blocks`` (3186, 29) u8, ``labels`` (3186,) u8; tests/golden/make_supervise_fixture.py), if present."""
    return golden("supervise_trial2.npz")


def supervised_losses(policy: BlockPolicy, blocks: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The loss of examples/train_supervise.py:74, :90-97 for one minibatch: mean ``CrossEntropyLoss`` of the
    logits on blocks (B, 29) against labels (B,), in the module's own precision (plain torch: the
    numerics reference of ``be_mlp_grad``'s cross-entropy mode)."""
    x = blocks.to(policy.affine1.weight.dtype)
    return F.cross_entropy(policy.logits(x), labels.long())


def supervised_update(policy: BlockPolicy, blocks: torch.Tensor, labels: torch.Tensor, optimizer, grads: str = "torch",
                      grad: Optional[BlockGrad] = None) -> float:
    """One minibatch step of examples/train_supervise.py:90-101: the mean cross-entropy, its gradients,
    optimizer.step().  Returns the loss value.  grads: "torch" (``supervised_losses`` + autograd) or "hip"
    (``grad``, a ``BlockGrad`` made for ``policy``: ``be_mlp_grad`` with scale = 1 / batch; blocks u8
    and labels u8 or integer, on its env's device).  The caller re-packs a ``HipBlockPolicy`` (``load``)
    when it next acts with the new weights -- unless optimizer is a ``HipBlockOptim`` (grads="hip" only): its
    step reads ``grad.grads`` directly and re-packs its own ``HipBlockPolicy``."""
    if grads not in ("torch", "hip"):
        raise ValueError("grads must be 'torch' or 'hip'")
    hip_optim = _check_block_optim(optimizer, None, policy)
    if hip_optim and grads != "hip":
        raise ValueError("a HipBlockOptim needs grads='hip'")
    if grads == "hip":
        if grad is None or grad.policy is not policy:
            raise ValueError("grads='hip' needs grad=BlockGrad(env, policy)")
        if labels.dtype != torch.uint8:
            labels = labels.to(torch.uint8)
        g = grad(blocks, labels.contiguous(), None, None, loss="xent", scale=1.0 / max(1, int(blocks.shape[0])))
        if hip_optim:
            optimizer.step(g, grad.losses)
            return float(grad.losses[0])
        grad.assign()
        loss = float(grad.losses[0])
        optimizer.step()
        return loss
    loss = supervised_losses(policy, blocks, labels)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return float(loss.detach())


class BlockTrainer(RolloutTrainer):
    """The REINFORCE training loop (ball_env_reinforce.py:88-108, :196-230) with no host round trip between
    two rollouts: per iteration ``BlockRollout`` -> ``a2c_targets_into`` (no values) -> ``BlockGrad``
    ("reinforce", scale 1) -> ``HipBlockOptim("adam").step`` (which re-packs the policy), all enqueued on
    the caller's current stream with nothing allocated and no synchronise.

    Owns a ``BlockRollout(record_obs=True)``, preallocated ``A2CTargets`` (returns_norm and valid), a
    ``BlockGrad`` and a ``HipBlockOptim`` (``.opt``; ``log_rows`` sizes its loss log).  ``capture()`` records
    the rollout (``BlockRollout.capture``, ``chunk`` steps per graph) and the update half into HIP graphs,
    linear chains on one stream, which ``train()`` then replays.  ``backend="fused"``: the rollout half is
    ``be_mlp_rollout`` launches of ``chunk`` steps (nothing of it to capture), the update half still one graph.
    ``losses()``: the loss log as (iterations, 2) f64 on the host -- the REINFORCE loss and the active rows
    of each iteration, the last ``log_rows`` of them once the ring has wrapped (synchronises)."""

    def __init__(self, env, policy: BlockPolicy, horizon: int, gamma: float = 0.99, lr: float = 1e-2,
                 betas=(0.9, 0.999), eps: float = 1e-8, seed: int = 0x5E1EC7, log_rows: int = 0, chunk: int = 250,
                 backend: str = "hip"):
        super().__init__(env, policy, BlockRollout(env, policy, horizon, record_obs=True, seed=seed, backend=backend,
                                                   chunk=chunk), gamma)
        self.chunk = self.GRAPH_CHUNK = int(chunk)
        self.grad = BlockGrad(env, policy)
        self.opt = HipBlockOptim(self.rollout.hp, policy, "adam", lr=lr, betas=betas, eps=eps, log_rows=log_rows)

    def _grads(self, ro, tg):
        return self.grad(ro.blocks, ro.actions, tg.returns_norm, tg.valid, "reinforce", 1.0), self.grad.losses


class SupervisedTrainer(GraphLoop):
    """The supervised loop of examples/train_supervise.py:80-101 on device-resident data, with no host round
    trip: per minibatch ``BlockGrad`` ("xent", scale 1 / batch) -> ``HipBlockOptim("sgd").step``.

    blocks (rows, 29) u8 and labels (rows,) u8, contiguous on the env's device
    (``reference_supervise_data()`` is the reference's own set: 3186 rows, 16 minibatches of 200, the last
    of 186).  The minibatches are contiguous views in the data's order (the reference does not shuffle), so
    nothing is copied.  Owns a ``HipBlockPolicy`` (``.hp``: it acts with the weights of the last step), a
    ``BlockGrad`` and the ``HipBlockOptim`` (``.opt``).  ``capture()`` records one epoch as one HIP graph, a
    linear chain, which ``train()`` then replays.
    ``losses()``: the loss log as (steps, 2) f64 on the host -- each minibatch's mean cross-entropy and its
    row count, the last ``log_rows`` of them once the ring has wrapped (synchronises)."""

    def __init__(self, env, policy: BlockPolicy, blocks: torch.Tensor, labels: torch.Tensor, batch_size: int = 200,
                 lr: float = 1e-2, log_rows: int = 0):
        rows = int(want(blocks, "blocks", torch.uint8, (None, BLOCKS), env.device).shape[0])
        want(labels, "labels", torch.uint8, (rows,), env.device)
        if rows < 1:
            raise ValueError("blocks must have at least one row")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        self.env, self.policy, self.blocks, self.labels = env, policy, blocks, labels
        self.batch_size = int(batch_size)
        self.hp = self._closes = HipBlockPolicy(env, policy)
        self.grad = BlockGrad(env, policy)
        self.opt = HipBlockOptim(self.hp, policy, "sgd", lr=lr, log_rows=log_rows)
        self._batches = [(blocks[i:j], labels[i:j], 1.0 / (j - i))
                         for i in range(0, rows, self.batch_size) for j in (min(rows, i + self.batch_size),)]

    def epoch(self) -> None:
        """One pass over the minibatches, enqueued on the caller's current stream."""
        for b, l, scale in self._batches:
            self.opt.step(self.grad(b, l, None, None, "xent", scale), self.grad.losses)

    _pass = epoch

    def train(self, epochs: int) -> None:
        """``epochs`` passes, enqueued without a synchronise."""
        super().train(epochs)
