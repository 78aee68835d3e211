"""The pixel agent of examples/ball_cnn_reinforce.py on the batched env.

``PixelPolicy`` is the reference's ``Policy`` (:60-83) as a plain torch module: three 5 x 5 stride-2
convolutions with BatchNorm on the 40 x 40 patch image, then ``Linear(132, 9)`` on the 128 features
and the 4 quadrant inputs, softmax.  Its inputs come from the env's HIP observation kernels
(``BatchedBallEnv.observe_pixels`` / ``observe_blocks``); the network itself runs in torch.

    policy = PixelPolicy().to(env.device)
    image, quadrant = pixel_inputs(env)              # (N, 3, 40, 40) f32, (N, 4) f32
    probs = policy(image, quadrant)                  # (N, 9)

``HipPixelPolicy`` runs the reference's ``select_action`` (:85-95) for every env in one launch of the
kernel in csrc/cnn_policy.hip (``be_cnn_act``) on the u8 image ``be_observe_pixels`` writes; ``PixelRollout``
is the T-step loop ``observe_pixels -> be_cnn_act -> be_step`` into (T, N) buffers, capturable into HIP
graphs.  The handle is a ``_bind.HipHandle`` and the loop ``rollout.StepRollout``'s: the two classes here add
their own ``load()`` / ``act()`` and the policy half of a step.
The reference never calls ``policy.eval()`` and feeds one image at a time, so every BatchNorm layer normalises with the statistics of that env's own feature map: ``norm="sample"`` (the default of
the HIP path).  ``norm="running"`` uses the stored running statistics, as ``PixelPolicy.eval()`` does.
``torch_pixel_forward`` / ``torch_pixel_select_action`` are both modes in plain PyTorch -- the numerics
reference of the tests.
``pixel_reinforce_losses`` / ``pixel_reinforce_update`` are the batched ``finish_episode`` (:98-117) over a
recorded ``PixelRollout(record_images=True)``: gradients from torch autograd over the recorded images, or with
grads="hip" from ``PixelGrad`` (``be_cnn_grad``, csrc/cnn_grad.hip: the loss and all 14 gradients straight from
the u8 images, "sample" mode only -- the mode the reference trains in).
``HipPixelAdam`` is ``optimizer.step()`` of that loop (``optim.Adam(lr=1e-3)``, :115, :244) fused with the re-pack
of the weight image (``be_cnn_adam``); ``PixelTrainer`` is the training loop with no host round trip:
rollout -> targets -> ``PixelGrad`` -> ``HipPixelAdam.step``, enqueued or graph-replayed.
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
from .block_policy import _episode_targets
from .optim import HipOptim, RowGrad
from .rollout import RolloutTrainer, StepRollout, a2c_targets

# be_cnn_act's work split (csrc/cnn_host.h): a persistent grid of one workgroup per compute unit, WAVES waves
# each, a workgroup taking TILE envs per round (tile t of G workgroups: workgroup t % G, round t // G)
TILE, WAVES = 4, 8
# be_cnn_grad's (csrc/cnn_grad_host.h): a persistent grid of one workgroup per compute unit (at most
# GRAD_MAX_SLOTS), GRAD_WAVES waves each, a workgroup taking GRAD_TILE rows per round (tile t of G workgroups:
# workgroup t % G, round t // G)
GRAD_TILE, GRAD_WAVES, GRAD_MAX_SLOTS = 2, 8, 1024
IMAGE = (3, 40, 40)
NORMS = {"sample": _abi.CNN_NORM_SAMPLE, "running": _abi.CNN_NORM_RUNNING}
BN_EPS = 1e-5


class PixelPolicy(nn.Module):
    """ball_cnn_reinforce.py:60-83 (state_dict keys as the reference's: conv1..3, bn1..3, head)."""

    def __init__(self, num_actions: int = 9):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, kernel_size=5, stride=2)
        self.bn1 = nn.BatchNorm2d(16)
        self.conv2 = nn.Conv2d(16, 32, kernel_size=5, stride=2)
        self.bn2 = nn.BatchNorm2d(32)
        self.conv3 = nn.Conv2d(32, 32, kernel_size=5, stride=2)
        self.bn3 = nn.BatchNorm2d(32)
        self.head = nn.Linear(132, num_actions)       # 32 x 2 x 2 features + the quadrant one-hot

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.relu(self.bn3(self.conv3(x)))
        x = torch.cat((x.view(x.size(0), -1), y), 1)
        return F.softmax(self.head(x), dim=1)         # the reference's implicit dim of a 2-d input


def pixel_inputs(env):
    """Both inputs of :class:`PixelPolicy` for every env's current state: the (N, 3, 40, 40) f32
    patch image (extract_patch, :120-163) and the (N, 4) f32 quadrant one-hot of the goal (the first
    four block-count inputs, prep_state2's quadrant)."""
    return env.observe_pixels(f32=True), env.observe_blocks(f32=True)[:, :4]


def torch_pixel_forward(policy: PixelPolicy, image: torch.Tensor, quadrant: torch.Tensor,
                        norm: str = "sample") -> torch.Tensor:
    """``PixelPolicy``'s forward with the BatchNorm mode chosen by ``norm`` rather than by the module's
    train / eval flag, in the module's own precision: "sample" normalises each image's maps with
    their own statistics (``instance_norm``: biased variance, eps 1e-5 -- what the reference's
    ``train()``-mode forward of a batch of one computes), "running" with the stored running statistics
    (``eval()``).  image (N, 3, 40, 40) in [0, 1], quadrant (N, 4) one-hot; returns (N, A)
    probabilities.  Plain torch on any device, differentiable; no buffer is updated."""
    if norm not in NORMS:
        raise ValueError("norm must be 'sample' or 'running'")
    x = image
    for conv, bn in ((policy.conv1, policy.bn1), (policy.conv2, policy.bn2), (policy.conv3, policy.bn3)):
        x = conv(x)
        if norm == "sample":
            x = F.instance_norm(x, weight=bn.weight, bias=bn.bias, eps=bn.eps)
        else:
            x = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        x = F.relu(x)
    x = torch.cat((x.reshape(x.size(0), -1), quadrant.to(x.dtype)), 1)
    return F.softmax(policy.head(x), dim=1)


def torch_pixel_select_action(policy: PixelPolicy, image_u8: torch.Tensor, quadrant: torch.Tensor, u: torch.Tensor,
                              norm: str = "sample"):
    """select_action (ball_cnn_reinforce.py:85-95) for a batch, fp32: the forward on ``image_u8 / 255``
    (ToTensor) and the one-hot of ``quadrant`` ((N,) integers 0..3), then the draw
    ``a = #{j : cdf_j <= u}`` (clamped to the last action with p > 0) from given uniforms ``u`` (N,) -- the
    rule the HIP kernel uses.  Returns (action int64, log_prob, probs)."""
    x = image_u8.to(torch.float32) / 255.0
    q = F.one_hot(quadrant.long(), 4).to(torch.float32)
    probs = torch_pixel_forward(policy, x, q, norm)
    return (*categorical_pick(probs, u), probs)


def reference_pixel_weights() -> dict:
    """The ``state_dict`` of the reference's trained pixel policy
    (examples/stored_models/cnn_train_models/episode_900.pth), from the two committed fixtures
    tests/golden/pixel_policy_cnn.npz and pixel_policy_cnn_conv3.npz (make_pixel_policy_fixture.py);
    ``PixelPolicy().load_state_dict(reference_pixel_weights())`` loads it strictly."""
    sd = {}
    for name in ("pixel_policy_cnn.npz", "pixel_policy_cnn_conv3.npz"):
        with np.load(golden(name, required=True), allow_pickle=False) as d:
            for k in d.files:
                sd[k] = torch.from_numpy(np.array(d[k]))
    for i in (1, 2, 3):             # not a weight, not in the fixture: a fresh module's value
        sd[f"bn{i}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return {k: sd[k] for k in PixelPolicy().state_dict()}




class HipPixelPolicy(HipHandle):
    """``be_cnn_act`` bound to one BatchedBallEnv.

    ``load(policy)`` packs the module's current fp32 weights and BatchNorm buffers on the device (one
    small kernel, stream-ordered, graph-capturable) -- call it again after an optimiser step.  ``act()``
    writes ``action`` (N,) u8, ``log_prob`` (N,) f32 and, if ``probs=True``, ``probs`` (N, A) f32.
    Owns the (N, 3, 40, 40) u8 ``image`` buffer ``act()`` observes into."""

    ENTRIES = ("be_cnn_create", "be_cnn_destroy", "be_cnn_bytes")
    SEED = 0

    def __init__(self, env, policy: PixelPolicy, norm: str = "sample", probs: bool = False,
                 seed: Optional[int] = None):
        if norm not in NORMS:
            raise ValueError("norm must be 'sample' or 'running'")
        self.norm = norm
        A = int(policy.head.out_features)
        self.image = torch.zeros(env.num_envs, *IMAGE, dtype=torch.uint8, device=env.device)
        super().__init__(env, (A,), A, probs, seed)
        self.load(policy)

    def load(self, policy: PixelPolicy) -> None:
        sd = policy.state_dict()
        shapes = {k: tuple(v.shape) for k, v in PixelPolicy(self.num_actions).state_dict().items()}
        if int(policy.head.out_features) != self.num_actions:
            raise ValueError("policy's num_actions does not match this HipPixelPolicy")
        for k in _abi.CNN_TENSORS:
            if k not in sd or tuple(sd[k].shape) != shapes[k]:
                raise ValueError(f"policy tensor {k} must have shape {shapes[k]}")
        dev = self.env.device
        ws = [sd[k].detach().to(device=dev, dtype=torch.float32).contiguous() for k in _abi.CNN_TENSORS]
        w = _abi.BeCnnWeights(*[t.data_ptr() for t in ws])
        _abi.check(self._lib.be_cnn_load(self._h, C.byref(w), self.env._stream()), self.env._ctx)
        self._weights = ws          # keep alive until the packing kernel has run

    def act(self, image: Optional[torch.Tensor] = None, quadrant: Optional[torch.Tensor] = None,
            seed: Optional[int] = None):
        """select_action for every env.  image: the (N, 3, 40, 40) u8 images to run the forward on
        (default: ``env.observe_pixels`` of the current state into this object's ``image`` buffer, one
        more launch); quadrant: (N,) u8 in 0..3 (default: the goal's quadrant of the current state,
        computed in the kernel).  Nothing is allocated: capturable.  Returns (action, log_prob, probs)."""
        env, N = self.env, self.env.num_envs
        image = env.observe_pixels(out=self.image) if image is None else \
            want(image, "image", torch.uint8, (N, *IMAGE), env.device)
        want(quadrant, "quadrant", torch.uint8, (N,), env.device, optional=True)
        _abi.check(self._lib.be_cnn_act(self._h, C.byref(env._st), image.data_ptr(),
                                        None if quadrant is None else quadrant.data_ptr(), NORMS[self.norm],
                                        C.byref(self._out), self._seed(seed), env._stream()), env._ctx)
        return self.action, self.log_prob, self.probs


class PixelRollout(StepRollout):
    """T steps of every env with the pixel policy in the loop (ball_cnn_reinforce.py's episode loop,
    batched): per step ``be_observe_pixels`` writes the images (with ``record_images`` into row t of
    ``images`` (T, N, 3, 40, 40) u8), ``be_cnn_act`` writes action and log_prob into row t, then
    ``be_step`` writes rewards and dones into row t.  With ``record_images`` ``be_observe_quadrant`` also
    writes the goal's quadrant into row t of ``quadrants`` (T, N) u8, which ``be_cnn_act`` then reads -- the
    value it would compute itself, so the steps are the same bit for bit.  The loop, its (T, N) buffers,
    ``capture()`` and ``run()`` are ``StepRollout``'s (rollout.py)."""

    def __init__(self, env, policy: PixelPolicy, horizon: int, norm: str = "sample", seed: int = 0,
                 record_images: bool = False):
        super().__init__(env, policy, HipPixelPolicy(env, policy, norm=norm, seed=int(seed)), horizon, seed)
        self.images = torch.zeros(self.T, env.num_envs, *IMAGE, dtype=torch.uint8, device=env.device) \
            if record_images else None
        self.quadrants = torch.zeros(self.T, env.num_envs, dtype=torch.uint8, device=env.device) \
            if record_images else None

    def _act(self, t: int, s) -> None:
        """observe + select_action of every env, results into row t."""
        env, lib = self.env, self._lib
        img = (self.hp.image if self.images is None else self.images[t]).data_ptr()
        rc = lib.be_observe_pixels(env._ctx, C.byref(env._st), None, img, None, s)
        if rc:
            _abi.check(rc, env._ctx)
        quad = None
        if self.quadrants is not None:
            quad = self.quadrants[t].data_ptr()
            rc = lib.be_observe_quadrant(env._ctx, C.byref(env._st), quad, s)
            if rc:
                _abi.check(rc, env._ctx)
        rc = lib.be_cnn_act(self.hp._h, C.byref(env._st), img, quad, NORMS[self.hp.norm],
                            C.byref(self._act_outs[t]), self.seed & (2**64 - 1), s)
        if rc:
            _abi.check(rc, env._ctx)


class PixelGrad(RowGrad):
    """``be_cnn_grad`` bound to one BatchedBallEnv and one PixelPolicy: the loss sum of
    ``pixel_reinforce_losses`` and what ``loss.backward()`` leaves in each of the 14 ``.grad``, from the
    recorded u8 images in three launches ("sample" mode: each image's own BatchNorm statistics; the conv
    biases' gradients are exact zeros there).  The workspace, the gradient tensors (``.grads``), the checks of
    the weights and ``assign()``: ``RowGrad`` (optim.py); ``.losses`` is its f64 pair (scale * the sum of the
    row losses, the number of active rows)."""

    LOSS_WIDTH = 2
    SLOTS = len(_abi.CNN_PARAMS)
    WEIGHTS, GRADS = _abi.BeCnnWeights, _abi.BeCnnGrads

    def __init__(self, env, policy: PixelPolicy):
        self.num_actions = int(policy.head.out_features)
        super().__init__(env, policy, _abi.CNN_PARAMS, "be_cnn_grad_workspace_bytes", (self.num_actions,), ())
        self.losses = self._losses

    def _params(self):
        """The module's 14 parameters, checked, and their be_cnn_weights (the running statistics NULL)."""
        ps, dev = dict(self.policy.named_parameters()), self.env.device
        if ps.keys() != set(self._names):
            raise ValueError("PixelGrad needs a PixelPolicy module")
        ws = {k: want(ps[k].detach(), f"policy parameter {k}", torch.float32, tuple(self.grads[k].shape), dev)
              for k in self._names}
        return list(ws.values()), self.WEIGHTS(*(ws[k].data_ptr() if k in ws else None for k in _abi.CNN_TENSORS))

    def __call__(self, images: torch.Tensor, quadrants: torch.Tensor, actions: torch.Tensor,
                 coef: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, scale: float = 1.0,
                 probs: Optional[torch.Tensor] = None):
        """images (T, N, 3, 40, 40) or (rows, 3, 40, 40) u8; quadrants u8 in 0..3, actions u8, coef f32 or None
        (= 1), valid u8 / bool or None (= every row), each (T, N) or (rows,); probs: an f32 tensor of that
        leading shape + (A,) that receives the forward's probabilities, or None: contiguous, on the env's
        device.  Asynchronous on the caller's current stream.  Returns ``.grads``."""
        dev = self.env.device
        lead = (None, None) if isinstance(images, torch.Tensor) and images.dim() == 5 else (None,)
        lead = tuple(want(images, "images", torch.uint8, (*lead, *IMAGE), dev).shape[:-3])
        want(quadrants, "quadrants", torch.uint8, lead, dev)
        want(actions, "actions", torch.uint8, lead, dev)
        want(coef, "coef", torch.float32, lead, dev, optional=True)
        want(valid, "valid", (torch.bool, torch.uint8), lead, dev, optional=True)
        want(probs, "probs", torch.float32, (*lead, self.num_actions), dev, optional=True)
        rows = 1
        for n in lead:
            rows *= int(n)
        ws, w = self._params()
        g = self._g
        if probs is not None:
            g = self.GRADS(*(self.grads[k].data_ptr() for k in self._names), self._losses.data_ptr(), probs.data_ptr())
        rc = self._lib.be_cnn_grad(self.env._ctx, images.data_ptr(), quadrants.data_ptr(), actions.data_ptr(),
                                   None if coef is None else coef.data_ptr(),
                                   None if valid is None else valid.data_ptr(), rows, float(scale), C.byref(w),
                                   self.num_actions, self.workspace.data_ptr(), self.workspace.numel() * 8,
                                   C.byref(g), self.env._stream())
        return self._ran(rc, ws)


class HipPixelAdam(HipOptim):
    """``be_cnn_adam`` bound to one ``HipPixelPolicy`` and its ``PixelPolicy`` module: ``torch.optim.Adam``
    (weight_decay=0, amsgrad=False, maximize=False -- ball_cnn_reinforce.py:115) on the 14 parameters in place
    *and* the re-pack of the new weights into ``hip_pixel_policy``, in one asynchronous entry
    (include/ballenv.h pins the arithmetic; reproducible bit for bit).  After ``step()``
    ``policy.state_dict()`` is current and ``be_cnn_act`` runs the new weights: no ``HipPixelPolicy.load`` is
    needed.  The BatchNorm running statistics are no parameters: the step leaves them, and their rows of the
    weight image, as the last ``load`` wrote them.

    Owns the moments (``exp_avg`` / ``exp_avg_sq``, keyed like ``policy.named_parameters()``, which is the
    order of ``torch.optim.Adam(policy.parameters())``'s state), the device ``state`` [t, beta1^t, beta2^t, lr]
    and, with ``log_rows`` > 0, a (log_rows, 2) f64 ``loss_log`` ring: the step that starts at count t copies
    the ``losses`` it is given (the 2 f64 of ``PixelGrad.losses``) into row t % log_rows.  Nothing is allocated
    per call and nothing synchronises, so a step can be graph-captured; the learning rate lives on the device,
    so a captured step follows ``opt.lr = ...``.  eps must be > 0: ``PixelGrad``'s conv-bias gradients are exact
    zeros, and 0 / (0 + eps) leaves those weights alone where 0 / 0 would make them NaN.  ``step``,
    ``state_dict`` and the rest: ``HipOptim`` (optim.py)."""

    KINDS = {"adam": ()}
    LOSS_WIDTH = 2
    SLOTS = len(_abi.CNN_PARAMS)
    STRUCT = _abi.BeCnnTensors
    ON, MODULE = "HipPixelPolicy", "a PixelPolicy module of the HipPixelPolicy's num_actions"

    def __init__(self, hip_pixel_policy: HipPixelPolicy, policy: PixelPolicy, lr: float = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-8, log_rows: int = 0):
        if float(eps) == 0.0:
            raise ValueError("HipPixelAdam needs eps > 0 (the conv biases' gradients are exact zeros: 0 / 0)")
        shapes = dict(PixelPolicy(hip_pixel_policy.num_actions).named_parameters())
        super().__init__(hip_pixel_policy, policy, _abi.lib().be_cnn_adam, _abi.CNN_PARAMS,
                         [tuple(shapes[k].shape) for k in _abi.CNN_PARAMS], "adam", lr, betas, eps, log_rows)

    def load_state_dict(self, sd: dict) -> None:
        if "eps" in sd["param_groups"][0] and float(sd["param_groups"][0]["eps"]) == 0.0:
            raise ValueError("HipPixelAdam needs eps > 0 (the conv biases' gradients are exact zeros: 0 / 0)")
        super().load_state_dict(sd)


def pixel_reinforce_losses(policy: PixelPolicy, images: torch.Tensor, quadrants: torch.Tensor, actions: torch.Tensor,
                           rewards: torch.Tensor, dones: torch.Tensor, gamma: float = 0.99, targets=None) -> torch.Tensor:
    """Batched ``finish_episode`` (examples/ball_cnn_reinforce.py:98-117) over a recorded rollout:
    ``block_policy.reinforce_losses`` for this network, in plain torch.

    images (T, N, 3, 40, 40) u8 and quadrants (T, N) u8 -- what each action was drawn from; actions (T, N);
    rewards (T, N) f64; dones (T, N) bool.  Every maximal run of an env's steps that ends at a done (or at the
    horizon) is one episode; per episode R_t = r_t + gamma R_{t+1}, torch.tensor(R) (fp32),
    R^ = (R - R.mean()) / (R.std() + eps), loss = sum_t -log pi(a_t|s_t) R^_t; episodes of one step are left
    out.  log pi is recomputed with autograd: ``torch_pixel_forward(norm="sample")`` in the module's own
    precision, then ``Categorical(probs).log_prob``.  Returns the loss summed over all episodes (f64).
    targets: ``(returns_norm, valid)``, both (T, N), from ``a2c_targets(env, rewards, dones, None, gamma)``."""
    T, N = rewards.shape
    if targets is None:
        Rn, valid = _episode_targets(rewards, dones, gamma, float(np.finfo(np.float32).eps))
    else:
        Rn, valid = targets[0], targets[1]
        if tuple(Rn.shape) != (T, N) or tuple(valid.shape) != (T, N):
            raise ValueError("targets must be (returns_norm, valid), both (T, N)")
        Rn, valid = Rn.reshape(-1), valid.reshape(-1).to(torch.bool)
    dtype = policy.conv1.weight.dtype
    x = images.reshape(T * N, *IMAGE).to(dtype) / 255.0
    q = F.one_hot(quadrants.reshape(-1).long(), 4).to(dtype)
    probs = torch_pixel_forward(policy, x, q, "sample")
    logp = torch.distributions.Categorical(probs=probs).log_prob(actions.reshape(-1).long())
    return -(logp.double() * Rn.double())[valid].sum()      # products and sum in f64: no rounding of its own


def pixel_reinforce_update(rollout: PixelRollout, optimizer, gamma: float = 0.99, targets: str = "hip",
                           grads: str = "torch") -> float:
    """One REINFORCE step on a recorded rollout (record_images=True, norm="sample"): the targets
    (targets="hip": ``be_a2c_targets`` with no values; "torch": ``pixel_reinforce_losses``' own),
    loss.backward(), optimizer.step(), then the new weights re-packed for the HIP kernel
    (``rollout.hp.load``).  Returns the loss value.  grads: "torch" (``pixel_reinforce_losses`` + autograd)
    or "hip" (``PixelGrad``, cached on the rollout: the loss and every .grad from ``be_cnn_grad``, no autograd
    graph and no f32 copy of the images; needs targets="hip").  optimizer: a torch optimiser over
    ``rollout.policy.parameters()``, or with grads="hip" a ``HipPixelAdam`` bound to ``rollout.hp`` (the step reads
    ``PixelGrad.grads`` directly and re-packs: no .grad copies, no load)."""
    if rollout.images is None:
        raise ValueError("pixel_reinforce_update needs PixelRollout(record_images=True)")
    if rollout.hp.norm != "sample":
        raise ValueError("pixel_reinforce_update needs a PixelRollout with norm='sample' (the mode the reference trains in)")
    if targets not in ("torch", "hip"):
        raise ValueError("targets must be 'torch' or 'hip'")
    if grads not in ("torch", "hip"):
        raise ValueError("grads must be 'torch' or 'hip'")
    hip_optim = isinstance(optimizer, HipPixelAdam)
    if hip_optim and (optimizer.hp is not rollout.hp or optimizer.policy is not rollout.policy):
        raise ValueError("the HipPixelAdam must be bound to this rollout's HipPixelPolicy and PixelPolicy")
    if hip_optim and grads != "hip":
        raise ValueError("a HipPixelAdam needs grads='hip'")
    if grads == "hip":
        if targets != "hip":
            raise ValueError("grads='hip' needs targets='hip'")
        t = a2c_targets(rollout.env, rollout.rewards, rollout.dones, None, gamma, with_returns=False)
        pg = getattr(rollout, "_pixel_grad", None)
        if pg is None or pg.policy is not rollout.policy:
            pg = rollout._pixel_grad = PixelGrad(rollout.env, rollout.policy)
        g = pg(rollout.images, rollout.quadrants, rollout.actions, t.returns_norm, t.valid, scale=1.0)
        if hip_optim:
            optimizer.step(g, pg.losses)
            return float(pg.losses[0])
        pg.assign()
        loss = float(pg.losses[0])
        optimizer.step()
        rollout.hp.load(rollout.policy)
        return loss
    tg = None
    if targets == "hip":
        t = a2c_targets(rollout.env, rollout.rewards, rollout.dones, None, gamma, with_returns=False)
        tg = (t.returns_norm, t.valid)
    loss = pixel_reinforce_losses(rollout.policy, rollout.images, rollout.quadrants, rollout.actions, rollout.rewards,
                                  rollout.dones, gamma, targets=tg)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    rollout.hp.load(rollout.policy)
    return float(loss.detach())


class PixelTrainer(RolloutTrainer):
    """The pixel agent's REINFORCE training loop (ball_cnn_reinforce.py:98-117, :244) with no host round
    trip between two rollouts: per iteration ``PixelRollout`` -> ``a2c_targets_into`` (no values) ->
    ``PixelGrad`` (scale 1) -> ``HipPixelAdam.step`` (which re-packs the policy), all enqueued on the caller's
    current stream with nothing allocated and no synchronise.

    Owns a ``PixelRollout(record_images=True, norm="sample")``, preallocated ``A2CTargets`` (returns_norm and
    valid), a ``PixelGrad`` and a ``HipPixelAdam`` (``.opt``; ``log_rows`` sizes its loss log).  ``capture()``
    records the rollout (``PixelRollout.capture``, ``chunk`` steps per graph) and the update half into HIP graphs,
    linear chains on one stream, which ``train()`` then replays.  ``losses()``: the loss log as (iterations, 2)
    f64 on the host -- the REINFORCE loss and the active rows of each iteration, the last ``log_rows`` of them
    once the ring has wrapped (synchronises)."""

    def __init__(self, env, policy: PixelPolicy, horizon: int, gamma: float = 0.99, lr: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8, seed: int = 0x5E1EC7, log_rows: int = 0, chunk: int = 250):
        super().__init__(env, policy, PixelRollout(env, policy, horizon, norm="sample", seed=seed, record_images=True),
                         gamma)
        self.chunk = self.GRAPH_CHUNK = int(chunk)
        self.grad = PixelGrad(env, policy)
        self.opt = HipPixelAdam(self.rollout.hp, policy, lr=lr, betas=betas, eps=eps, log_rows=log_rows)

    def _grads(self, ro, tg):
        return self.grad(ro.images, ro.quadrants, ro.actions, tg.returns_norm, tg.valid, scale=1.0), self.grad.losses
