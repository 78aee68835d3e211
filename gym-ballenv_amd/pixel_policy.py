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
graphs.  The reference never calls ``policy.eval()`` and feeds one image at a time, so every BatchNorm
layer normalises with the statistics of that env's own feature map: ``norm="sample"`` (the default of
the HIP path).  ``norm="running"`` uses the stored running statistics, as ``PixelPolicy.eval()`` does.
``torch_pixel_forward`` / ``torch_pixel_select_action`` are both modes in plain PyTorch -- the numerics
reference of the tests.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi
from .rollout import capture_steps

# be_cnn_act's work split (csrc/cnn_host.h): a persistent grid of one workgroup per compute unit, WAVES waves
# each, a workgroup taking TILE envs per round (tile t of G workgroups: workgroup t % G, round t // G)
TILE, WAVES = 4, 8
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
    cdf = probs.cumsum(-1)
    a = (cdf <= u.unsqueeze(-1)).sum(-1)
    nz = torch.arange(probs.shape[-1], device=probs.device).expand_as(probs).masked_fill(probs <= 0, 0)
    a = torch.minimum(a, nz.max(-1).values)
    logp = torch.log(probs.gather(-1, a.unsqueeze(-1))).squeeze(-1)
    return a, logp, probs


def reference_pixel_weights() -> dict:
    """The ``state_dict`` of the reference's trained pixel policy
    (examples/stored_models/cnn_train_models/episode_900.pth), from the two committed fixtures
    tests/golden/pixel_policy_cnn.npz and pixel_policy_cnn_conv3.npz (make_pixel_policy_fixture.py);
    ``PixelPolicy().load_state_dict(reference_pixel_weights())`` loads it strictly."""
    g = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tests", "golden")
    sd = {}
    for name in ("pixel_policy_cnn.npz", "pixel_policy_cnn_conv3.npz"):
        with np.load(os.path.join(g, name), allow_pickle=False) as d:
            for k in d.files:
                sd[k] = torch.from_numpy(np.array(d[k]))
    for i in (1, 2, 3):             # not a weight, not in the fixture: a fresh module's value
        sd[f"bn{i}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return {k: sd[k] for k in PixelPolicy().state_dict()}


class HipPixelPolicy:
    """``be_cnn_act`` bound to one BatchedBallEnv.

    ``load(policy)`` packs the module's current fp32 weights and BatchNorm buffers on the device (one
    small kernel, stream-ordered, graph-capturable) -- call it again after an optimiser step.  ``act()``
    writes ``action`` (N,) u8, ``log_prob`` (N,) f32 and, if ``probs=True``, ``probs`` (N, A) f32.
    Owns the (N, 3, 40, 40) u8 ``image`` buffer ``act()`` observes into."""

    def __init__(self, env, policy: PixelPolicy, norm: str = "sample", probs: bool = False, seed: int = 0):
        if norm not in NORMS:
            raise ValueError("norm must be 'sample' or 'running'")
        self.env, self.norm, self.seed = env, norm, int(seed)
        self._lib = _abi.lib()
        self.num_actions = int(policy.head.out_features)
        dev, N = env.device, env.num_envs
        self.action = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.log_prob = torch.zeros(N, dtype=torch.float32, device=dev)
        self.probs = torch.zeros(N, self.num_actions, dtype=torch.float32, device=dev) if probs else None
        self.image = torch.zeros(N, *IMAGE, dtype=torch.uint8, device=dev)
        self._out = _abi.BeActOut(self.action.data_ptr(), self.log_prob.data_ptr(), None,
                                  None if self.probs is None else self.probs.data_ptr())
        h = C.c_void_p()
        _abi.check(self._lib.be_cnn_create(env._ctx, self.num_actions, C.byref(h)), env._ctx)
        self._h = h
        self._weights = None
        self.load(policy)

    def load(self, policy: PixelPolicy) -> None:
        sd = policy.state_dict()
        want = {k: tuple(v.shape) for k, v in PixelPolicy(self.num_actions).state_dict().items()}
        if int(policy.head.out_features) != self.num_actions:
            raise ValueError("policy's num_actions does not match this HipPixelPolicy")
        for k in _abi.CNN_TENSORS:
            if k not in sd or tuple(sd[k].shape) != want[k]:
                raise ValueError(f"policy tensor {k} must have shape {want[k]}")
        dev = self.env.device
        ws = [sd[k].detach().to(device=dev, dtype=torch.float32).contiguous() for k in _abi.CNN_TENSORS]
        w = _abi.BeCnnWeights(*[t.data_ptr() for t in ws])
        _abi.check(self._lib.be_cnn_load(self._h, C.byref(w), self.env._stream()), self.env._ctx)
        self._weights = ws          # keep alive until the packing kernel has run

    @property
    def packed_bytes(self) -> int:
        return int(self._lib.be_cnn_bytes(self._h))

    def act(self, image: Optional[torch.Tensor] = None, quadrant: Optional[torch.Tensor] = None,
            seed: Optional[int] = None):
        """select_action for every env.  image: the (N, 3, 40, 40) u8 images to run the forward on
        (default: ``env.observe_pixels`` of the current state into this object's ``image`` buffer, one
        more launch); quadrant: (N,) u8 in 0..3 (default: the goal's quadrant of the current state,
        computed in the kernel).  Nothing is allocated: capturable.  Returns (action, log_prob, probs)."""
        env, N = self.env, self.env.num_envs
        if image is None:
            image = env.observe_pixels(out=self.image)
        elif image.dtype != torch.uint8 or tuple(image.shape) != (N, *IMAGE) or not image.is_contiguous() or \
                image.device != env.device:
            raise ValueError("image must be an (N, 3, 40, 40) contiguous u8 tensor on the env's device")
        if quadrant is not None and (quadrant.dtype != torch.uint8 or tuple(quadrant.shape) != (N,) or
                                     not quadrant.is_contiguous() or quadrant.device != env.device):
            raise ValueError("quadrant must be an (N,) contiguous u8 tensor on the env's device")
        s = self.seed if seed is None else int(seed)
        _abi.check(self._lib.be_cnn_act(self._h, C.byref(env._st), image.data_ptr(),
                                        None if quadrant is None else quadrant.data_ptr(), NORMS[self.norm],
                                        C.byref(self._out), s & (2**64 - 1), env._stream()), env._ctx)
        return self.action, self.log_prob, self.probs

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.env.device)
            self._lib.be_cnn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PixelRollout:
    """T steps of every env with the pixel policy in the loop (ball_cnn_reinforce.py's episode loop,
    batched): per step ``be_observe_pixels`` writes the images (with ``record_images`` into row t of
    ``images`` (T, N, 3, 40, 40) u8), ``be_cnn_act`` writes action and log_prob into row t, then
    ``be_step`` writes rewards and dones into row t.  The per-step out-structs point into the (T, N)
    buffers, so there are no copy kernels; ``capture()`` records the loop into HIP graphs (a linear chain
    on one stream) and ``run()`` replays them."""

    def __init__(self, env, policy: PixelPolicy, horizon: int, norm: str = "sample", seed: int = 0,
                 record_images: bool = False):
        self.env, self.policy, self.T, self.seed = env, policy, int(horizon), int(seed)
        dev, N, T = env.device, env.num_envs, self.T
        self.actions = torch.zeros(T, N, dtype=torch.uint8, device=dev)
        self.log_probs = torch.zeros(T, N, dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(T, N, dtype=torch.float64, device=dev)
        self.dones = torch.zeros(T, N, dtype=torch.bool, device=dev)
        self.images = torch.zeros(T, N, *IMAGE, dtype=torch.uint8, device=dev) if record_images else None
        self.hp = HipPixelPolicy(env, policy, norm=norm, seed=self.seed)
        self._lib = _abi.lib()
        self._graphs = []
        self._act_outs = [_abi.BeActOut(self.actions[t].data_ptr(), self.log_probs[t].data_ptr(), None, None)
                          for t in range(T)]
        o = env._out
        self._step_outs = [_abi.BeOut(o.obs, o.obs_f32, self.rewards[t].data_ptr(), self.dones[t].data_ptr(),
                                      o.truncated, o.terminal_obs, o.final_return, o.final_len, o.stats)
                           for t in range(T)]

    def step(self, t: int, stream_ptr=None) -> None:
        """observe + select_action + env step of every env, results into row t."""
        env, lib = self.env, self._lib
        s = env._stream() if stream_ptr is None else stream_ptr
        img = (self.hp.image if self.images is None else self.images[t]).data_ptr()
        calls = ((lib.be_observe_pixels, (env._ctx, C.byref(env._st), None, img, None, s)),
                 (lib.be_cnn_act, (self.hp._h, C.byref(env._st), img, None, NORMS[self.hp.norm],
                                   C.byref(self._act_outs[t]), self.seed & (2**64 - 1), s)),
                 (lib.be_step, (env._ctx, C.byref(env._st), C.c_void_p(self.actions[t].data_ptr()), None, None,
                                C.byref(self._step_outs[t]), s)))
        for fn, args in calls:
            rc = fn(*args)
            if rc:
                _abi.check(rc, env._ctx)

    def run_eager(self) -> None:
        for t in range(self.T):
            self.step(t)

    def capture(self, chunk: int = 250, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Record the T steps into HIP graphs of ``chunk`` steps each (stream: the stream to capture
        on; default a new one from torch's pool)."""
        self._graphs = capture_steps(self.step, self.T, chunk, self.env.device, stream)

    def run(self) -> None:
        """Replay the captured horizon (capture() first)."""
        if not self._graphs:
            raise RuntimeError("capture() first")
        for g in self._graphs:
            g.replay()

    def close(self) -> None:
        self._graphs = []
        self.hp.close()
