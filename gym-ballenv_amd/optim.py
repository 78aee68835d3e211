"""What the on-GPU optimisers and gradient classes share.  ``HipOptim`` is the base of ``HipAdam`` (rollout.py:
``be_a2c_adam`` on the six ``Policy`` tensors), ``HipBlockOptim`` (block_policy.py: ``be_mlp_opt`` on the four
or six ``BlockPolicy`` tensors) and ``HipPixelAdam`` (pixel_policy.py: ``be_cnn_adam`` on the 14 ``PixelPolicy``
parameters).  The C entries take the same arguments behind their handle -- params, grads and
the two moments as tensor structs, the device state, the Adam constants, the losses and the loss log -- so
everything but the names, shapes, struct and entry lives here: the tensor checks, ``step()`` up to the
C call, the device state and learning rate, the loss-log ring and ``state_dict`` interchange with the torch
optimisers.  ``RowGrad`` is the same for ``A2CGrad``, ``BlockGrad`` and ``PixelGrad`` (``be_a2c_grad``, ``be_mlp_grad``,
``be_cnn_grad``): the
workspace, the gradient tensors, the checks of the weights and of the row tensors, and ``assign()``.  Also the
helpers of that surface other classes use: ``is_f32`` (the weight check: ``_bind.fits`` for f32),
``unrolled_log`` and ``_beta_powers``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _abi
from ._bind import fits, want


def is_f32(x, shape, device) -> bool:
    """x is a contiguous f32 tensor of this shape (a tuple) on this device: what every kernel here reads
    its weights, gradients and moments as."""
    return fits(x, torch.float32, tuple(shape), device)


def _beta_powers(t: int, betas):
    """(beta1^t, beta2^t) as the optimisers' device state holds them after t steps: the running f64
    products, one multiply per step (``beta ** t`` differs in the last bits)."""
    p1 = p2 = 1.0
    for _ in range(int(t)):
        p1 *= float(betas[0])
        p2 *= float(betas[1])
    return p1, p2


def unrolled_log(log: torch.Tensor, t: int) -> torch.Tensor:
    """A (rows, width) ring whose step s wrote row s % rows, after t steps: the last min(t, rows)
    entries in step order (a view or a rolled copy on ``log``'s device)."""
    rows = log.shape[0]
    return log[:t] if t <= rows else torch.roll(log, -(t % rows), 0)


class HipOptim:
    """An optimiser step fused with the re-pack of the policy kernel's weight image, in one asynchronous C
    entry (include/ballenv.h pins the arithmetic; reproducible bit for bit).  After ``step()``
    ``policy.state_dict()`` is current and the policy kernels run the new weights: no ``load`` is needed.

    Owns the moments (adam: ``exp_avg`` / ``exp_avg_sq``, keyed like ``policy.state_dict()``), the device
    ``state`` [t, beta1^t, beta2^t, lr] and, with ``log_rows`` > 0, a (log_rows, LOSS_WIDTH) f64
    ``loss_log`` ring: the step that starts at count t copies the ``losses`` it is given into row
    t % log_rows.  Nothing is allocated per call and nothing synchronises, so a step can be
    graph-captured; the learning rate lives on the device, so a captured step follows ``opt.lr = ...``.

    A subclass says what differs, as data: KINDS (kind -> the C arguments between the handle and the
    tensor structs), LOSS_WIDTH, STRUCT (the ctypes tensor struct, SLOTS pointers -- six unless the subclass says
    otherwise --: unused ones stay NULL),
    ON / MODULE (the messages' words for the policy handle and the module), and to ``__init__`` the entry
    and the parameters' names and shapes in the struct's order."""

    KINDS: dict = {}
    LOSS_WIDTH = 0
    SLOTS = 6
    STRUCT = None
    ON = MODULE = ""

    def __init__(self, hip_policy, policy, entry, names, shapes, kind: str, lr: float, betas, eps: float,
                 log_rows: int):
        who = type(self).__name__
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {sorted(self.KINDS)}")
        self.hp, self.policy, self.kind = hip_policy, policy, kind
        self.env = env = hip_policy.env
        self._lib, self._entry, self._lead = _abi.lib(), entry, self.KINDS[kind]
        dev = env.device
        self._names, self._name_set, self._shapes = tuple(names), frozenset(names), dict(zip(names, shapes))
        self._pad = (None,) * (self.SLOTS - len(self._names))
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0) or self.eps < 0.0 or lr < 0.0:
            raise ValueError(f"{who} needs betas in [0, 1), eps >= 0 and lr >= 0")
        self._params()                      # ValueError for a module this policy handle was not made for
        self.exp_avg = self.exp_avg_sq = None
        self._mv = (None, None)             # the moments' structs, by reference (kept alive in _m / _v)
        if kind == "adam":
            self.exp_avg = {k: torch.zeros(s, dtype=torch.float32, device=dev) for k, s in self._shapes.items()}
            self.exp_avg_sq = {k: torch.zeros(s, dtype=torch.float32, device=dev) for k, s in self._shapes.items()}
            self._m = self.STRUCT(*(self.exp_avg[k].data_ptr() for k in self._names), *self._pad)
            self._v = self.STRUCT(*(self.exp_avg_sq[k].data_ptr() for k in self._names), *self._pad)
            self._mv = (C.byref(self._m), C.byref(self._v))
        self._lr = float(lr)
        self.state = torch.tensor([0.0, 1.0, 1.0, self._lr], dtype=torch.float64, device=dev)
        self.loss_log = torch.zeros(int(log_rows), self.LOSS_WIDTH, dtype=torch.float64, device=dev) \
            if log_rows > 0 else None
        self._keep = None

    def _check(self, what: str, k: str, x) -> torch.Tensor:
        if not is_f32(x, self._shapes[k], self.env.device):
            raise ValueError(f"{what} {k} must be a contiguous f32 tensor of shape {self._shapes[k]} on the "
                             f"{self.ON}'s device")
        return x

    def _params(self):
        ps = dict(self.policy.named_parameters())
        if ps.keys() != self._name_set:
            raise ValueError(f"{type(self).__name__} needs {self.MODULE}")
        return [self._check("policy parameter", k, ps[k].detach()) for k in self._names]

    def step(self, grads=None, losses: Optional[torch.Tensor] = None) -> None:
        """One optimiser step and the re-pack, asynchronous on the caller's current stream.
        grads: the gradient class's ``.grads`` (a dict keyed like ``policy.state_dict()``), default: the
        parameters' ``.grad``.  losses: its LOSS_WIDTH f64 on the device, logged if there is a ``loss_log``."""
        ws = self._params()
        if grads is None:
            ps = dict(self.policy.named_parameters())
            if any(ps[k].grad is None for k in self._names):
                raise ValueError(f"{type(self).__name__}.step() without grads= needs every parameter's .grad")
            gs = [self._check("gradient of", k, ps[k].grad) for k in self._names]
        else:
            gs = [self._check("gradient of", k, grads[k]) for k in self._names]
        lp = gp = None
        if losses is not None and self.loss_log is not None:
            if not fits(losses, torch.float64, (None,) * losses.dim(), self.env.device) or \
                    losses.numel() != self.LOSS_WIDTH:
                raise ValueError(f"losses must be {self.LOSS_WIDTH} contiguous f64 on the {self.ON}'s device")
            lp, gp = losses.data_ptr(), self.loss_log.data_ptr()
        w = self.STRUCT(*(x.data_ptr() for x in ws), *self._pad)
        g = self.STRUCT(*(x.data_ptr() for x in gs), *self._pad)
        rc = self._entry(self.hp._h, *self._lead, C.byref(w), C.byref(g), *self._mv, self.state.data_ptr(),
                         self.betas[0], self.betas[1], self.eps, lp, gp,
                         0 if gp is None else self.loss_log.shape[0], self.env._stream())
        if rc:
            _abi.check(rc, self.env._ctx)
        self._keep = (ws, gs, losses)       # alive until the kernels have run

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.policy.zero_grad(set_to_none=set_to_none)

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float) -> None:
        self._lr = float(value)
        self.state[3:].fill_(self._lr)      # stream-ordered: steps enqueued earlier keep the old rate

    def step_count(self) -> int:
        """Steps taken so far (synchronises)."""
        return int(self.state[0].item())

    def losses(self) -> torch.Tensor:
        """The loss log on the host, (steps, LOSS_WIDTH) f64 in step order: the last ``log_rows`` steps once
        the ring has wrapped (synchronises)."""
        if self.loss_log is None:
            raise ValueError(f"{type(self).__name__}(log_rows=...) keeps the loss log")
        return unrolled_log(self.loss_log, self.step_count()).cpu()

    def _torch_optim(self):
        if self.kind == "adam":
            return torch.optim.Adam(self.policy.parameters(), lr=self._lr, betas=self.betas, eps=self.eps)
        return torch.optim.SGD(self.policy.parameters(), lr=self._lr)

    def state_dict(self) -> dict:
        """``torch.optim.Adam.state_dict()``'s (resp. ``torch.optim.SGD``'s) format, parameters in
        ``policy.parameters()`` order, so the torch optimiser's ``load_state_dict(...)`` continues this run
        (synchronises).  Plain SGD keeps no per-parameter state, so its ``state`` is empty and the step count
        (which only picks the loss log's row) does not travel."""
        state = {}
        if self.kind == "adam":
            t = self.step_count()
            if t > 0:
                state = {i: {"step": torch.tensor(float(t)), "exp_avg": self.exp_avg[k].clone(),
                             "exp_avg_sq": self.exp_avg_sq[k].clone()} for i, k in enumerate(self._names)}
        return {"state": state, "param_groups": self._torch_optim().state_dict()["param_groups"]}

    def load_state_dict(self, sd: dict) -> None:
        """From ``state_dict()`` of an optimiser of this class and kind or of the torch optimiser over
        ``policy.parameters()``.  adam: beta^t is rebuilt by the repeated f64 product the device runs, so a
        round trip continues bit for bit.  sgd: the learning rate is all there is; the step count stays."""
        who, n = type(self).__name__, len(self._names)
        if len(sd["param_groups"]) != 1 or len(sd["param_groups"][0]["params"]) != n:
            raise ValueError(f"{who} needs one parameter group over the {n} parameters of {self.MODULE}")
        grp, st = sd["param_groups"][0], sd["state"]
        if grp.get("weight_decay", 0) != 0 or grp.get("maximize", False):
            raise ValueError(f"{who} has no weight_decay or maximize")
        if self.kind == "sgd":
            if "betas" in grp:
                raise ValueError(f"this {who} is kind='sgd': not an SGD state_dict")
            if grp.get("momentum", 0) != 0 or grp.get("dampening", 0) != 0 or grp.get("nesterov", False):
                raise ValueError(f"{who}'s SGD has no momentum, dampening or Nesterov")
            if any(s.get("momentum_buffer") is not None for s in st.values()):
                raise ValueError(f"{who}'s SGD has no momentum buffers")
            self.lr = float(grp["lr"])
            return
        if "betas" not in grp or "eps" not in grp:
            raise ValueError(f"this {who} is kind='adam': not an Adam state_dict")
        if grp.get("amsgrad", False):
            raise ValueError(f"{who} has no amsgrad")
        steps = {int(float(st[i]["step"])) for i in st}
        if st and (len(st) != n or len(steps) != 1):
            raise ValueError(f"{who} needs the state of every parameter at one common step")
        t = steps.pop() if st else 0
        for j, k in enumerate(self._names):
            i = grp["params"][j]
            for mine, key in ((self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
                if st:
                    if tuple(st[i][key].shape) != self._shapes[k]:
                        raise ValueError(f"{key} of {k} has the wrong shape")
                    mine[k].copy_(st[i][key])
                else:
                    mine[k].zero_()
        self.betas, self.eps, self._lr = (float(grp["betas"][0]), float(grp["betas"][1])), float(grp["eps"]), \
            float(grp["lr"])
        p1, p2 = _beta_powers(t, self.betas)
        self.state.copy_(torch.tensor([float(t), p1, p2, self._lr], dtype=torch.float64))


class RowGrad:
    """A loss and its gradients over recorded rows, in one asynchronous C entry bound to one BatchedBallEnv and
    one policy module (include/ballenv.h pins the arithmetic; reproducible bit for bit).

    Owns the workspace, the gradient tensors (``.grads``, keyed like ``policy.state_dict()``) and the
    LOSS_WIDTH f64 ``_losses``; nothing is allocated per call, so a call can be graph-captured.  The weights
    are read from the module's parameters at call time (fp32, contiguous, on the env's device).

    A subclass says what differs, as data: LOSS_WIDTH, WEIGHTS and GRADS (the ctypes structs: SLOTS tensor
    pointers -- six unless the subclass says otherwise --, unused ones NULL, then the network's sizes resp. the
    losses), and to ``__init__`` the parameters'
    names in the structs' order, the name of its ``*_workspace_bytes`` entry with that entry's sizes, and the
    sizes that end WEIGHTS.  Its ``__call__`` checks its rows (``_rows``), makes the C call on ``_params()``
    and ends in ``_ran``."""

    LOSS_WIDTH = 0
    SLOTS = 6
    WEIGHTS = GRADS = None

    def __init__(self, env, policy, names, workspace_entry: str, workspace_sizes, sizes):
        self.env, self.policy = env, policy
        self._lib = _abi.lib()
        dev = env.device
        nbytes = int(getattr(self._lib, workspace_entry)(env._ctx, *workspace_sizes))
        if nbytes < 0:
            _abi.check(nbytes, env._ctx)
        self.workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        self._names, self._sizes, self._pad = tuple(names), tuple(sizes), (None,) * (self.SLOTS - len(names))
        sd = policy.state_dict()
        self.grads = {k: torch.zeros(sd[k].shape, dtype=torch.float32, device=dev) for k in self._names}
        self._losses = torch.zeros(self.LOSS_WIDTH, dtype=torch.float64, device=dev)
        self._g = self.GRADS(*(self.grads[k].data_ptr() for k in self._names), *self._pad, self._losses.data_ptr())
        self._weights = None

    def _params(self):
        """The module's parameters, checked, and their WEIGHTS struct."""
        ps, dev = dict(self.policy.named_parameters()), self.env.device
        ws = [want(ps[k].detach(), f"policy parameter {k}", torch.float32, tuple(self.grads[k].shape), dev)
              for k in self._names]
        return ws, self.WEIGHTS(*(x.data_ptr() for x in ws), *self._pad, *self._sizes)

    def _rows(self, x, name: str, width: int, others) -> int:
        """Check the u8 rows ``x`` ((T, N, width) or (rows, width)) and ``others``, each (tensor, name, dtype,
        optional) of x's leading shape; returns the number of rows."""
        dev = self.env.device
        lead = (None, None) if isinstance(x, torch.Tensor) and x.dim() == 3 else (None,)
        lead = tuple(want(x, name, torch.uint8, (*lead, width), dev).shape[:-1])
        for y, yname, dtype, optional in others:
            want(y, yname, dtype, lead, dev, optional)
        return math.prod(lead)

    def _ran(self, rc: int, ws):
        if rc:
            _abi.check(rc, self.env._ctx)
        self._weights = ws          # keep alive until the kernels have run
        return self.grads

    def assign(self) -> None:
        """The gradients of the last call into the module's ``.grad`` (copies; stream-ordered)."""
        for k, prm in self.policy.named_parameters():
            if prm.grad is None:
                prm.grad = self.grads[k].clone()
            else:
                prm.grad.copy_(self.grads[k])
