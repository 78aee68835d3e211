"""What the Python bindings of the three policies share (policy.py, block_policy.py, pixel_policy.py and the
rollouts, gradients and optimisers over them), next to the torch-free ``_abi``: ``fits`` / ``want`` (the one
check of a tensor argument: dtype, shape, contiguity, device), ``categorical_pick`` (the inverse-CDF draw of
the three kernels in plain torch), ``golden`` (the path of a committed fixture) and ``HipHandle`` (the base
of ``HipPolicy``, ``HipBlockPolicy`` and ``HipPixelPolicy``: the C handle's life, the output buffers, the seed).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _abi

_DTYPES = {torch.uint8: "u8", torch.bool: "bool", torch.float32: "f32", torch.float64: "f64"}


def fits(x, dtype, shape, device) -> bool:
    """x is a contiguous tensor of this dtype (one, or a tuple of them) and shape (a tuple; None: any extent)
    on this device: what every kernel here reads its arguments as."""
    return isinstance(x, torch.Tensor) and x.dtype in (dtype if isinstance(dtype, tuple) else (dtype,)) and \
        x.dim() == len(shape) and all(s is None or s == n for s, n in zip(shape, x.shape)) and \
        x.is_contiguous() and x.device == device


def want(x, name: str, dtype, shape, device, optional: bool = False):
    """``x`` if it ``fits`` (or is None and ``optional``), else ValueError naming the argument."""
    if not (fits(x, dtype, shape, device) or (x is None and optional)):
        dts = " / ".join(_DTYPES.get(d, str(d)) for d in (dtype if isinstance(dtype, tuple) else (dtype,)))
        dims = ", ".join("*" if s is None else str(int(s)) for s in shape)
        raise ValueError(f"{name} must be a contiguous {dts} tensor of shape ({dims}) on the env's device")
    return x


def categorical_pick(probs: torch.Tensor, u: torch.Tensor):
    """The draw of the three policy kernels from probabilities (N, A) and uniforms ``u`` (N,):
    ``a = #{j : cdf_j <= u}``, clamped to the last action with p > 0.  Returns (action int64, log p_a)."""
    cdf = probs.cumsum(-1)
    a = (cdf <= u.unsqueeze(-1)).sum(-1)
    nz = torch.arange(probs.shape[-1], device=probs.device).expand_as(probs).masked_fill(probs <= 0, 0)
    a = torch.minimum(a, nz.max(-1).values)
    return a, torch.log(probs.gather(-1, a.unsqueeze(-1))).squeeze(-1)


def golden(name: str, required: bool = False) -> Optional[str]:
    """Path of the committed fixture tests/golden/<name>; if it is missing None, or with ``required``
    FileNotFoundError."""
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tests", "golden", name)
    if os.path.exists(p):
        return p
    if required:
        raise FileNotFoundError(p)
    return None


class HipHandle:
    """A policy kernel's C handle bound to one BatchedBallEnv: the ``action`` (N,) u8, ``log_prob`` (N,) f32,
    ``value`` (N,) f32 (None without a value head) and, with ``probs=True``, ``probs`` (N, A) f32 buffers
    ``act()`` writes, their ``be_act_out`` struct (``_out``), the seed and the handle's life.

    A subclass says what differs, as data: ENTRIES (the names of its create / destroy / bytes entries), VALUE
    (whether the kernel writes a value) and SEED (the default seed), and to ``__init__`` the arguments of
    create between the context and the handle.  ``load()`` and ``act()`` are its own."""

    ENTRIES = ("", "", "")
    VALUE = False
    SEED = 0x5E1EC7

    def __init__(self, env, create_args, num_actions: int, probs: bool = False, seed: Optional[int] = None):
        self.env, self._lib = env, _abi.lib()
        self.num_actions, self.seed = int(num_actions), int(self.SEED if seed is None else seed)
        dev, N = env.device, env.num_envs
        self.action = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.log_prob = torch.zeros(N, dtype=torch.float32, device=dev)
        self.value = torch.zeros(N, dtype=torch.float32, device=dev) if self.VALUE else None
        self.probs = torch.zeros(N, self.num_actions, dtype=torch.float32, device=dev) if probs else None
        self._out = _abi.BeActOut(self.action.data_ptr(), self.log_prob.data_ptr(),
                                  None if self.value is None else self.value.data_ptr(),
                                  None if self.probs is None else self.probs.data_ptr())
        h = C.c_void_p()
        _abi.check(getattr(self._lib, self.ENTRIES[0])(env._ctx, *create_args, C.byref(h)), env._ctx)
        self._h = h
        self._weights = None        # load() keeps its tensors here until the packing kernel has run

    def _seed(self, seed: Optional[int] = None) -> int:
        """The 64-bit seed argument of a C call: ``seed``, default the handle's own."""
        return (self.seed if seed is None else int(seed)) & (2**64 - 1)

    @property
    def packed_bytes(self) -> int:
        return int(getattr(self._lib, self.ENTRIES[2])(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.env.device)
            getattr(self._lib, self.ENTRIES[1])(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
