"""numpy reference of be_observe_pixels (extract_patch of examples/ball_cnn_reinforce.py:120-163):

* ``patch_ref``   the frame of ``gym_ballenv_amd.render.draw``, padded with white, cut around the agent;
* ``coeffs_ref``  PIL's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for bicubic 100 -> 40, in doubles;
* ``resize_ref``  PIL's two-pass 8-bit resample in integers (horizontal into u8, then vertical);
* ``to_f32``      ToTensor's ``v / 255`` in f32.
"""
from __future__ import annotations

import numpy as np

from gym_ballenv_amd import render

PATCH, OUT, SPAN, BITS = 100, 40, 50, 22


def patch_ref(cfg, agent, goal, statics, dynamics) -> np.ndarray:
    """(100, 100, 3) u8, top row first: cell (i, j) is world pixel (ax - 50 + j, ay + 49 - i)."""
    screen = render.draw(cfg, agent, goal, statics, dynamics)
    ax, ay = int(agent[0]) + SPAN, screen.shape[0] - int(agent[1]) + SPAN          # :133-135
    padded = np.pad(screen, ((SPAN, SPAN), (SPAN, SPAN), (0, 0)), constant_values=255)   # :136
    return np.ascontiguousarray(padded[ay - SPAN:ay + SPAN, ax - SPAN:ax + SPAN])  # :146


def patches_of(env_cfg, state) -> np.ndarray:
    """patch_ref of every env of a SoA numpy state (BatchedBallEnv.state_dict layout)."""
    n = state["agent"].shape[0]
    ns, nd = env_cfg.num_static, env_cfg.num_dynamic
    return np.stack([patch_ref(env_cfg, state["agent"][i].tolist(), state["goal"][i].tolist(),
                               state["static_obs"][:ns, i].tolist(), state["dyn_obs"][:nd, i].tolist())
                     for i in range(n)])


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs_ref(in_size: int = PATCH, out_size: int = OUT):
    """(kk (out, 10) i32 zero-padded, bounds (out, 2) i32 = first input index, tap count)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    kk = np.zeros((out_size, 10), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)           # int(): C's truncation
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            kk[xx, x] = int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


_COEFFS = None


def _pass(a: np.ndarray, kk, bounds) -> np.ndarray:
    """One resample pass along axis 0 of a (100, ...) u8 array -> (40, ...) u8."""
    out = np.empty((kk.shape[0],) + a.shape[1:], np.uint8)
    src = a.astype(np.int64)
    for xx in range(kk.shape[0]):
        x0, n = bounds[xx]
        acc = np.tensordot(kk[xx, :n].astype(np.int64), src[x0:x0 + n], axes=(0, 0)) + (1 << (BITS - 1))
        assert np.abs(acc).max() < 2 ** 31               # PIL accumulates in int
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return out


def resize_ref(patch: np.ndarray) -> np.ndarray:
    """(..., 100, 100, 3) u8 -> (..., 3, 40, 40) u8: Image.fromarray(patch).resize((40, 40), BICUBIC)."""
    global _COEFFS
    if _COEFFS is None:
        _COEFFS = coeffs_ref()
    kk, bounds = _COEFFS
    p = np.asarray(patch, np.uint8)
    lead = p.shape[:-3]
    p = p.reshape((-1,) + p.shape[-3:])
    h = _pass(np.moveaxis(p, 2, 0), kk, bounds)          # x first: (40 xx, B, 100 y, 3)
    v = _pass(np.moveaxis(h, 2, 0), kk, bounds)          # (40 yy, 40 xx, B, 3)
    return np.ascontiguousarray(v.transpose(2, 3, 0, 1)).reshape(lead + (3, OUT, OUT))


def to_f32(img: np.ndarray) -> np.ndarray:
    return img.astype(np.float32) / np.float32(255)
