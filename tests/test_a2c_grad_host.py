"""be_a2c_grad on the host side: the numpy restatement of its pinned formulas (tests/a2c_grad_ref.py)
equals torch f64 autograd of a2c_losses, the library declares and exports both entries, and a NULL
ctx is refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import torch

from a2c_grad_ref import (PARAMS, SHAPE_CASES, TILE_EDGE_CASES, a2c_grad_ref, case_inputs, case_policy, kink_rows,
                          make_inputs, multi_tile_cases, torch_reference, weights64)
from gym_ballenv_amd import _abi
from gym_ballenv_amd.policy import Policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_f64_autograd():
    """W = 5, rows = 300: gradients and losses to 1e-12 relative (of each tensor's largest element).
    Pins the smooth-L1 branches and the undifferentiated v in the advantage."""
    torch.manual_seed(0)
    pol = Policy(5)
    obs, actions, rn, valid = make_inputs(np.random.default_rng(5), 300, 5)
    ref = a2c_grad_ref(weights64(pol), obs, actions, rn, valid)
    grads, (pl, vl) = torch_reference(pol, obs, actions, rn, valid, torch.float64)
    d = np.abs(rn.astype(np.float64))
    assert (d > 2).any() and (d < 0.5).any()
    for k in PARAMS:
        want = grads[k]
        err = np.abs(ref["grads"][k].reshape(want.shape) - want).max() / np.abs(want).max()
        assert err <= 1e-12, (k, err)
    assert abs(ref["losses"][0] - pl) <= 1e-12 * ref["abs_terms"][0]
    assert abs(ref["losses"][1] - vl) <= 1e-12 * ref["abs_terms"][1]
    assert ref["losses"][2] == int((valid != 0).sum())
    # with v differentiated in the advantage the value head's gradient would differ: the test can tell
    assert np.abs(grads["value_head.bias"]).max() > 0


def test_inactive_rows_and_kink_mask():
    """valid = 0 and out-of-range actions drop a row; the kink mask of the GPU test is sparse."""
    torch.manual_seed(0)
    pol = Policy(5)
    w = weights64(pol)
    obs, actions, rn, valid = make_inputs(np.random.default_rng(6), 300, 5)
    a = a2c_grad_ref(w, obs, actions, rn, valid)
    actions2, valid2 = actions.copy(), valid.copy()
    rows = np.flatnonzero(valid)[:3]
    actions2[rows[0]], actions2[rows[1]] = 9, 255
    valid2[rows[:2]] = 0
    b = a2c_grad_ref(w, obs, actions2, rn, valid)
    c = a2c_grad_ref(w, obs, actions, rn, valid2)
    assert b["losses"] == c["losses"] and b["losses"][2] == a["losses"][2] - 2
    for k in PARAMS:
        assert np.array_equal(b["grads"][k], c["grads"][k])
    assert kink_rows(w, obs).mean() <= 0.01


def test_fixture_weights_kink_share():
    """The committed Policy(10) fixture with the GPU test's observations: at most 1 % of the rows lie
    on a relu kink (the GPU test excludes them)."""
    from gym_ballenv_amd.policy import reference_weights
    path = reference_weights(10)
    assert path, "tests/golden/policy_w10.npz is missing"
    pol = Policy.from_npz(path, 10)
    obs = make_inputs(np.random.default_rng(1000 + 11951), 11951, 10)[0]
    share = kink_rows(weights64(pol), obs).mean()
    print(f"kink share, fixture weights: {share:.4%}")
    assert share <= 0.01


def test_new_cases_kink_share():
    """Every multi-tile (at 256 workgroups: an MI355X), shape and tile-edge case of the GPU test: at
    most 1 % of its rows lie on a relu kink (the GPU test clears their valid under the same cap) and
    at least half of the rows stay valid."""
    cases = [c + (False,) for c in SHAPE_CASES + TILE_EDGE_CASES] + list(multi_tile_cases(256).values())
    assert len(cases) == 23 and all(rows > 64 * 256 for _, _, _, rows, _ in multi_tile_cases(256).values())
    for W, hidden, A, rows, fixture in cases:
        pol = case_policy(W, hidden, A, fixture)
        obs, actions, rn, valid, kink = case_inputs(pol, W, rows, A)
        left = int((np.where(kink, 0, valid) != 0).sum())
        print(f"W={W} hidden={hidden} A={A} rows={rows} fixture={fixture}: {kink.sum()} kink rows, {left} valid")
        assert kink.sum() <= 0.01 * rows, (W, hidden, A, rows, fixture, int(kink.sum()))
        assert left >= 0.5 * rows and (actions < A).all(), (W, hidden, A, rows, fixture, left)


def test_library_declares_and_exports_be_a2c_grad():
    txt = open(os.path.join(ROOT, "include", "ballenv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+be_a2c_grad\s*\(", txt), "be_a2c_grad is not declared in include/ballenv.h"
    assert re.search(r"\bint64_t\s+be_a2c_grad_workspace_bytes\s*\(", txt)
    assert re.search(r"\}\s*be_a2c_weights\s*;", txt) and re.search(r"\}\s*be_a2c_grads\s*;", txt)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT be_a2c_grad\b", out), "be_a2c_grad not exported"
    assert re.search(r"\bT be_a2c_grad_workspace_bytes\b", out), "be_a2c_grad_workspace_bytes not exported"
    L = _abi.lib()
    assert len(L.be_a2c_grad.argtypes) == 11 and len(L.be_a2c_grad_workspace_bytes.argtypes) == 3
    assert "be_a2c_grad" not in _abi.EXPORTS and "be_a2c_grad_workspace_bytes" not in _abi.EXPORTS
    assert L.be_abi_version() == _abi.ABI_VERSION == 7        # additive: no ABI bump


def test_null_ctx_is_invalid():
    """The first check of both entries, before anything touches a device."""
    L = _abi.lib()
    w = _abi.BeA2CWeights(8, 8, 8, 8, 8, 8, 128, 9)
    g = _abi.BeA2CGrads(8, 8, 8, 8, 8, 8, 8)
    assert L.be_a2c_grad(None, 8, 8, 8, 8, 1, C.byref(w), 8, 1 << 30, C.byref(g), None) == _abi.BE_E_INVALID
    assert b"ctx" in L.be_last_error(None)
    assert L.be_a2c_grad_workspace_bytes(None, 128, 9) == _abi.BE_E_INVALID
