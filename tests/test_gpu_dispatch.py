"""Which kernel a context runs, pinned per entry point.

Contexts only: be_create, be_kernel_name for the five entries, be_pool_bytes, be_destroy -- no state
is allocated and nothing is launched beyond what be_create itself does.  The expected names were
recorded with this table against the library of the commit before the host ABI was split out of
csrc/ballenv.hip (tools/build_rev_lib.sh, BALLENV_LIB) and cross-checked against that commit's
pick_kernel / pick_rollout / be_create; the batch-size thresholds follow the device's CU count as
be_create computes them.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

ENTRIES = ("step", "step_sampled", "rollout", "reset", "observe")
ENV_VARS = ("BALLENV_POOL", "BALLENV_STEP_LPE", "BALLENV_STEP5_LPE", "BALLENV_ROLLOUT5_LPE", "BALLENV_GENERIC_KERNELS",
            "BALLENV_POOL_ONELANE_MAX", "BALLENV_POOL_PERIOD")

STEP2 = "step2_kernel<10, 13, 5, {}>"
ONE = "be_kernel<{}, 0, 13, 5, {}>"
STEPW = "stepw_kernel<5, 13, 5, {}, {}>"
ROLL = "rollout_kernel<{}, 13, 5, 0, 1, 10>"
ROLLW = "rolloutw_kernel<5, 13, 5, {}>"


def generic(wt, mode):
    """be_kernel's generic instance: wt = W for the staged windows (1..16, 21), 0 for run-time W"""
    return f"be_kernel<{wt}, {mode}, 0, 0, false>"


def case(id, W, n, step, rollout, pool, env=None, wt=None, **cfg):
    """n: envs, or a function of the CU count.  step_sampled / reset / observe always run the generic
    instance of the window (wt, W unless given)."""
    wt = W if wt is None else wt
    want = {"step": step, "step_sampled": generic(wt, 0), "rollout": rollout, "reset": generic(wt, 1),
            "observe": generic(wt, 2)}
    return pytest.param(W, n, env or {}, cfg, want, pool, id=id)


TWO_GOALS_EQUAL = [(12, 122), (12, 122), (87, 150), (430, 440), (230, 11)]
WIDE_ACTION = [(1, 1), (1, -1), (2, 0), (0, 1), (0, -1), (0, 0), (-1, 1), (-1, 0), (-1, -1)]

CASES = [
    # ---- W = 10
    case("w10-defaults", 10, 1000, STEP2.format("true"), ROLL.format(10), True),
    case("w10-pool-off", 10, 1000, STEP2.format("false"), ROLL.format(10), False, env={"BALLENV_POOL": "0"}),
    case("w10-no-autoreset", 10, 1000, STEP2.format("false"), ROLL.format(10), False, autoreset=False),
    case("w10-one-lane", 10, 1000, ONE.format(10, "true"), ROLL.format(10), True, env={"BALLENV_STEP_LPE": "1"}),
    case("w10-generic-only", 10, 1000, generic(10, 0), None, False, env={"BALLENV_GENERIC_KERNELS": "1"}),
    # two lanes per env up to 96 x 4 x CUs envs, one lane past it
    case("w10-two-lane-max", 10, lambda cus: 96 * 4 * cus, STEP2.format("true"), ROLL.format(10), True),
    case("w10-two-lane-max+1", 10, lambda cus: 96 * 4 * cus + 1, ONE.format(10, "true"), ROLL.format(10), True),
    # the one-lane kernel consumes the pool up to 2 x 64 x 4 x CUs envs
    case("w10-one-lane-pool-max", 10, lambda cus: 2 * 64 * 4 * cus, ONE.format(10, "true"), ROLL.format(10), True),
    case("w10-one-lane-pool-max+1", 10, lambda cus: 2 * 64 * 4 * cus + 1, ONE.format(10, "false"), ROLL.format(10), False),
    # ---- W = 5
    case("w5-4096", 5, 4096, STEPW.format(8, "true"), ROLLW.format(8), True),
    case("w5-lanes-max", 5, lambda cus: 64 * cus, STEPW.format(8, "true"), ROLLW.format(8), True),
    case("w5-lanes-max+1", 5, lambda cus: 64 * cus + 1, ONE.format(5, "true"), ROLL.format(5), True),
    case("w5-step-4-lanes", 5, 4096, STEPW.format(4, "true"), ROLLW.format(8), True, env={"BALLENV_STEP5_LPE": "4"}),
    case("w5-rollout-1-lane", 5, 4096, STEPW.format(8, "true"), ROLL.format(5), True, env={"BALLENV_ROLLOUT5_LPE": "1"}),
    # ---- every fixed-shape precondition falls back to the generic kernel (and the per-step rollout)
    case("generic-12-statics", 10, 1000, generic(10, 0), None, False, num_static=12),
    case("generic-speed-2", 10, 1000, generic(10, 0), None, False, speed_x=2),
    case("generic-wide-action", 10, 1000, generic(10, 0), None, False, actions=WIDE_ACTION),
    case("generic-equal-goals", 10, 1000, generic(10, 0), None, False, goals=TWO_GOALS_EQUAL),
    # R = 64 > HW_MAX.  (No radius makes the random-action rollout outgrow the LDS while the fixed
    # shape still holds: at R = 63 it needs 63 760 dynamic bytes of 160 KB and stays fused, the next
    # case; past 63 the rollout entry is None because the shape is no longer fixed.)
    # So be_kernel_name's "does not fit the LDS -> None" branch cannot be reached for the random-action
    # rollout and is not pinned here; only the policy rollout outgrows the LDS (tests/test_gpu_rollout.py).
    case("generic-radius-64", 10, 1000, generic(10, 0), None, False, radius_obstacle=59),
    case("w10-radius-63-fused", 10, 1000, ONE.format(10, "true"), ROLL.format(10), True, radius_obstacle=58),
    # R = 30 at W = 10: the 64-bit span table no longer fits (W-1+2R > 63), so the one-lane kernel
    case("w10-radius-30-one-lane", 10, 1000, ONE.format(10, "true"), ROLL.format(10), True, radius_obstacle=25),
    # ---- other windows: staged, run-time W, staged
    case("w7-staged", 7, 1000, generic(7, 0), None, False),
    case("w17-runtime", 17, 1000, generic(0, 0), None, False, wt=0),
    case("w21-staged", 21, 1000, generic(21, 0), None, False),
]


@pytest.mark.parametrize("W,n,env,cfg_kw,want,pool", CASES)
def test_dispatch(gpu, monkeypatch, W, n, env, cfg_kw, want, pool):
    from gym_ballenv_amd import _abi
    from gym_ballenv_amd.config import EnvConfig
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = _abi.lib()
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = n(cus) if callable(n) else n
    cfg = EnvConfig(**cfg_kw).to_abi(n, W)
    assert not _abi.config_check(cfg)
    ctx = C.c_void_p()
    _abi.check(lib.be_create(C.byref(cfg), torch.device(gpu).index or 0, C.byref(ctx)))
    try:
        got = {}
        for k, name in enumerate(ENTRIES):
            r = lib.be_kernel_name(ctx, k)
            got[name] = r.decode() if r else None
        got_pool = int(lib.be_pool_bytes(ctx))
    finally:
        lib.be_destroy(ctx)
    print(n, cus, got, got_pool)
    assert got == want, (n, cus)
    assert (got_pool > 0) == pool, (n, cus, got_pool)
