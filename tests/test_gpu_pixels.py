"""be_observe_pixels on the GPU: the pixel agent's observation (extract_patch of
examples/ball_cnn_reinforce.py:120-163) byte for byte against PIL's images of the fixture's states and
against the numpy reference (tests/pixels_ref.py: render.draw + pad + crop, PIL's integer resize) on
Philox rollouts -- every subset of the three outputs, out= tensors, obstacle counts 0 .. 30, other radii
and a non-square screen, an env index past 2^31 bytes of patch, graph capture, the caller's stream, and
the reference's training loop on PixelPolicy."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import helpers
import pixels_ref
from test_gpu_parity import KEYS, load_np_state, make_env, np_state

pytestmark = pytest.mark.gpu


def soa_state(agent, goal, static, dyn):
    """SoA numpy state from (E, 2), (E, 2), (E, Ns, 2), (E, Nd, 2) coordinates."""
    E = agent.shape[0]
    so = np.ascontiguousarray(static.transpose(1, 0, 2).astype(np.int16)) if static.shape[1] else np.zeros((1, E, 2), np.int16)
    do = np.ascontiguousarray(dyn.transpose(1, 0, 2).astype(np.int16)) if dyn.shape[1] else np.zeros((1, E, 2), np.int16)
    return dict(agent=agent.astype(np.int16), goal=goal.astype(np.int16), prev_dist=np.zeros(E), total_dist=np.ones(E),
                ep_return=np.zeros(E), ep_len=np.zeros(E, np.int32), episode=np.ones(E, np.uint32), static_obs=so,
                dyn_obs=do, dyn_goal=np.zeros((max(dyn.shape[1], 1), E), np.uint8))


def reference(env, index=None):
    """(patch, image) of the env's current state from the numpy reference (of the envs in index)."""
    st = np_state(env)
    if index is not None:
        st = {k: (v[index] if k in ("agent", "goal") else v[:, index]) for k, v in st.items() if k in
              ("agent", "goal", "static_obs", "dyn_obs")}
    patch = pixels_ref.patches_of(env.cfg, st)
    return patch, pixels_ref.resize_ref(patch)


def check_all(env, msg=""):
    patch, img = reference(env)
    got_img, got_patch = env.observe_pixels(patch=True)
    got_f32 = env.observe_pixels(f32=True)
    np.testing.assert_array_equal(got_patch.cpu().numpy(), patch, err_msg=msg + " patch")
    np.testing.assert_array_equal(got_img.cpu().numpy(), img, err_msg=msg + " u8")
    np.testing.assert_array_equal(got_f32.cpu().numpy(), pixels_ref.to_f32(img), err_msg=msg + " f32")
    return patch


@pytest.fixture(scope="module")
def fixture_env(gpu):
    from gym_ballenv_amd.config import EnvConfig
    fx = helpers.load("pixels")
    env = make_env(EnvConfig(), fx["agent"].shape[0], 10, gpu)
    load_np_state(env, soa_state(fx["agent"], fx["goal"], fx["static"], fx["dyn"]))
    yield env, fx
    env.close()


def test_fixture_states_equal_pil(fixture_env):
    env, fx = fixture_env
    assert env.status() == 0
    before = env.state_dict()
    img, patch = env.observe_pixels(patch=True)
    f32 = env.observe_pixels(f32=True)
    assert img.shape == (16, 3, 40, 40) and img.dtype == torch.uint8 and patch.shape == (16, 100, 100, 3)
    assert f32.shape == (16, 3, 40, 40) and f32.dtype == torch.float32
    np.testing.assert_array_equal(img.cpu().numpy(), fx["images"])
    np.testing.assert_array_equal(f32.cpu().numpy(), pixels_ref.to_f32(fx["images"]))
    ref_patch = pixels_ref.patches_of(env.cfg, np_state(env))
    np.testing.assert_array_equal(patch.cpu().numpy(), ref_patch)
    # no state change, no status bit
    for k in KEYS:
        assert torch.equal(getattr(env, k), before[k]), k
    assert env.status() == 0


def test_every_subset_of_the_outputs_gives_the_same_bytes(fixture_env, gpu):
    from gym_ballenv_amd import _abi
    env, _ = fixture_env
    N = env.num_envs
    full_img, full_patch = env.observe_pixels(patch=True)
    full_f32 = env.observe_pixels(f32=True)
    cs = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    for want in itertools.product((False, True), repeat=3):
        patch = torch.full((N, 100, 100, 3), 7, dtype=torch.uint8, device=gpu) if want[0] else None
        img = torch.full((N, 3, 40, 40), 7, dtype=torch.uint8, device=gpu) if want[1] else None
        f32 = torch.full((N, 3, 40, 40), -1.0, device=gpu) if want[2] else None
        rc = env._lib.be_observe_pixels(env._ctx, C.byref(env._st), *(None if t is None else t.data_ptr() for t in (patch, img, f32)), cs)
        if not any(want):
            assert rc == _abi.BE_E_INVALID and b"needs patch, out or out_f32" in env._lib.be_last_error(env._ctx)
            continue
        assert rc == _abi.BE_OK, want
        for got, full in ((patch, full_patch), (img, full_img), (f32, full_f32)):
            if got is not None:
                assert torch.equal(got, full), want
    # a misaligned pointer is rejected, not written through
    img = torch.zeros(N * 4800 + 16, dtype=torch.uint8, device=gpu)
    assert env._lib.be_observe_pixels(env._ctx, C.byref(env._st), None, img.data_ptr() + 4, None, cs) == _abi.BE_E_INVALID
    assert b"16-byte" in env._lib.be_last_error(env._ctx)
    torch.cuda.synchronize(gpu)
    assert int(img.sum()) == 0


def test_out_tensors_are_written_in_place(fixture_env, gpu):
    env, fx = fixture_env
    N = env.num_envs
    img = torch.full((N, 3, 40, 40), 9, dtype=torch.uint8, device=gpu)
    patch = torch.full((N, 100, 100, 3), 9, dtype=torch.uint8, device=gpu)
    f32 = torch.full((N, 3, 40, 40), 9.0, device=gpu)
    ptrs = [t.data_ptr() for t in (img, patch, f32)]
    r_img, r_patch = env.observe_pixels(patch=True, out=(img, patch))
    r_f32 = env.observe_pixels(f32=True, out=f32)
    assert r_img is img and r_patch is patch and r_f32 is f32
    assert [t.data_ptr() for t in (img, patch, f32)] == ptrs
    np.testing.assert_array_equal(img.cpu().numpy(), fx["images"])
    np.testing.assert_array_equal(f32.cpu().numpy(), pixels_ref.to_f32(fx["images"]))
    assert torch.equal(patch, env.observe_pixels(patch=True)[1])
    with pytest.raises(ValueError):
        env.observe_pixels(out=f32)                      # f32 tensor for the u8 image
    with pytest.raises(ValueError):
        env.observe_pixels(out=img[:8])


@pytest.mark.parametrize("N,ns,nd", [(301, 13, 5), (67, 0, 0), (67, 2, 1), (67, 30, 5), (1, 13, 5)])
def test_philox_rollout_with_autoreset(gpu, N, ns, nd):
    """N is no multiple of the envs a workgroup takes at a time (8, one per wave); compared at two of 40 steps."""
    from gym_ballenv_amd.config import EnvConfig
    cfg = EnvConfig(num_static=ns, num_dynamic=nd, obstacle_speed=[1 + (k % 3) for k in range(nd)], time_limit=30,
                    autoreset=True)
    env = make_env(cfg, N, 10, gpu, seed=1234 + N + ns)
    env.reset()
    acts = env.sample_actions(40, seed=5)
    n_done, shown = 0, 0
    for t in range(40):
        _, _, done, _ = env.step(acts[t])
        n_done += int(done.sum())
        if t in (16, 39):
            patch = check_all(env, f"t={t}")
            shown += int((patch != 255).any(axis=(1, 2, 3)).sum())
    assert n_done >= N                                   # every env passed its TimeLimit and was reset
    assert shown > 0
    assert env.status() == 0
    env.close()


def test_other_radii_and_a_non_square_screen(gpu):
    """radius_obstacle 7 and 33, radius_agent 9, a 300 x 420 screen (a width / height swap shows at the
    right and top edges), agents on every edge and corner."""
    from gym_ballenv_amd.config import EnvConfig
    rng = np.random.default_rng(11)
    for ro, (sw, sh) in ((7, (300, 420)), (33, (300, 420)), (33, (420, 300))):
        cfg = EnvConfig(screen_width=sw, screen_height=sh, radius_obstacle=ro, radius_agent=9, strip_goal_x=sw,
                        strip_agent_x=sw, num_static=6, num_dynamic=3, obstacle_speed=[1, 1, 1], autoreset=False, time_limit=0)
        E = 23
        agent = np.stack([rng.integers(0, sw + 1, E), rng.integers(0, sh + 1, E)], 1)
        agent[:8] = [(0, 0), (sw, sh), (0, sh), (sw, 0), (sw - 1, sh // 2), (sw // 2, sh - 1), (sw - 30, sh - 45), (sw - 49, 50)]
        goal = agent + rng.integers(-40, 41, (E, 2))
        static = agent[:, None, :] + rng.integers(-90, 91, (E, 6, 2))
        dyn = agent[:, None, :] + rng.integers(-70, 71, (E, 3, 2))
        static[:, 0] = agent + (50 + ro - 1, 0)              # the patch's edge for this radius: in by one row of pixels
        static[:, 1] = agent + (0, -(50 + ro))               # and just out
        env = make_env(cfg, E, 10, gpu)
        load_np_state(env, soa_state(agent, goal, static, dyn))
        check_all(env, f"ro={ro} {sw}x{sh}")
        assert env.status() == 0
        env.close()


def test_many_envs_a_wave_and_patch_offsets_past_2_31(gpu):
    """71 600 envs: every wave takes several envs, and the last envs' patches start past 2^31 bytes."""
    from gym_ballenv_amd.config import EnvConfig
    N = 71600
    assert (N - 1) * 30000 > 2 ** 31
    env = make_env(EnvConfig(time_limit=30), N, 10, gpu, seed=99)
    env.reset()
    acts = env.sample_actions(12, seed=3)
    for t in range(12):
        env.step(acts[t])
    index = np.array([0, 1, 2047, 2048, 2049, 4095, 4096, 30000, 65535, 65536, 71582, 71583, 71584, N - 2, N - 1])
    patch, img = reference(env, index)
    got_img, got_patch = env.observe_pixels(patch=True)
    got_f32 = env.observe_pixels(f32=True)
    idx = torch.from_numpy(index).to(gpu)
    np.testing.assert_array_equal(got_patch[idx].cpu().numpy(), patch)
    np.testing.assert_array_equal(got_img[idx].cpu().numpy(), img)
    np.testing.assert_array_equal(got_f32[idx].cpu().numpy(), pixels_ref.to_f32(img))
    # the envs in between: a patch holds only 0 and 255, and the three calls agree
    assert bool(((got_patch == 0) | (got_patch == 255)).all())
    assert torch.equal(got_img, env.observe_pixels())
    table = torch.from_numpy(pixels_ref.to_f32(np.arange(256, dtype=np.uint8))).to(gpu)
    assert torch.equal(got_f32, table[got_img.to(torch.int32)])
    env.close()


def test_graph_capture_with_out_and_replay_after_a_step(gpu):
    from gym_ballenv_amd.config import EnvConfig
    N = 301
    env = make_env(EnvConfig(time_limit=30), N, 10, gpu, seed=21)
    env.reset()
    img = torch.zeros((N, 3, 40, 40), dtype=torch.uint8, device=gpu)
    f32 = torch.zeros((N, 3, 40, 40), device=gpu)
    env.observe_pixels(out=img)                           # the first call outside the capture
    torch.cuda.synchronize(gpu)
    side = torch.cuda.Stream(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        env.observe_pixels(out=img)
        env.observe_pixels(f32=True, out=f32)
    g.replay()
    torch.cuda.synchronize(gpu)
    first = env.observe_pixels()
    assert torch.equal(img, first)
    acts = env.sample_actions(9, seed=2)
    for t in range(9):
        env.step(acts[t])
    g.replay()
    torch.cuda.synchronize(gpu)
    now = env.observe_pixels()
    assert torch.equal(img, now) and not torch.equal(now, first)
    assert torch.equal(f32, env.observe_pixels(f32=True))
    np.testing.assert_array_equal(img.cpu().numpy(), reference(env)[1])
    env.close()


def test_runs_on_the_callers_stream(gpu):
    """The launch is ordered behind the work the caller queued on its current stream: the state is
    loaded on a side stream behind a spin, and the observation on that stream must show it."""
    from gym_ballenv_amd.config import EnvConfig
    N = 67
    env, other = (make_env(EnvConfig(time_limit=30), N, 10, gpu, seed=s) for s in (5, 6))
    env.reset()
    other.reset()
    want = other.observe_pixels().clone()
    assert not torch.equal(want, env.observe_pixels())
    new = other.state_dict()
    torch.cuda.synchronize(gpu)
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)
        env.load_state_dict(new)
        got = env.observe_pixels()
    side.synchronize()
    assert torch.equal(got, want)
    env.close()
    other.close()


def test_the_references_loop_on_pixel_policy(gpu):
    """Three iterations of INTEGRATION.md's ball_cnn_reinforce.py loop: pixels + quadrant -> PixelPolicy ->
    Categorical -> env.step."""
    from gym_ballenv_amd import PixelPolicy, pixel_inputs
    from gym_ballenv_amd.config import EnvConfig
    N = 67
    env = make_env(EnvConfig(time_limit=30), N, 10, gpu, seed=8)
    env.reset()
    torch.manual_seed(0)
    policy = PixelPolicy().to(gpu)
    log_probs = []
    for _ in range(3):
        image, quadrant = pixel_inputs(env)
        assert image.shape == (N, 3, 40, 40) and image.dtype == torch.float32 and quadrant.shape == (N, 4)
        assert torch.equal(quadrant.sum(1), torch.ones(N, device=gpu))
        probs = policy(image, quadrant)
        assert probs.shape == (N, 9) and bool(torch.isfinite(probs).all())
        m = torch.distributions.Categorical(probs)
        action = m.sample()
        log_probs.append(m.log_prob(action))
        _, reward, done, _ = env.step(action)
    loss = -(torch.stack(log_probs) * 1.0).sum()
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in policy.parameters())
    assert env.status() == 0
    env.close()
