"""The loss-log ring's read-back (optim.unrolled_log) on plain CPU tensors: no GPU test wraps the A2C log."""
import pytest
import torch

ROWS = 4


@pytest.mark.parametrize("width", [2, 3])
@pytest.mark.parametrize("t", [0, 3, 4, 5, 8, 11])
def test_unrolled_log_is_the_last_rows_in_step_order(t, width):
    from gym_ballenv_amd.optim import unrolled_log
    # the ring as the device leaves it: step s writes (s, 10 s [, 100 s]) into row s % ROWS
    log = torch.full((ROWS, width), -1.0, dtype=torch.float64)
    for s in range(t):
        log[s % ROWS] = torch.tensor([float(s), 10.0 * s, 100.0 * s][:width], dtype=torch.float64)
    before = log.clone()
    out = unrolled_log(log, t)
    steps = list(range(max(0, t - ROWS), t))
    assert out.dtype == torch.float64 and tuple(out.shape) == (min(t, ROWS), width)
    assert out[:, 0].tolist() == [float(s) for s in steps]
    assert out[:, 1].tolist() == [10.0 * s for s in steps]
    if width == 3:
        assert out[:, 2].tolist() == [100.0 * s for s in steps]
    assert torch.equal(log, before)          # a pure function of (log, t)
