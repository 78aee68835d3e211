"""A cold import of the package's optimisers and trainers in a fresh interpreter: no import cycle through
the shared optim module, the lazy __getattr__ still works, and both optimisers derive from the one base."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cold_import_of_optimisers_and_trainers():
    code = (
        "import sys; sys.path.insert(0, sys.argv[1])\n"
        "import gym_ballenv_amd as gb\n"
        "assert 'gym_ballenv_amd.optim' not in sys.modules          # the torch-dependent parts load lazily\n"
        "names = ('HipBlockOptim', 'HipAdam', 'SupervisedTrainer', 'BlockTrainer', 'A2CTrainer')\n"
        "got = {n: getattr(gb, n) for n in names}\n"
        "from gym_ballenv_amd.optim import HipOptim\n"
        "assert issubclass(gb.HipAdam, HipOptim) and issubclass(gb.HipBlockOptim, HipOptim)\n"
        "assert gb.HipAdam.__mro__[1] is HipOptim and gb.HipBlockOptim.__mro__[1] is HipOptim\n"
        "assert gb.HipAdam.step is gb.HipBlockOptim.step is HipOptim.step\n"
        "assert gb.HipAdam.LOSS_WIDTH == 3 and gb.HipBlockOptim.LOSS_WIDTH == 2\n"
        "assert all(isinstance(c, type) and c.__name__ == n for n, c in got.items())\n"
        "assert all(n in gb.__all__ for n in names)\n"
        "print('cold import: OK')\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "cold import: OK" in r.stdout, r.stdout + r.stderr
    # the other order: the block module first, then the module it builds on
    code2 = ("import sys; sys.path.insert(0, sys.argv[1])\n"
             "import gym_ballenv_amd.block_policy as bp, gym_ballenv_amd.rollout as ro, gym_ballenv_amd.optim as op\n"
             "assert bp.HipOptim is ro.HipOptim is op.HipOptim\n"
             "print('cold import: OK')\n")
    r = subprocess.run([sys.executable, "-c", code2, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "cold import: OK" in r.stdout, r.stdout + r.stderr
