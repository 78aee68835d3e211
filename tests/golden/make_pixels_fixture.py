"""Writes tests/golden/pixels.npz: 16 crafted env states (default config: 13 static + 5 dynamic
obstacles), PIL's own 40 x 40 bicubic images of their 100 x 100 patches, and the resize's coefficient
rows.  Needs Pillow; the tests that read the fixture do not.

    python tests/golden/make_pixels_fixture.py
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pixels_ref  # noqa: E402
from gym_ballenv_amd.config import EnvConfig  # noqa: E402

NS, ND, E = 13, 5, 16


def states():
    rng = np.random.default_rng(20240521)
    agent = rng.integers(60, 440, (E, 2))
    goal = rng.integers(0, 500, (E, 2))
    # obstacles scattered around the agent so that most patches show a few
    static = agent[:, None, :] + rng.integers(-160, 161, (E, NS, 2))
    dyn = agent[:, None, :] + rng.integers(-120, 121, (E, ND, 2))
    agent[0], agent[1], agent[2], agent[3] = (0, 0), (500, 500), (0, 500), (500, 0)      # the four corners
    agent[4] = (250, 0)                                                                  # an edge midpoint
    for e in range(5):                 # something to see in the visible quarter / half
        sx, sy = (1 if agent[e][0] < 250 else -1), (1 if agent[e][1] < 250 else -1)
        static[e, 0] = agent[e] + (sx * 30, sy * 25)
        dyn[e, 0] = agent[e] + (sx * 8, sy * 44)
        goal[e] = agent[e] + (sx * 20, sy * 6)
    static[5, 3] = agent[5]                                # an obstacle over the agent
    static[6, 2] = agent[6] + (22, -17)                    # a dynamic obstacle over a static one
    dyn[6, 1] = static[6, 2] + (8, 5)
    goal[7] = agent[7] + (3, -4)                           # the goal within 10 px of the agent
    goal[8] = agent[8] + (-2, 9)
    agent[9] = (30, 28)                                    # disks cut by the screen's edge inside the patch
    static[9, 0], static[9, 1], dyn[9, 0] = (5, 40), (44, -3), (-12, 10)
    goal[9] = (3, 2)
    for e, d in ((10, 69), (11, 70), (12, 71)):            # the patch's edge: |dx|, |dy| = 69, 70, 71 (radius 20)
        static[e] = agent[e] + rng.integers(200, 300, (NS, 2))      # the rest out of sight
        dyn[e] = agent[e] - rng.integers(200, 300, (ND, 2))
        static[e, 0], static[e, 1] = agent[e] + (d, 0), agent[e] + (-d, 0)
        dyn[e, 0], dyn[e, 1] = agent[e] + (3, d), agent[e] + (-3, -d)
        static[e, 2], dyn[e, 2] = agent[e] + (d - 15, d - 15), agent[e] + (15 - d, 15 - d)
    return agent, goal, static, dyn


def main():
    cfg = EnvConfig()
    agent, goal, static, dyn = states()
    patches = np.stack([pixels_ref.patch_ref(cfg, agent[e].tolist(), goal[e].tolist(), static[e].tolist(), dyn[e].tolist())
                        for e in range(E)])
    images = np.stack([np.asarray(Image.fromarray(p, "RGB").resize((40, 40), Image.BICUBIC)).transpose(2, 0, 1)
                       for p in patches])
    kk, bounds = pixels_ref.coeffs_ref()
    assert np.array_equal(pixels_ref.resize_ref(patches), images), "the integer restatement disagrees with PIL"
    out = os.path.join(HERE, "pixels.npz")
    np.savez_compressed(out, agent=agent.astype(np.int16), goal=goal.astype(np.int16), static=static.astype(np.int16),
                        dyn=dyn.astype(np.int16), images=np.ascontiguousarray(images, np.uint8), kk=kk, bounds=bounds)
    colours = [len(np.unique(p.reshape(-1, 3), axis=0)) for p in patches]
    print(out, os.path.getsize(out), "bytes; colours per patch", colours)


if __name__ == "__main__":
    main()
