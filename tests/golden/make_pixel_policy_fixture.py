"""Convert the reference's trained pixel policy to two small .npz fixtures.

The reference stores the pixel agent's weights (examples/ball_cnn_reinforce.py:60-83 Policy: conv1..3 +
bn1..3 + head) as torch state_dicts under examples/stored_models/cnn_train_models/.  episode_900.pth is
the last of them that holds the conv net (episode_1000.pth and episode_2000.pth in that folder hold the
block MLP).  It is loaded here with torch.load(weights_only=True) (no unpickling of code) and its 20
float tensors -- the conv and head weights and biases, each BatchNorm's weight, bias, running_mean and
running_var -- are written as plain float32 arrays under their state_dict names, so tests on a machine
without the reference checkout can run be_cnn_act with the reference's own trained weights.
(num_batches_tracked is not a weight and is left out; gym_ballenv_amd.reference_pixel_weights() puts
zeros in its place.)

Two files, so that each stays smaller than the largest fixture so far: pixel_policy_cnn_conv3.npz holds
conv3.weight (about 100 KB), pixel_policy_cnn.npz the other 19 tensors.

    python tests/golden/make_pixel_policy_fixture.py <path of the reference checkout>
"""
import os
import sys

import numpy as np
import torch

SRC = os.path.join("examples", "stored_models", "cnn_train_models", "episode_900.pth")
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"conv1.weight": (16, 3, 5, 5), "conv2.weight": (32, 16, 5, 5), "conv3.weight": (32, 32, 5, 5),
          "head.weight": (9, 132), "head.bias": (9,)}
for _i, _c in ((1, 16), (2, 32), (3, 32)):
    for _k in (f"conv{_i}.bias", f"bn{_i}.weight", f"bn{_i}.bias", f"bn{_i}.running_mean", f"bn{_i}.running_var"):
        SHAPES[_k] = (_c,)


def main(ref):
    sd = torch.load(os.path.join(ref, SRC), weights_only=True, map_location="cpu")
    arrs = {k: sd[k].numpy().astype(np.float32) for k in SHAPES}
    assert {k: v.shape for k, v in arrs.items()} == SHAPES
    assert all(np.isfinite(v).all() for v in arrs.values())
    big = {"conv3.weight": arrs.pop("conv3.weight")}
    for name, part in (("pixel_policy_cnn.npz", arrs), ("pixel_policy_cnn_conv3.npz", big)):
        out = os.path.join(HERE, name)
        np.savez_compressed(out, **part)
        print(out, os.path.getsize(out), sorted(part))


if __name__ == "__main__":
    main(sys.argv[1])
