"""Convert the reference's trained block-count policies to small .npz fixtures.

The reference stores the REINFORCE / supervised agents' weights (examples/ball_env_reinforce.py:57-73
Policy, examples/train_supervise.py:11-28 Model: affine1 (29 -> 128) -> relu -> [affine2 (128 -> 128)
-> relu ->] last layer (-> 9) on the prep_state2 block counts) as torch state_dicts under
examples/stored_models/.  They are loaded here with torch.load(weights_only=True) (no unpickling
of code) and written as plain float32 arrays, so tests on the GPU box (which has no
/root/reference) can run be_mlp_act with the reference's own trained weights.

Two families:
* supervised3   supervised/episode_38999.pth: 3 layers, trained by train_supervise.py, whose forward
                returns affine3's scores with no relu (:22-28)  ->  final_relu = 0
* reinforce2    without_obs_rand/rand_obs1/episode_15000.pth: 2 layers (affine2 is 9 x 128), a
                REINFORCE agent of ball_env_reinforce.py, whose forward applies relu to every
                layer, the last included (:68-70)               ->  final_relu = 1

    python tests/golden/make_block_policy_fixture.py
"""
import os

import numpy as np
import torch

REF = "/root/reference/examples/stored_models"
SRC = {"supervised3": (os.path.join(REF, "supervised", "episode_38999.pth"), 3, 0),
       "reinforce2": (os.path.join(REF, "without_obs_rand", "rand_obs1", "episode_15000.pth"), 2, 1)}
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    for kind, (path, layers, final_relu) in SRC.items():
        sd = torch.load(path, weights_only=True, map_location="cpu")
        arrs = {k.replace(".", "_"): v.numpy().astype(np.float32) for k, v in sd.items()}
        assert len(arrs) == 2 * layers and arrs["affine1_weight"].shape == (128, 29), {k: v.shape for k, v in arrs.items()}
        assert arrs[f"affine{layers}_weight"].shape == (9, 128)
        out = os.path.join(HERE, f"block_policy_{kind}.npz")
        np.savez_compressed(out, source=os.path.relpath(path, "/root/reference"), layers=np.int32(layers),
                            final_relu=np.int32(final_relu), **arrs)
        print(out, {k: v.shape for k, v in arrs.items()})


if __name__ == "__main__":
    main()
