"""Convert the reference's supervised training data to a small .npz fixture.

examples/train_supervise.py fits the block-count MLP (Model, :11-28) to one recorded human trial:
* examples/State_info_trail_no2  a pickled list of 3 186 prep_state2 rows (29 block counts each), read by
                                 prepare_train_X (:32-38)
* examples/Trial_no_2            the pickled actions of the same steps, (dx, dy) in tens of pixels;
                                 prepare_train_Y (:42-59) divides by 10 and looks the tuple up in the
                                 move list, the label being its index 0..8

Both are Python 2 pickles of numpy arrays: loaded with encoding="latin1", checked (integer counts
0..3, every action in the move list) and written as two u8 arrays, so the tests and
supervised_update can run train_supervise.py's loop on the reference's own data without the
reference checkout.

    python tests/golden/make_supervise_fixture.py <reference checkout>
"""
import os
import pickle
import sys

import numpy as np

MOVES = [(1, 1), (1, -1), (1, 0), (0, 1), (0, -1), (0, 0), (-1, 1), (-1, 0), (-1, -1)]     # train_supervise.py:43
HISTOGRAM = [299, 199, 637, 336, 286, 688, 153, 397, 191]
HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    ex = os.path.join(ref, "examples")
    with open(os.path.join(ex, "State_info_trail_no2"), "rb") as fp:
        xs = pickle.load(fp, encoding="latin1")
    with open(os.path.join(ex, "Trial_no_2"), "rb") as fp:
        ys = pickle.load(fp, encoding="latin1")
    x = np.stack([np.asarray(r, dtype=np.float64).reshape(-1) for r in xs])
    assert x.shape == (3186, 29) and len(ys) == 3186, (x.shape, len(ys))
    assert (x == np.round(x)).all() and x.min() >= 0 and x.max() <= 3, (x.min(), x.max())
    labels = []
    for a in ys:
        a = np.asarray(a)
        tup = (int(a[0]) // 10, int(a[1]) // 10)
        assert (tup[0] * 10, tup[1] * 10) == (int(a[0]), int(a[1])), a
        labels.append(MOVES.index(tup))
    labels = np.asarray(labels, dtype=np.uint8)
    hist = np.bincount(labels, minlength=9).tolist()
    assert hist == HISTOGRAM, hist
    out = os.path.join(HERE, "supervise_trial2.npz")
    np.savez_compressed(out, blocks=x.astype(np.uint8), labels=labels,
                        source="examples/State_info_trail_no2 + examples/Trial_no_2")
    print(out, x.shape, labels.shape, hist, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
