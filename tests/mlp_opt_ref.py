"""numpy restatement of be_mlp_opt (include/ballenv.h): the pinned SGD step (Adam's is
a2c_adam_ref.adam_step_ref, which takes any dict of tensors), mlp_pack_kernel's map from image index to
source element (csrc/mlp_policy.hip) and the inverse the update kernel scatters through.  Test
infrastructure only."""
import numpy as np

BLOCKS, KS1, HT, NO = 29, 8, 8, 16          # the input row, its 4-wide k steps, 128 / 16 hidden tiles, padded actions


def sgd_step_ref(w, g, state):
    """One step in place.  w, g: dicts of f32 arrays (g is read); state: f64 [t, b1^t, b2^t, lr]."""
    lr = np.float64(state[3])
    for k in w:
        assert w[k].dtype == g[k].dtype == np.float32
        prod = lr * g[k].astype(np.float64)
        w[k][...] = (w[k].astype(np.float64) - prod).astype(np.float32)
    state[0] = state[0] + 1.0


def names(layers):
    return [f"affine{i + 1}.{w}" for i in range(layers) for w in ("weight", "bias")]


def shapes(layers, h1, h2, A):
    s = [(h1, BLOCKS), (h1,)] + ([(h2, h1), (h2,), (A, h2), (A,)] if layers == 3 else [(A, h1), (A,)])
    return dict(zip(names(layers), s))


def layout(layers):
    """Offsets (in floats) of the image's parts, as mlp_layout(layers, 8, 8)."""
    ht2 = HT if layers == 3 else 0
    L = {"f1": 0}
    L["b1"] = L["f1"] + KS1 * HT * 64
    L["f2"] = L["b1"] + 16 * HT
    L["b2"] = L["f2"] + 4 * HT * ht2 * 64
    L["f3"] = L["b2"] + 16 * ht2
    L["b3"] = L["f3"] + 4 * HT * 64
    L["hb"] = L["b3"] + 16
    L["total"] = L["hb"] + 16
    return L


def pack_forward(layers, h1, h2, A):
    """mlp_pack_kernel's map, one image index at a time: a list of (tensor name, flat source index) for a
    weight, ("hb", m) for the 16 softmax biases, None for a pad entry."""
    L, nm = layout(layers), names(layers)
    ht2 = HT if layers == 3 else 0
    hl = h2 if layers == 3 else h1
    out = []
    for i in range(L["total"]):
        src = None
        if i < L["b1"]:
            lane, t = i & 63, i >> 6
            ht, kk = t % HT, t // HT
            m, k = 16 * ht + (lane & 15), 4 * kk + (lane >> 4)
            if m < h1 and k < BLOCKS:
                src = (nm[0], m * BLOCKS + k)
        elif i < L["f2"]:
            m = i - L["b1"]
            if m < h1:
                src = (nm[1], m)
        elif i < L["b2"]:
            j = i - L["f2"]
            lane, t = j & 63, j >> 6
            mt, s = t % ht2, t // ht2
            m, k = 16 * mt + (lane & 15), 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3)
            if m < h2 and k < h1:
                src = (nm[2], m * h1 + k)
        elif i < L["f3"]:
            m = i - L["b2"]
            if m < h2:
                src = (nm[3], m)
        elif i < L["b3"]:
            j = i - L["f3"]
            lane, s = j & 63, j >> 6
            m, k = lane & 15, 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3)
            if m < A and k < hl:
                src = (nm[-2], m * hl + k)
        elif i < L["hb"]:
            m = i - L["b3"]
            if m < A:
                src = (nm[-1], m)
        else:
            src = ("hb", i - L["hb"])
        out.append(src)
    return out


def image_index(layers, h1, h2, A):
    """The inverse, vectorised as the update kernel computes it: per tensor name the image index of
    every source element (int64 arrays of the tensor's flat size)."""
    L, nm = layout(layers), names(layers)
    ht2 = HT if layers == 3 else 0
    hl = h2 if layers == 3 else h1

    def frag(m, k):                         # f2 / f3: (s, lane) of weight (m, k)
        return ((k >> 4) << 2) | (k & 3), (((k >> 2) & 3) << 4) | (m & 15)

    out = {}
    j = np.arange(h1 * BLOCKS, dtype=np.int64)
    m, k = j // BLOCKS, j % BLOCKS
    out[nm[0]] = L["f1"] + (((k >> 2) * HT + (m >> 4)) << 6) + (((k & 3) << 4) | (m & 15))
    out[nm[1]] = L["b1"] + np.arange(h1, dtype=np.int64)
    if layers == 3:
        j = np.arange(h2 * h1, dtype=np.int64)
        m, k = j // h1, j % h1
        s, lane = frag(m, k)
        out[nm[2]] = L["f2"] + ((s * ht2 + (m >> 4)) << 6) + lane
        out[nm[3]] = L["b2"] + np.arange(h2, dtype=np.int64)
    j = np.arange(A * hl, dtype=np.int64)
    m, k = j // hl, j % hl
    s, lane = frag(m, k)
    out[nm[-2]] = L["f3"] + (s << 6) + lane
    out[nm[-1]] = L["b3"] + np.arange(A, dtype=np.int64)
    return out
