"""numpy side of be_cnn_adam's tests.  The Adam step is tests/a2c_adam_ref.py's adam_step_ref, which takes
any dict of tensors; here are the packed image's layout (csrc/cnn_host.h's constants, mirrored), the
inverse map of the fused re-pack written independently of the C++ (``image_index``, vectorised), a walk
of the pack kernel's forward rule (``pack_forward``), and the fixed rows of the overfit test with torch's
own training run on them.  Test infrastructure only."""
import numpy as np

PARAMS = ("conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "conv2.weight", "conv2.bias", "bn2.weight",
          "bn2.bias", "conv3.weight", "conv3.bias", "bn3.weight", "bn3.bias", "head.weight", "head.bias")
CONV_BIASES = ("conv1.bias", "conv2.bias", "conv3.bias")
CHANNELS = (16, 32, 32)

# offsets in floats (csrc/cnn_host.h)
F1 = 0                      # [19][64] conv1's fragments
FH = F1 + 19 * 64           # [33][64] the head's
P = (FH + 33 * 64, FH + 33 * 64 + 5 * 16, FH + 33 * 64 + 5 * 16 + 5 * 32)      # [5][C] per layer
HBIAS = P[2] + 5 * 32       # [16]
HB = HBIAS + 16             # [16] 0 / -inf
STAGED = HB + 16
F2 = STAGED                 # [100][2][64]
F3 = F2 + 100 * 2 * 64      # [200][2][64]
TOTAL = F3 + 200 * 2 * 64


def shapes(A):
    out = {}
    for i, (cin, c) in enumerate(((3, 16), (16, 32), (32, 32)), 1):
        out[f"conv{i}.weight"], out[f"conv{i}.bias"] = (c, cin, 5, 5), (c,)
        out[f"bn{i}.weight"], out[f"bn{i}.bias"] = (c,), (c,)
    out["head.weight"], out["head.bias"] = (A, 132), (A,)
    return {k: out[k] for k in PARAMS}


def image_index(A):
    """{parameter: int64 array of its shape}: the image index that holds each element."""
    idx = {}
    m, ci, ky, kx = np.indices((16, 3, 5, 5))
    j = 5 * ci + ky
    idx["conv1.weight"] = F1 + np.where(kx < 4, j, 15 + j // 4) * 64 + np.where(kx < 4, kx, j % 4) * 16 + m
    for name, base, cin in (("conv2.weight", F2, 16), ("conv3.weight", F3, 32)):
        m, ci, ky, kx = np.indices((32, cin, 5, 5))
        step = 25 * (ci // 4) + 5 * ky + kx
        idx[name] = base + (2 * step + m // 16) * 64 + (ci % 4) * 16 + m % 16
    m, k = np.indices((A, 132))
    idx["head.weight"] = FH + (k // 4) * 64 + (k % 4) * 16 + m
    idx["head.bias"] = HBIAS + np.arange(A)
    for layer, c in enumerate(CHANNELS):
        for row, name in enumerate(("conv%d.bias", "bn%d.weight", "bn%d.bias")):
            idx[name % (layer + 1)] = P[layer] + row * c + np.arange(c)
    return {k: idx[k].astype(np.int64) for k in PARAMS}


def running_index():
    """The image indices of the six running-statistics vectors (rows 3 and 4 of each layer's [5][C])."""
    return np.concatenate([P[layer] + 3 * c + np.arange(2 * c) for layer, c in enumerate(CHANNELS)])


def pack_forward(A):
    """cnn_pack_source's rule walked index by index: a list of TOTAL entries, (state_dict key, flat element),
    "zero" or "neginf"."""
    vec = ("conv%d.bias", "bn%d.weight", "bn%d.bias", "bn%d.running_mean", "bn%d.running_var")
    out = []
    for i in range(TOTAL):
        if i < FH:
            s, lane = divmod(i, 64)
            l4, m = divmod(lane, 16)
            if s < 15:
                ci, ky, kx = s // 5, s % 5, l4
            else:
                j = 4 * (s - 15) + l4
                if j >= 15:
                    out.append("zero")
                    continue
                ci, ky, kx = j // 5, j % 5, 4
            out.append(("conv1.weight", ((m * 3 + ci) * 5 + ky) * 5 + kx))
        elif i < P[0]:
            s, lane = divmod(i - FH, 64)
            l4, m = divmod(lane, 16)
            out.append(("head.weight", m * 132 + 4 * s + l4) if m < A else "zero")
        elif i < HBIAS:
            layer = 0 if i < P[1] else (1 if i < P[2] else 2)
            row, e = divmod(i - P[layer], CHANNELS[layer])
            out.append((vec[row] % (layer + 1), e))
        elif i < HB:
            out.append(("head.bias", i - HBIAS) if i - HBIAS < A else "zero")
        elif i < STAGED:
            m = i - HB
            out.append("zero" if (m < A or m == 15) else "neginf")
        else:
            third = i >= F3
            t, lane = divmod(i - (F3 if third else F2), 64)
            s, rt = divmod(t, 2)
            l4, m15 = divmod(lane, 16)
            m, ci, tap = 16 * rt + m15, 4 * (s // 25) + l4, s % 25
            out.append(("conv3.weight" if third else "conv2.weight", (m * (32 if third else 16) + ci) * 25 + tap))
    return out


OVERFIT_SEEDS = (0, 1, 2)


def overfit_rows():
    """The overfit test's 8 fixed rows: images and quadrants of pixel_policy_cases.given_images(8, 3) (two
    noise images, six fixture images), actions 0..7, every coef 1."""
    import torch
    from pixel_policy_cases import given_images
    img, quad = given_images(8, 3)
    return img, quad, torch.arange(8, dtype=torch.uint8)


def torch_overfit_losses(seed, steps=10, lr=1e-3):
    """torch's own run on those rows from random_policy(seed) in f32: per step the loss
    sum -Categorical(probs).log_prob(a) of torch_pixel_forward(..., "sample"), then torch.optim.Adam(lr).step()."""
    import torch
    import torch.nn.functional as F
    from gym_ballenv_amd.pixel_policy import torch_pixel_forward
    from pixel_policy_cases import random_policy
    img, quad, act = overfit_rows()
    pol = random_policy(seed).float()
    opt = torch.optim.Adam(pol.parameters(), lr=lr)
    x, q = img.float() / 255.0, F.one_hot(quad.long(), 4).float()
    out = []
    for _ in range(steps):
        probs = torch_pixel_forward(pol, x, q, "sample")
        loss = -torch.distributions.Categorical(probs=probs).log_prob(act.long()).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return out
