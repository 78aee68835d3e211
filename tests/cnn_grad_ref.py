"""The references of be_cnn_grad's tests (tests/test_pixel_grad_host.py, tests/test_gpu_pixel_grad.py).

``restatement``: the formulas include/ballenv.h pins for be_cnn_grad, written out in float64 -- unfold /
matrix products for the convolutions, the BatchNorm backward and the clamp of Categorical by hand, fold for
the transposed convolution; no autograd.  ``torch_reference``: the same loss through autograd on
``torch_pixel_forward(norm="sample")`` and ``Categorical.log_prob``, in a chosen dtype on a chosen device.
Both return ``Ref``: the 14 gradients keyed like ``state_dict``, the loss, the sum of the absolute row
terms (the loss comparison's scale), the number of active rows and the probabilities.

``inputs`` builds the shared inputs of the tolerance tests and ``check_rule`` applies the project's rule
err_hip <= 4 * err_torch32 + 1e-6 per tensor, both errors max-abs distances from the restatement over its
max-abs."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from pixel_policy_cases import given_images

EPS = float(np.finfo(np.float32).eps)
BN_EPS = 1e-5
PARAMS = tuple(f"{m}.{w}" for i in (1, 2, 3) for m in (f"conv{i}", f"bn{i}") for w in ("weight", "bias")) + \
    ("head.weight", "head.bias")
CONV_BIASES = ("conv1.bias", "conv2.bias", "conv3.bias")
Ref = namedtuple("Ref", "grads loss abs_loss count probs")


def _active(actions, valid, A):
    act = actions.long()
    ok = act < A
    if valid is not None:
        ok = ok & (valid != 0)
    return act.clamp(max=A - 1), ok


def restatement(pol, images, quadrants, actions, coef=None, valid=None, scale=1.0):
    """be_cnn_grad's contract in float64 on the CPU, no autograd.  images (rows, 3, 40, 40) u8, quadrants /
    actions (rows,) u8, coef f32 or None, valid u8 / bool or None."""
    sd = {k: v.detach().double().cpu() for k, v in pol.state_dict().items()}
    A = sd["head.weight"].shape[0]
    n = images.shape[0]
    x = images.double().cpu() / 255.0
    act, ok = _active(actions.cpu(), None if valid is None else valid.cpu(), A)
    c = torch.ones(n, dtype=torch.float64) if coef is None else coef.double().cpu()
    saved = []
    for i in (1, 2, 3):
        W, b = sd[f"conv{i}.weight"], sd[f"conv{i}.bias"]
        gamma, beta = sd[f"bn{i}.weight"], sd[f"bn{i}.bias"]
        co = W.shape[0]
        side = (x.shape[-1] - 5) // 2 + 1
        cols = F.unfold(x, 5, stride=2)                                  # (n, ci * 25, L)
        conv = torch.matmul(W.reshape(co, -1), cols) + b[None, :, None]   # (n, co, L)
        mean = conv.mean(-1, keepdim=True)
        var = ((conv - mean) ** 2).mean(-1, keepdim=True)
        inv = 1.0 / torch.sqrt(var + BN_EPS)
        xhat = (conv - mean) * inv
        pre = xhat * gamma[None, :, None] + beta[None, :, None]
        saved.append((cols, xhat, inv, pre, tuple(x.shape[1:])))
        x = pre.clamp(min=0).reshape(n, co, side, side)
    feat = torch.cat((x.reshape(n, -1), torch.eye(4, dtype=torch.float64)[quadrants.long().cpu()]), 1)
    z = feat @ sd["head.weight"].T + sd["head.bias"]
    p = torch.softmax(z, 1)
    pa = p.gather(1, act[:, None]).squeeze(1)
    terms = torch.where(ok, -c * torch.log(pa.clamp(EPS, 1.0 - EPS)), torch.zeros_like(pa))
    inside = ok & (pa >= EPS) & (pa <= 1.0 - EPS)
    dz = torch.where(inside[:, None], c[:, None] * (p - F.one_hot(act, A).double()), torch.zeros_like(p))
    g = {"head.weight": dz.T @ feat, "head.bias": dz.sum(0)}
    dy = (dz @ sd["head.weight"][:, :128]).reshape(n, 32, 4)
    for i in (3, 2, 1):
        cols, xhat, inv, pre, in_shape = saved[i - 1]
        gamma = sd[f"bn{i}.weight"]
        L = xhat.shape[-1]
        dyr = torch.where(pre > 0, dy, torch.zeros_like(dy))
        s1, s2 = dyr.sum(-1, keepdim=True), (dyr * xhat).sum(-1, keepdim=True)
        g[f"bn{i}.bias"], g[f"bn{i}.weight"] = s1.sum(0).squeeze(-1), s2.sum(0).squeeze(-1)
        dconv = gamma[None, :, None] * inv * (dyr - s1 / L - xhat * s2 / L)
        W = sd[f"conv{i}.weight"]
        g[f"conv{i}.weight"] = torch.einsum("nol,nkl->ok", dconv, cols).reshape(W.shape)
        g[f"conv{i}.bias"] = torch.zeros(W.shape[0], dtype=torch.float64)     # the mean subtracts the bias
        if i > 1:
            din = F.fold(torch.matmul(W.reshape(W.shape[0], -1).T, dconv), in_shape[1:], 5, stride=2)
            dy = din.reshape(n, in_shape[0], -1)
    g = {k: v * scale for k, v in g.items()}
    return Ref(g, float(terms.sum()) * scale, float(terms.abs().sum()) * abs(scale), int(ok.sum()), p)


def torch_reference(pol, images, quadrants, actions, coef=None, valid=None, dtype=torch.float64, device="cpu",
                    scale=1.0):
    """The same loss through autograd: torch_pixel_forward(norm="sample") + Categorical.log_prob in `dtype` on
    `device`; the gradients as float64 on the CPU."""
    import copy
    from gym_ballenv_amd.pixel_policy import torch_pixel_forward
    m = copy.deepcopy(pol).to(device=device, dtype=dtype)
    A = m.head.out_features
    act, ok = _active(actions.cpu(), None if valid is None else valid.cpu(), A)
    act, ok = act.to(device), ok.to(device)
    n = images.shape[0]
    c = torch.ones(n, dtype=dtype, device=device) if coef is None else coef.to(device=device, dtype=dtype)
    x = images.to(device=device, dtype=dtype) / 255.0
    q = F.one_hot(quadrants.long(), 4).to(device=device, dtype=dtype)
    probs = torch_pixel_forward(m, x, q, "sample")
    logp = torch.distributions.Categorical(probs=probs).log_prob(act)
    terms = -(logp * c)[ok]
    loss = terms.sum() * scale
    m.zero_grad()
    loss.backward()
    g = {k: v.grad.detach().double().cpu() for k, v in m.named_parameters()}
    return Ref(g, float(loss.detach().double()), float(terms.detach().double().abs().sum()) * abs(scale), int(ok.sum()),
               probs.detach().double().cpu())


def drop_constant(images, quadrants):
    """given_images' rows without the images whose bytes are all equal."""
    flat = images.reshape(images.shape[0], -1)
    keep = (flat != flat[:, :1]).any(1)
    return images[keep].contiguous(), quadrants[keep].contiguous()


def inputs(pol, rows, seed, constant=False):
    """The tolerance tests' shared inputs for a policy: `rows` images of given_images(., seed) without (or,
    with `constant`, with) the constant ones, actions drawn from the policy's own float64 probabilities, coef
    standard normal, valid 90 % of the rows with row 0 always valid; rows whose float64 p_a lies in one of
    Categorical's clamp bands get valid = 0 (at most max(4, rows // 1000) of them: asserted).
    Returns (images, quadrants, actions u8, coef f32, valid u8) on the CPU."""
    from gym_ballenv_amd.pixel_policy import torch_pixel_forward
    if constant:
        img, quad = given_images(rows, seed)
    else:
        img, quad = drop_constant(*given_images(rows + 2 * (rows // 28 + 2), seed))
        assert img.shape[0] >= rows
        img, quad = img[:rows].contiguous(), quad[:rows].contiguous()
    g = torch.Generator().manual_seed(1000 + seed)
    import copy
    with torch.no_grad():
        p = torch_pixel_forward(copy.deepcopy(pol).double(), img.double() / 255.0,
                                torch.eye(4, dtype=torch.float64)[quad.long()], "sample")
    act = torch.multinomial(p.clamp(min=0), 1, generator=g).squeeze(1)
    coef = torch.randn(rows, generator=g, dtype=torch.float32)
    valid = (torch.rand(rows, generator=g) < 0.9).to(torch.uint8)
    valid[0] = 1
    pa = p.gather(1, act[:, None]).squeeze(1)
    band = (pa < 2 * EPS) | (pa > 1.0 - 2 * EPS)
    assert int(band.sum()) <= max(4, rows // 1000), int(band.sum())
    valid[band] = 0
    return img, quad, act.to(torch.uint8), coef, valid


def errors(got, ref64):
    """Per tensor max|got - ref| / max|ref| (0 / 0 = 0), over the tensors of ref64 other than the conv biases."""
    out = {}
    for k in PARAMS:
        if k in CONV_BIASES:
            continue
        r = ref64[k].double().cpu()
        d = (got[k].double().cpu() - r).abs().max().item()
        m = r.abs().max().item()
        out[k] = d / m if m > 0 else d
    return out


def check_rule(hip, t32, r64, keys=None, show=None):
    """err_hip <= 4 * err_torch32 + 1e-6 for every tensor of `keys` (default: all but the conv biases) and
    for the loss over the sum of absolute row terms.  hip: (grads dict, loss); t32, r64: Ref."""
    eh, et = errors(hip[0], r64.grads), errors(t32.grads, r64.grads)
    scale = r64.abs_loss if r64.abs_loss > 0 else 1.0
    eh["loss"], et["loss"] = abs(hip[1] - r64.loss) / scale, abs(t32.loss - r64.loss) / scale
    bad = []
    for k in (keys or list(eh)):
        if show is not None:
            show(f"{k}: hip {eh[k]:.3e} torch32 {et[k]:.3e}")
        if not eh[k] <= 4.0 * et[k] + 1e-6:
            bad.append((k, eh[k], et[k]))
    assert not bad, bad
