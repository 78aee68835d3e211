"""The arithmetic include/ballenv.h pins for be_mlp_grad, restated in numpy f64, and the torch autograd
references of tests/test_mlp_grad_host.py and tests/test_gpu_mlp_grad.py (not a test module).

REINFORCE follows Categorical(probs).log_prob (examples/ball_env_reinforce.py:88-108): the probability
of the action clamped to fp32's [eps, 1 - eps] before the log, no gradient outside the clamp; XENT
follows CrossEntropyLoss on the logits (examples/train_supervise.py:74, :97)."""
import numpy as np
import torch

EPS = float(np.finfo(np.float32).eps)
REINFORCE, XENT = "reinforce", "xent"


def param_names(layers):
    return [f"affine{i + 1}.{w}" for i in range(layers) for w in ("weight", "bias")]


def weights64(pol):
    return [p.detach().cpu().double().numpy() for lin in pol.linears() for p in (lin.weight, lin.bias)]


def mlp_grad_ref(w, blocks, actions, coef, valid, loss, final_relu, scale=1.0):
    """w: [W1, b1, W2, b2(, W3, b3)] f64.  Returns dict(grads={name: f64}, losses=[scale * sum, count],
    abs_terms=sum of |row loss|, pa=p_a of every row (its action taken mod A), active, clamped)."""
    layers = len(w) // 2
    x = np.asarray(blocks, dtype=np.float64)
    rows = x.shape[0]
    A = w[-1].shape[0]
    c = np.ones(rows) if coef is None else np.asarray(coef, dtype=np.float64)
    v = np.ones(rows, bool) if valid is None else np.asarray(valid).astype(bool)
    act = np.asarray(actions).astype(np.int64)
    active = v & (act < A)
    a = np.where(act < A, act, 0)
    pre1 = x @ w[0].T + w[1]
    h1 = np.maximum(pre1, 0)
    if layers == 3:
        pre2 = h1 @ w[2].T + w[3]
        h2 = np.maximum(pre2, 0)
    h = h2 if layers == 3 else h1
    zp = h @ w[-2].T + w[-1]
    z = np.maximum(zp, 0) if final_relu else zp
    m = z.max(1)
    e = np.exp(z - m[:, None])
    S = e.sum(1)
    p = e / S[:, None]
    idx = np.arange(rows)
    pa = p[idx, a]
    onehot = np.zeros_like(p)
    onehot[idx, a] = 1.0
    if loss == REINFORCE:
        rl = -c * np.log(np.clip(pa, EPS, 1 - EPS))
        inb = (pa >= EPS) & (pa <= 1 - EPS)
        dz = c[:, None] * (p - onehot) * inb[:, None]
    else:
        inb = np.ones(rows, bool)
        rl = -c * (z[idx, a] - m - np.log(S))
        dz = c[:, None] * (p - onehot)
    rl = np.where(active, rl, 0.0)
    dz = dz * active[:, None]
    dzp = np.where(zp <= 0, 0.0, dz) if final_relu else dz
    g = {}
    names = param_names(layers)
    g[names[-2]] = dzp.T @ h
    g[names[-1]] = dzp.sum(0)
    dh = dzp @ w[-2]
    if layers == 3:
        dpre2 = np.where(pre2 > 0, dh, 0.0)
        g["affine2.weight"] = dpre2.T @ h1
        g["affine2.bias"] = dpre2.sum(0)
        dh = dpre2 @ w[2]
    dpre1 = np.where(pre1 > 0, dh, 0.0)
    g["affine1.weight"] = dpre1.T @ x
    g["affine1.bias"] = dpre1.sum(0)
    g = {k: g[k] * scale for k in names}
    return dict(grads=g, losses=np.array([rl.sum() * scale, float(active.sum())]),
                abs_terms=float(np.abs(rl).sum() * abs(scale)), pa=pa, probs=p, active=active, clamped=active & ~inb)


def torch_reference(pol, blocks, actions, coef, valid, loss, dtype, scale=1.0, device="cpu"):
    """torch autograd in `dtype` on `device`: ({name: numpy f64 of .grad}, loss).  REINFORCE is
    reinforce_losses' expression on given coefficients (fp32: Categorical(probs).log_prob; f64: its fp32
    clamp restated, as tests/test_block_policy_host.py does), XENT supervised_losses' with a weight per row
    and a sum times scale for the mean.  Rows with valid = 0 or an action >= A are left out."""
    import copy
    import torch.nn.functional as F
    p = copy.deepcopy(pol).to(device=device, dtype=dtype)
    p.zero_grad()
    A = p.num_actions
    act = torch.as_tensor(np.asarray(actions).astype(np.int64), device=device)
    keep = act < A
    if valid is not None:
        keep = keep & torch.as_tensor(np.asarray(valid).astype(bool), device=device)
    c = torch.ones(act.shape[0]) if coef is None else torch.as_tensor(np.asarray(coef, dtype=np.float32))
    c = c.to(device)
    x = torch.as_tensor(np.asarray(blocks), device=device).to(dtype)
    a = torch.where(keep, act, torch.zeros_like(act))
    if loss == REINFORCE:
        probs = p(x)
        if dtype == torch.float32:
            logp = torch.distributions.Categorical(probs=probs).log_prob(a)
        else:
            logp = torch.log((probs / probs.sum(-1, keepdim=True)).clamp(EPS, 1 - EPS)).gather(-1, a[:, None])[:, 0]
        total = -(logp.double() * c.double())[keep].sum() * scale
    else:
        ce = F.cross_entropy(p.logits(x), a, reduction="none")
        total = (ce * c.to(dtype))[keep].sum() * scale
    if keep.any():
        total.backward()
    grads = {k: (torch.zeros_like(q) if q.grad is None else q.grad).detach().cpu().double().numpy()
             for k, q in p.named_parameters()}
    return grads, float(total.detach())


def sample_actions(probs, rng):
    """One action per row drawn from the row's own probabilities (f64), as u8."""
    u = rng.random(probs.shape[0])
    a = (probs.cumsum(1) <= u[:, None]).sum(1)
    return np.minimum(a, probs.shape[1] - 1).astype(np.uint8)


def clamp_band(pa):
    """Rows whose p_a lies where fp32 and f64 may fall on different sides of Categorical's clamp:
    [eps / 2, 2 eps] or [1 - 2 eps, 1 - eps / 2]."""
    return ((pa >= EPS / 2) & (pa <= 2 * EPS)) | ((pa >= 1 - 2 * EPS) & (pa <= 1 - EPS / 2))
