"""CPU: an audit of the pixel policy's GPU tests themselves.  For every entry of pixel_policy_cases.CASES --
the comparisons of be_cnn_act against torch with a random or calibrated policy -- it shows that the
compared outputs, the centred logits, depend on the whole packed image: on (nearly) every element of every
weight tensor and per-channel vector, by more than ten times the bound the GPU test allows.  A defect of
the size of a weight in any such element then fails the GPU test.  No GPU and no HIP runtime.

The measure.  In fp64, influence[e] = max over rows r and actions a of |w_e * dz[r, a] / dw_e|, one
autograd.grad per (row, action) on a batch of one image.  It is a FIRST-ORDER measure: it says what an
infinitesimal relative change of w_e does, and an element behind a relu that is off on every row has
influence 0 however large a change would switch it on.

Cases of one policy are audited together, on the union of their rows: the cases of N = 1 .. 17 cannot see
every weight on their own and are prefixes of the same policy's N = 67 case (given_images cycles one pool);
the action-count cases are the first A rows of one head on five images each (action_policy).  thr is ten
times the largest logit_bound among the cases taken together, and the caps are the same for every policy.
Not held to the caps (audited()): A = 1, whose one centred logit is 0 whatever the weights are, and random x3
weights in "running" mode, the blind spot the calibrated cases were added for.
"""
import pytest
import torch
import torch.nn.functional as F

from gym_ballenv_amd import _abi
from gym_ballenv_amd.pixel_policy import BN_EPS
from pixel_policy_cases import (CASES, case_inputs, centred_logits, given_images, logit_bound, random_policy, reference,
                                trained_policy)

WEIGHTS = ("conv1.weight", "conv2.weight", "conv3.weight", "head.weight")
CONV_BIASES = ("conv1.bias", "conv2.bias", "conv3.bias")
BN_AFFINE = tuple(f"bn{i}.{k}" for i in (1, 2, 3) for k in ("weight", "bias"))
BN_STATS = tuple(f"bn{i}.{k}" for i in (1, 2, 3) for k in ("running_mean", "running_var"))
MAX_SHARE = 0.02        # of a weight tensor's elements below thr
MAX_VECTOR = 1          # elements of a per-channel vector below thr


def leaves_of(pol):
    """The 20 packed tensors as fp64 leaves -- the BatchNorm buffers too."""
    sd = pol.state_dict()
    return {k: sd[k].detach().double().clone().requires_grad_() for k in _abi.CNN_TENSORS}


def centred_logits_of(w, x, quad, norm):
    """torch_pixel_forward up to the softmax, on a dict of tensors, so that the running statistics are
    differentiable too: (n, A) logits minus their row mean."""
    for i in (1, 2, 3):
        x = F.conv2d(x, w[f"conv{i}.weight"], w[f"conv{i}.bias"], stride=2)
        gamma, beta = w[f"bn{i}.weight"], w[f"bn{i}.bias"]
        if norm == "sample":
            x = F.instance_norm(x, weight=gamma, bias=beta, eps=BN_EPS)
        else:           # written out: F.batch_norm gives no gradient to its running statistics
            mean, var = w[f"bn{i}.running_mean"].view(1, -1, 1, 1), w[f"bn{i}.running_var"].view(1, -1, 1, 1)
            x = (x - mean) / torch.sqrt(var + BN_EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        x = F.relu(x)
    x = torch.cat((x.reshape(x.size(0), -1), torch.eye(4, dtype=x.dtype)[quad.long()]), 1)
    z = F.linear(x, w["head.weight"], w["head.bias"])
    return z - z.mean(-1, keepdim=True)


def influence(pol, img, quad, norm):
    """{tensor name: max over (row, action) of |w * dz / dw|}, the conv biases' largest per row (N,), and the
    centred logits (N, A)."""
    w = leaves_of(pol)
    names = [k for k in w if norm == "running" or k not in BN_STATS]
    leaves = [w[k] for k in names]
    infl = {k: torch.zeros_like(w[k]) for k in names}
    bias_rows = torch.zeros(img.shape[0], dtype=torch.float64)
    x = img.double() / 255.0
    zs = []
    for r in range(img.shape[0]):
        z = centred_logits_of(w, x[r:r + 1], quad[r:r + 1], norm)[0]
        zs.append(z.detach())
        for a in range(z.shape[0]):
            grads = torch.autograd.grad(z[a], leaves, retain_graph=a + 1 < z.shape[0])
            for k, g in zip(names, grads):
                one = (w[k].detach() * g).abs()
                infl[k] = torch.maximum(infl[k], one)
                if k in CONV_BIASES:
                    bias_rows[r] = max(bias_rows[r], one.max())
    return infl, bias_rows, torch.stack(zs)


def case_bound(pol, img, quad, norm, z_audit=None):
    """logit_bound of a case as the GPU test computes it: from torch fp32 and fp64 alone."""
    _, _, rpr, pr64 = reference(pol, img, quad, torch.zeros(img.shape[0]), norm)
    z64, mask = centred_logits(pr64)
    z32, _ = centred_logits(rpr.double(), mask)
    assert not mask.any()                                # a random or calibrated case has no entry below 1e-30
    if z_audit is not None:                              # the audit differentiates the function the test compares
        assert (z_audit - z64).abs().max().item() <= 1e-9
    return logit_bound(z64, z32)


def group_key(case):
    """Cases with the same key run the same weights in the same mode (the action-count cases: the first A
    rows of one head)."""
    if case.kind == "actions":
        return ("actions", case.seed, case.norm)
    if case.kind == "calibrated":
        return ("calibrated", case.N, case.A, case.seed, case.norm)
    return ("random", case.A, case.seed, case.norm)


def audited(case):
    """Not held to the caps: A = 1 (nothing to see) and random x3 weights in "running" mode, which stay in the
    GPU test as its large-logit cases (min p 1e-11) and whose blind spot is why the calibrated cases exist
    (test_why_the_calibrated_cases_exist)."""
    return not (case.kind == "random" and (case.A == 1 or case.norm == "running"))


GROUPS = {}
for _case in CASES:
    if audited(_case):
        GROUPS.setdefault(group_key(_case), []).append(_case)


def shares(infl, thr):
    return {k: (v < thr).sum().item() / v.numel() for k, v in infl.items()}


def fmt(sh):
    return "  ".join(f"{k} {100 * sh[k]:.2f}%" for k in WEIGHTS)


def test_which_cases_are_audited():
    assert len(CASES) == 28 + 6 + 15 and len(set(CASES)) == len(CASES)
    left_out = [c for c in CASES if not audited(c)]
    assert len(left_out) == 14 + 2 and all(c.kind == "random" for c in left_out)
    assert sum(len(g) for g in GROUPS.values()) + len(left_out) == len(CASES)
    assert len(GROUPS) == 4 + 6 + 1


@pytest.mark.parametrize("key", list(GROUPS), ids=lambda k: "-".join(str(x) for x in k))
def test_compared_outputs_depend_on_the_whole_packed_image(key):
    cases = sorted(GROUPS[key], key=lambda c: (-c.N, -c.A))
    norm = cases[0].norm
    bound, infl, rows = 0.0, None, 0
    for c in cases:
        pol, img, quad = case_inputs(c)
        if c.kind != "actions" and infl is not None:      # a prefix of the largest case: its rows are in the union already
            assert torch.equal(img, big[1][:c.N]) and torch.equal(quad, big[2][:c.N])
            assert all(torch.equal(a, b) for a, b in zip(pol.state_dict().values(), big[0].state_dict().values()))
            bound = max(bound, case_bound(pol, img, quad, norm))
            continue
        if c.A == 1:                                      # of the action counts: z = 0, no influence to add
            continue
        big = (pol, img, quad)
        part, bias_rows, z = influence(pol, img, quad, norm)
        bound = max(bound, case_bound(pol, img, quad, norm, z))
        rows += img.shape[0]
        if norm == "sample":
            # the conv biases are subtracted with the mean: nobody may count on this mode to test them.  On a
            # constant image every map is constant, each 1 / sqrt(0 + eps) multiplies fp64's own rounding by 316
            # and dz / d(conv output) is that much larger per layer: there the zero is shown to 1e-12 * eps**-1.5
            # (measured: 3.4e-9 on such rows, at most 2.5e-14 on all others)
            const = (img == img[:, :, :1, :1]).all(-1).all(-1).all(-1)
            for flag, cap in ((~const, 1e-12), (const, 1e-12 * BN_EPS ** -1.5)):
                if flag.any():
                    assert bias_rows[flag].max().item() < cap, (c, bias_rows)
        if infl is None:
            infl = part
        else:                                             # action counts: the head's first A rows
            for k, v in part.items():
                sl = tuple(slice(0, n) for n in v.shape)
                infl[k][sl] = torch.maximum(infl[k][sl], v)
    thr = 10.0 * bound
    sh = shares(infl, thr)
    below = {k: int((v < thr).sum()) for k, v in infl.items()}
    print(f"{key}: rows {rows}  logit_bound {bound:.3g}  thr {thr:.3g}  {fmt(sh)}  "
          + "  ".join(f"{k} {below[k]}" for k in infl if k not in WEIGHTS + (() if norm == "running" else CONV_BIASES) and below[k]))
    for k in WEIGHTS:
        assert sh[k] <= MAX_SHARE, (k, sh[k])
    for k in BN_AFFINE + (CONV_BIASES + BN_STATS if norm == "running" else ()) + ("head.bias",):
        assert below[k] <= MAX_VECTOR, (k, below[k])


def test_why_the_calibrated_cases_exist():
    """Documentation, not a gate on the cases: random x3 weights in "running" mode leave more than a tenth of
    conv3.weight without influence on any compared output of given_images(67, 0) -- half its input channels
    are dead behind running means of +-0.3 on positive inputs -- and the trained weights leave more."""
    img, quad = given_images(67, 0)
    pol = random_policy(0, 9)
    infl = influence(pol, img, quad, "running")[0]
    thr = 10.0 * case_bound(pol, img, quad, "running")
    sh = shares(infl, thr)
    print(f"random x3, running: thr {thr:.3g}  {fmt(sh)}")
    assert sh["conv3.weight"] > 0.10
    pol = trained_policy()
    _, _, rpr, pr64 = reference(pol, img, quad, torch.zeros(67), "sample")
    z64, mask = centred_logits(pr64)
    thr = 10.0 * logit_bound(z64, centred_logits(rpr.double(), mask)[0])
    infl = influence(pol, img, quad, "sample")[0]
    print(f"trained, sample: thr {thr:.3g}  masked {int(mask.sum())}  rows with p > 0.999: {int((pr64.max(1).values > 0.999).sum())}  "
          f"{fmt(shares(infl, thr))}")
