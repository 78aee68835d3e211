"""The pixel policy's test cases, shared by tests/test_gpu_pixel_policy.py (be_cnn_act against torch) and
tests/test_pixel_policy_coverage_host.py (which of the packed weights those comparisons can see): the
policies, the images, the torch fp32 / fp64 reference, and the comparison in logit space.

Why logit space.  A softmax row with one probability near 1 hides every other logit behind the common
factor 1 / sum: at |probs - torch| <= 2e-5 most single-weight defects of conv2, conv3 and the head are
invisible on the trained weights and on random weights in "running" mode.  z_a = log p_a - mean_a log p_a
recovers the logits up to a constant from the probabilities the kernel already writes; 1 / sum cancels in
the centring, so a saturated row is compared as sharply as a flat one.

Why calibrated running statistics.  random_policy() draws running_mean in +-0.3 for layers whose inputs
are post-relu, hence positive: about half the channels of conv2 and conv3 are then dead on every image
and their weights have no influence on any output.  calibrated_policy() sets each layer's running
statistics to the pooled statistics of its conv output over the test's own images -- the state of a real
eval-mode net -- which brings "running" mode to the coverage of "sample" mode; and "running" is the only
mode in which the conv biases matter at all ("sample" subtracts them with the mean).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import helpers


def trained_policy():
    from gym_ballenv_amd.pixel_policy import PixelPolicy, reference_pixel_weights
    pol = PixelPolicy()
    pol.load_state_dict(reference_pixel_weights(), strict=True)
    return pol


def random_policy(seed, A=9):
    """conv and head parameters x3, gamma in [0.5, 1.5], beta in +-0.5, running mean in +-0.3, var in [0.2, 2]."""
    from gym_ballenv_amd.pixel_policy import PixelPolicy
    torch.manual_seed(seed)
    pol = PixelPolicy(A)
    with torch.no_grad():
        for m in (pol.conv1, pol.conv2, pol.conv3, pol.head):
            m.weight.mul_(3.0)
            m.bias.mul_(3.0)
        for bn in (pol.bn1, pol.bn2, pol.bn3):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.3, 0.3)
            bn.running_var.uniform_(0.2, 2.0)
    return pol


def given_images(N, seed):
    """(N, 3, 40, 40) u8 and (N,) u8 quadrants: all-white, all-black, white with one black pixel, noise, the
    16 fixture images, more noise -- cycled from an offset of `seed`, so N = 1 takes another one per seed."""
    g = torch.Generator().manual_seed(100 + seed)
    white = torch.full((3, 40, 40), 255, dtype=torch.uint8)
    dot = white.clone()
    dot[:, 17, 22] = 0
    pool = [white, torch.zeros(3, 40, 40, dtype=torch.uint8), dot]
    pool += [torch.randint(0, 256, (3, 40, 40), generator=g, dtype=torch.uint8) for _ in range(2)]
    pool += list(torch.from_numpy(helpers.load("pixels")["images"]))
    pool += [torch.randint(0, 256, (3, 40, 40), generator=g, dtype=torch.uint8) for _ in range(9)]
    img = torch.stack([pool[(i + seed) % len(pool)] for i in range(N)])
    return img.contiguous(), (torch.arange(N) % 4).to(torch.uint8)


def reference(pol, img, quad, u, norm):
    """(action, log_prob, probs) of torch fp32 and the fp64 probs, on the CPU."""
    from gym_ballenv_amd.pixel_policy import torch_pixel_forward, torch_pixel_select_action
    with torch.no_grad():
        ra, rlp, rpr = torch_pixel_select_action(pol.float(), img, quad, u, norm)
        pr64 = torch_pixel_forward(pol.double(), img.double() / 255.0, torch.eye(4, dtype=torch.float64)[quad.long()], norm)
        pol.float()
    return ra, rlp, rpr, pr64


def calibrated_policy(seed, A, images_u8):
    """random_policy(seed, A) with every BatchNorm's running_mean / running_var set to the per-channel mean
    and biased variance of that layer's conv output over (N, H, W) of images_u8 / 255, layer by layer in
    fp64: each layer's output goes through its BatchNorm (with the statistics just stored) and relu before
    the next layer is measured -- the eval-mode forward of the net being calibrated."""
    pol = random_policy(seed, A)
    x = images_u8.double() / 255.0
    with torch.no_grad():
        for conv, bn in ((pol.conv1, pol.bn1), (pol.conv2, pol.bn2), (pol.conv3, pol.bn3)):
            y = F.conv2d(x, conv.weight.double(), conv.bias.double(), stride=2)
            bn.running_mean.copy_(y.mean((0, 2, 3)))
            bn.running_var.copy_(y.var((0, 2, 3), unbiased=False))
            x = F.relu(F.batch_norm(y, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(),
                                    bn.bias.double(), False, 0.0, bn.eps))
    return pol


P_FLOOR = 1e-30     # an fp64 probability below this is not compared: its f32 value nears the denormals


def centred_logits(probs64, mask=None):
    """(z, mask) of (N, A) fp64 probabilities: z = log p - mean_a log p per row, the logits up to a
    constant.  mask marks the entries that are left out, by default those with p < 1e-30; they count
    neither in the comparison nor in their row's mean, which runs over the remaining entries, and their z
    is 0.  Give the fp64 reference's mask to centre another set of probabilities (torch fp32's, the
    kernel's, as doubles) over the same entries."""
    if mask is None:
        mask = probs64 < P_FLOOR
    keep = ~mask
    lp = torch.where(keep, torch.log(torch.where(keep, probs64, torch.ones_like(probs64))), torch.zeros_like(probs64))
    mean = lp.sum(-1, keepdim=True) / keep.sum(-1, keepdim=True).clamp(min=1)
    return torch.where(keep, lp - mean, torch.zeros_like(lp)), mask


def logit_bound(z64, z32):
    """The largest |z_hip - z64| a correct kernel may show, from the two references alone.

    4 * max|z32 - z64|: the project's rule for every kernel -- four times torch fp32's own error against
    fp64 on the same inputs.
    8 * 2**-23 * (1 + max|z64|): derived, not measured -- what the kernel's softmax (policy_core.h's
    policy_dist) adds on exact logits.  p = v_exp_f32((z - max) * log2(e)) * rcp(sum), and |z - max| is up
    to 2 max|z| for centred z.  The f32 subtraction, the f32 constant log2(e) and the f32 product are each
    rounded to 2**-24 relative, so the exponent is off by up to 3 * 2 max|z| * log2(e) * 2**-24, which is
    3 max|z| * 2**-23 relative in p and so absolute in log p; v_exp_f32 is accurate to 1 ulp, 2**-23; the
    product with rcp(sum) and p's rounding are 2**-24 each; rcp(sum)'s own error is common to a row and
    cancels in the centring.  Per entry (3 max|z| + 2) * 2**-23, at most twice that once the row's mean
    of such errors is subtracted: (6 max|z| + 4) * 2**-23, under the 8 (max|z| + 1) * 2**-23 asked."""
    return 4.0 * (z32 - z64).abs().max().item() + 8.0 * 2.0 ** -23 * (1.0 + z64.abs().max().item())


def action_policy(seed, A):
    """random_policy(seed, 15) seen through its first A actions: the same convolutions and BatchNorms for every
    A, the head's first A rows.  The fifteen action counts are then one policy, each head row is run by every
    case with more actions than its index, and the coverage audit can take the fifteen cases together."""
    from gym_ballenv_amd.pixel_policy import PixelPolicy
    full = random_policy(seed, 15)
    pol = PixelPolicy(A)
    sd = full.state_dict()
    sd["head.weight"], sd["head.bias"] = sd["head.weight"][:A].clone(), sd["head.bias"][:A].clone()
    pol.load_state_dict(sd, strict=True)
    return pol


# Every comparison of be_cnn_act against torch with a random or calibrated policy, one entry per test case
# of tests/test_gpu_pixel_policy.py.  kind "random": random_policy(seed, A) on given_images(N, seed);
# "calibrated": calibrated_policy(seed, A, those images) on them; "actions": action_policy(seed, A) on
# given_images(N, action_images(A)) -- every action count, so every number of -inf pad rows of the head,
# each on five images of its own (A = 15, whose last head row no other case runs, on five noise images).
Case = namedtuple("Case", "kind norm N A seed")

RANDOM_SHAPES = [(1, 9), (15, 15), (16, 1), (16, 9), (17, 9), (67, 15), (67, 9)]
CALIBRATED_SHAPES = [(67, 9), (67, 15), (17, 9)]
ACTION_COUNTS = list(range(1, 16))
ACTION_N, ACTION_SEED = 5, 2

CASES = [Case("random", norm, N, A, seed) for N, A in RANDOM_SHAPES for seed in (0, 1) for norm in ("sample", "running")]
CASES += [Case("calibrated", "running", N, A, seed) for N, A in CALIBRATED_SHAPES for seed in (0, 1)]
CASES += [Case("actions", "sample", ACTION_N, A, ACTION_SEED) for A in ACTION_COUNTS]


def action_images(A):
    """given_images' offset for the action-count case A: 21 (its pool's last nine images are noise) for A = 15,
    two further round the pool per action less."""
    return 21 + 2 * (15 - A)


def case_inputs(case):
    """(policy, images u8, quadrants u8) of a case."""
    if case.kind == "actions":
        return (action_policy(case.seed, case.A),) + given_images(case.N, action_images(case.A))
    img, quad = given_images(case.N, case.seed)
    if case.kind == "calibrated":
        return calibrated_policy(case.seed, case.A, img), img, quad
    return random_policy(case.seed, case.A), img, quad
