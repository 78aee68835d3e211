"""The pixel agent of examples/ball_cnn_reinforce.py on the batched env.

``PixelPolicy`` is the reference's ``Policy`` (:60-83) as a plain torch module: three 5 x 5 stride-2
convolutions with BatchNorm on the 40 x 40 patch image, then ``Linear(132, 9)`` on the 128 features
and the 4 quadrant inputs, softmax.  Its inputs come from the env's HIP observation kernels
(``BatchedBallEnv.observe_pixels`` / ``observe_blocks``); the network itself runs in torch.

    policy = PixelPolicy().to(env.device)
    image, quadrant = pixel_inputs(env)              # (N, 3, 40, 40) f32, (N, 4) f32
    probs = policy(image, quadrant)                  # (N, 9)
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


class PixelPolicy(nn.Module):
    """ball_cnn_reinforce.py:60-83 (state_dict keys as the reference's: conv1..3, bn1..3, head)."""

    def __init__(self, num_actions: int = 9):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, kernel_size=5, stride=2)
        self.bn1 = nn.BatchNorm2d(16)
        self.conv2 = nn.Conv2d(16, 32, kernel_size=5, stride=2)
        self.bn2 = nn.BatchNorm2d(32)
        self.conv3 = nn.Conv2d(32, 32, kernel_size=5, stride=2)
        self.bn3 = nn.BatchNorm2d(32)
        self.head = nn.Linear(132, num_actions)       # 32 x 2 x 2 features + the quadrant one-hot

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.relu(self.bn3(self.conv3(x)))
        x = torch.cat((x.view(x.size(0), -1), y), 1)
        return F.softmax(self.head(x), dim=1)         # the reference's implicit dim of a 2-d input


def pixel_inputs(env):
    """Both inputs of :class:`PixelPolicy` for every env's current state: the (N, 3, 40, 40) f32
    patch image (extract_patch, :120-163) and the (N, 4) f32 quadrant one-hot of the goal (the first
    four block-count inputs, prep_state2's quadrant)."""
    return env.observe_pixels(f32=True), env.observe_blocks(f32=True)[:, :4]
