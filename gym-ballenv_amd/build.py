"""In-tree build of libballenv.so (gfx950) -- also run by __graft_entry__.build().

    python -m gym_ballenv_amd.build [--force]

Translation units, compiled separately (each embeds its own gfx950 code
object) and linked into one shared library:
  csrc/ballenv.hip  the step engine's kernels (step / reset / observe, the fused rollouts, the
                    autoreset pool's fill) and their dispatcher
  csrc/abi.hip      be_ctx and the step engine's C entry points (no kernels; step_types.h is the
                    interface between the two)
  csrc/internal.h   the host toolkit every unit's entry points share: error reporting, entering a
  csrc/host_logic.h context's device, the status word (internal.h); the pool's bookkeeping, the blob
                    layout, be_pool_entry's word order, be_out_at (host_logic.h: no HIP, CPU-tested)
  csrc/policy.hip   select_action kernel (-fno-slp-vectorize: scalar f32 FMAs
                    interleave better with MFMAs than SLP-packed ones on gfx950)
  csrc/features.hip sibling observation formats (prep_state2 block counts)
  csrc/pixels.hip   the pixel agent's observation (extract_patch: the 100 x 100 patch around the agent as row
                    bitmasks, PIL's bicubic resize to 40 x 40 byte for byte); its host half without HIP --
                    PIL's coefficients, the argument checks -- is csrc/pixels_host.h (CPU-tested)
  csrc/board.hip    the createBoard physics profile + featureExtractor
  csrc/a2c.hip      A2C targets of a recorded rollout (the batched finish_episode)
  csrc/a2c_grad.hip A2C losses and Policy gradients of recorded rows (f32 MFMAs; no VGPR_MFMA:
                    its accumulators live for the whole kernel, and with them in VGPRs the W = 10
                    instance measured 14 % slower, W = 5 the same: profiles/a2c_grad_ab.json)
  csrc/optim_core.h the pinned optimiser arithmetic, once: an Adam step's constants, one element's Adam
                    and SGD update (f64 operations with -ffp-contract=off, as every unit: no FMA)
  csrc/a2c_adam.hip the Adam step on the six Policy tensors and the re-pack of the policy image
                    (optim_core.h); and the one-thread state kernel all three optimiser entries launch
  csrc/mlp_policy.hip select_action of the REINFORCE / supervised block-count MLP (f32 MFMAs) straight
                    from the env state; shares blocks_core.h (prep_state2 of one env) with features.hip;
                    and next to its pack kernel the Adam / SGD step fused with the re-pack (be_mlp_opt,
                    optim_core.h)
  csrc/mlp_core.h   the block MLP's packed image and forward, shared by mlp_policy.hip (be_mlp_act) and ballenv.hip's
                    fused block-policy rollout (mlp_rollout_kernel behind be_mlp_rollout); ballenv.hip's
                    VGPR_MFMA holds for it as for the fused policy rollouts: its accumulators are read by VALU code
                    (relu, the logits) right after each layer
  csrc/mlp_grad.hip the block-count MLP's REINFORCE / cross-entropy losses and gradients of recorded rows
                    (f32 MFMAs; no VGPR_MFMA, for a2c_grad.hip's reason: the gradient accumulators live
                    for the whole kernel, the AGPR half of the register file is where they belong)
  csrc/cnn_policy.hip select_action of the pixel agent's conv net (f32 MFMAs as implicit GEMMs, the reference's
                    per-env BatchNorm statistics) on be_observe_pixels' image (be_cnn_act), and next
                    to its pack kernel the Adam step fused with the re-pack (be_cnn_adam, optim_core.h, DESIGN
                    3.21); its host half without HIP -- the packed image's layout, its index function and that
                    function's inverse, the argument checks -- is csrc/cnn_host.h (CPU-tested)
  csrc/cnn_grad.hip the pixel agent's REINFORCE loss and gradients of recorded rows (be_cnn_grad, DESIGN 3.20: f32
                    MFMAs, the accumulators in the AGPR half as mlp_grad.hip's) and be_observe_quadrant; its host
                    half without HIP -- the workspace's layout, the argument checks -- is csrc/cnn_grad_host.h
                    (CPU-tested)
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.realpath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
HDR = os.path.join(ROOT, "include", "ballenv.h")
OUT = os.path.join(PKG, "libballenv.so")
ARCH = os.environ.get("BALLENV_OFFLOAD_ARCH", "gfx950")

BASE_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", f"--offload-arch={ARCH}"]
# -amdgpu-mfma-vgpr-form: MFMA accumulators in VGPRs.  The compiler's default put the fc1
# tiles' accumulators in AGPRs, which costs 12 v_accvgpr_read per tile row (of ~70 VALU); only
# the kernels with MFMAs (the policy forward and the fused policy rollouts) change.
VGPR_MFMA = ["-mllvm", "-amdgpu-mfma-vgpr-form"]
# -amdgpu-kernarg-preload-count: leading scalar kernel arguments (up to 14 dwords) arrive in user
# SGPRs at wave launch instead of through a scalar load from the kernarg segment (step2_kernel's
# prologue); the compiler keeps an s_load entry for firmware without the preload.
KARG_PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
UNITS = {"ballenv.hip": [*VGPR_MFMA, *KARG_PRELOAD], "abi.hip": [], "policy.hip": ["-fno-slp-vectorize", *VGPR_MFMA],
         "features.hip": [], "pixels.hip": [], "board.hip": [], "a2c.hip": [], "a2c_grad.hip": [], "a2c_adam.hip": [],
         "mlp_policy.hip": [], "mlp_grad.hip": [], "cnn_policy.hip": [], "cnn_grad.hip": []}
HEADERS = [HDR, *(os.path.join(CSRC, h) for h in ("philox.h", "internal.h", "host_logic.h", "pool_layout.h", "policy_core.h", "blocks_core.h", "mlp_core.h", "diag.h",
                                              "step_types.h", "optim_core.h", "pixels_host.h", "cnn_host.h", "cnn_grad_host.h"))]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force: bool = False, verbose: bool = True, extra_flags=(), out: str = OUT) -> str:
    srcs = [os.path.join(CSRC, u) for u in UNITS]
    if not (force or extra_flags or _stale(out, [*srcs, *HEADERS, __file__])):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
    objs, cmds = [], []
    for u, flags in UNITS.items():
        obj = f"{out}.{os.path.splitext(u)[0]}.o"
        objs.append(obj)
        cmds.append([hipcc, *BASE_FLAGS, *flags, *extra_flags, *inc, "-c", os.path.join(CSRC, u), "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(len(cmds)) as ex:
        list(ex.map(run, cmds))
    link = [hipcc, "-shared", f"--offload-arch={ARCH}", *objs, "-o", out + ".tmp"]
    run(link)
    os.replace(out + ".tmp", out)
    for o in objs:
        os.remove(o)
    return out


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
