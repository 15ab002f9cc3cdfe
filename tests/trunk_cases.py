"""The seeded cases of tests/test_trunk_f32_issue_gpu.py and tests/golden/make_trunk_bits.py:
AlphaZeroNet(n blocks x 128) on the fp16x2 trunk at a few boards, as the persistent trunk +
heads launch (az_trunk_wino4_heads_gpu / az_trunk_wino4_gpu) and as one launch per conv
(az_conv3x3_wino4_gpu, the heads fused into the last)."""
import hashlib
import os

import numpy as np
import torch

BATCHES = (1, 2, 3, 5)
BLOCKS = (1, 5)
KINDS = ("trunk", "layers")


def planes5():
    """Five canonical boards [5, 64]: random stones, an all-zero board, stones on the edges and
    corners only, two more random ones -- each times its own power of ten from 1e-3 to 1e3 (the
    stem is a plain fp32 convolution of these floats, so every layer sees per-board ranges six
    decades apart).  The first B rows are the batch of B."""
    rng = np.random.default_rng(20240521)
    p = rng.integers(-1, 2, size=(5, 8, 8)).astype(np.float32)
    p[1] = 0.0
    edge = np.zeros((8, 8), bool)
    edge[0, :] = edge[7, :] = edge[:, 0] = edge[:, 7] = True
    p[2] = np.where(edge, rng.choice(np.array([-1.0, 1.0], np.float32), size=(8, 8)), 0.0)
    # the all-zero board has no range of its own: the other four span the six decades
    scale = np.array([1e3, 1.0, 1e-3, 10 ** -1.5, 10 ** 1.5], np.float32)
    return torch.from_numpy((p * scale[:, None, None]).reshape(5, 64))


def make_net(n_blocks):
    """The seeded random-init net; its BatchNorm statistics moved off the identity so the folded
    biases and scales are not trivial (the stem's shift aside, below)."""
    from Models import AlphaZeroNet

    g = torch.Generator().manual_seed(1000 + n_blocks)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(2000 + n_blocks)
        net = AlphaZeroNet(8, 65, n_blocks, 128)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.running_mean.copy_(0.05 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(1.0 + 0.2 * torch.rand(m.running_var.shape, generator=g))
        # no shift in the stem: the first block conv's input is the stem's ReLU of a pure
        # scaling of the planes -- all zeros for the all-zero board (input range 0), and
        # per-board ranges the same six decades apart as the planes
        net.bn0.bias.zero_()
        net.bn0.running_mean.zero_()
    return net.eval()


def run(fused, x, kind):
    """(priors [B, 65], values [B], tower output [B, 128, 8, 8]) of the fused net on planes x:
    kind "trunk" = the persistent launches, "layers" = one launch per conv.  The small-batch
    channel-split form is switched off for the call: these few boards run the whole-K kernels."""
    from Models import FusedInferenceNet

    B = x.shape[0]
    old_env, old_flag = os.environ.get("AZ_SPLITK"), FusedInferenceNet.fuse_trunk4
    os.environ["AZ_SPLITK"] = "0"
    FusedInferenceNet.fuse_trunk4 = kind == "trunk"
    try:
        pr = torch.full((B, 65), float("nan"), device="cuda")
        va = torch.full((B,), float("nan"), device="cuda")
        with torch.no_grad():
            fused.evaluate_into(x, pr, va)
            h = fused._trunk(x.view(B, 1, 8, 8))
        torch.cuda.synchronize()
    finally:
        FusedInferenceNet.fuse_trunk4 = old_flag
        if old_env is None:
            del os.environ["AZ_SPLITK"]
        else:
            os.environ["AZ_SPLITK"] = old_env
    return pr.cpu().numpy(), va.cpu().numpy(), h.cpu().numpy()


def bits_sha(a):
    """sha256 of an fp32 array's bits in NCHW order with -0 counted as +0 (x + 0 is +0 for both)."""
    a = np.ascontiguousarray(a, dtype=np.float32) + np.float32(0.0)
    return hashlib.sha256(a.tobytes()).hexdigest()


def key(kind, n_blocks, B, what):
    return f"{kind}_nb{n_blocks}_B{B}_{what}"
