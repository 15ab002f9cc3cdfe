"""The fp16x2 trunk after the single-issue fp32 forms of csrc/conv_wino4.hip (two-wide fp32
operations issued one element per instruction: the input transform's ship -- col_comb,
combine_kx -- the fold's and the epilogues' were measured too): the same IEEE operations, so
the same results.

On the seeded cases of tests/trunk_cases.py -- B = 1, 2, 3 and 5 boards (a half-empty two-board
workgroup, a full one, odd tails), one residual block and all five, a random board, an all-zero
board, a board with stones on the edges and corners only, per-board ranges from 1e-3 to 1e3 --
the persistent trunk + heads launch and the per-layer conv launches are checked
  * against an fp64 host reference with the bar tests/test_nn_gpu.py uses: error <= 2x that of
    the untouched fp32 MFMA kernel az_conv3x3_gpu (the same net with precision="fp32") on the
    tower output (normalised per board: + 1e-7 max, + 1e-9 mean) and on priors and values
    (+ 1e-6);
  * bit for bit (-0 = +0) against tests/golden/trunk_bits.npz, the parent commit's outputs on
    the same inputs (tests/golden/make_trunk_bits.py)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trunk_cases as tc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _nets(n_blocks):
    """(fp16x2 net, fp32 MFMA net, fp64 host outputs on the five boards), built once."""
    from Models import inference_copy

    net = tc.make_net(n_blocks)
    x5 = tc.planes5()
    n64 = copy.deepcopy(net).double()
    with torch.no_grad():
        x64 = x5.double().view(5, 1, 8, 8)
        h64 = n64.res(F.relu(n64.bn0(n64.conv0(x64))))
        logits, v64 = n64(x64)
    ref = (torch.softmax(logits, -1).numpy(), v64.reshape(-1).numpy(), h64.numpy())
    return inference_copy(net, "cuda"), inference_copy(net, "cuda", precision="fp32"), ref


@functools.lru_cache(maxsize=None)
def _fp32_outputs(n_blocks, B):
    _, f32, _ = _nets(n_blocks)
    return tc.run(f32, tc.planes5()[:B].cuda().contiguous(), "layers")


def test_inputs_are_the_recorded_ones(golden):
    assert np.array_equal(golden("trunk_bits.npz")["planes"], tc.planes5().numpy())
    p = tc.planes5().numpy()
    assert not p[1].any() and p[2].reshape(8, 8)[1:7, 1:7].any() == False  # noqa: E712
    assert p[2].any() and np.abs(p).max() == 1e3 and np.abs(p[p != 0]).min() < 2e-3


@pytest.mark.parametrize("B", tc.BATCHES)
@pytest.mark.parametrize("n_blocks", tc.BLOCKS)
@pytest.mark.parametrize("kind", tc.KINDS)
def test_trunk_same_results(kind, n_blocks, B, golden):
    fused, _, (pr64, va64, h64) = _nets(n_blocks)
    assert fused.precision == "fp16x2"
    pr, va, h = tc.run(fused, tc.planes5()[:B].cuda().contiguous(), kind)
    pr32, va32, h32 = _fp32_outputs(n_blocks, B)
    assert np.isfinite(pr).all() and np.isfinite(va).all() and np.isfinite(h).all()
    # fp64 bar: the tower output relative to each board's magnitude
    ref = h64[:B]
    scale = np.maximum(np.abs(ref).max(axis=(1, 2, 3), keepdims=True), 1e-30)
    e_h, e_32 = np.abs(h.astype(np.float64) - ref) / scale, np.abs(h32.astype(np.float64) - ref) / scale
    print(kind, n_blocks, B, "tower max", e_h.max(), e_32.max(), "mean", e_h.mean(), e_32.mean())
    assert e_h.max() <= 2 * e_32.max() + 1e-7, (e_h.max(), e_32.max())
    assert e_h.mean() <= 2 * e_32.mean() + 1e-9, (e_h.mean(), e_32.mean())
    for got, got32, want in ((pr, pr32, pr64[:B]), (va, va32, va64[:B])):
        e, e32 = np.abs(got - want).max(), np.abs(got32 - want).max()
        print("  heads", e, e32)
        assert e <= 2 * e32 + 1e-6, (e, e32)
    # the parent commit's bits (== on floats: -0 equals +0; no NaN above)
    g = golden("trunk_bits.npz")
    assert np.array_equal(pr, g[tc.key(kind, n_blocks, B, "pr")])
    assert np.array_equal(va, g[tc.key(kind, n_blocks, B, "va")])
    assert tc.bits_sha(h) == str(g[tc.key(kind, n_blocks, B, "h_sha")])
