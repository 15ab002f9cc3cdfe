"""The FP16X2 kernels' numeric range contract: any finite fp32 board -- an all-zero board, a
board of subnormals and boards from 1e-41 to 1e30 in one batch included -- and any finite
weight tensor gives fp32-class output.  Every kernel on the default inference path scales its
operands by a power of two taken from a max |x| word before the fp16 hi / lo split and removes
the scales in its epilogue (az_scale_exp, csrc/common.h); these tests walk those exponents to
both ends and through their sum.

The bar is the one of test_nn_gpu.py's FP16X2 tests: against an fp64 reference on the CPU, with
the errors normalised per board by that board's max |ref|, max error <= 2x the fp32 MFMA
kernel's (az_conv3x3_gpu on the same inputs) + 1e-7 and mean error <= 2x + 1e-9; the output
finite everywhere."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")
from Models import (AlphaZeroNet, FastOthelloNet, FusedInferenceNet, board_absmax,  # noqa: E402
                    fp16x2_scale_exp, inference_copy)
from test_nn_gpu import _case, _mx_conv, _wino_conv  # noqa: E402

# one factor per board; neighbours (two- and four-board workgroups) mix the extremes, and the
# ninth board is a partial last workgroup in both forms.  1e-41: every value subnormal;
# 1.2e-38: the board's max just above the smallest normal, most values subnormal
LADDER = [1e30, 0.0, 1e-35, 1.0, 1e-41, 1e20, 1.2e-38, 1e3, 1e-20]

# kernel forms: (channels, launcher); the wino4 forms also return the per-board max |y|
FORMS = ["mx64", "mx128", "w4", "w4x4", "sk4", "sk16"]
RES_RELU = [(False, True), (True, True), (False, False)]


def _channels(form):
    return 64 if form == "mx64" else 128


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _conv64(x, w, b):
    return F.conv2d(x.cpu().double(), w.cpu().double(), b.cpu().double(), padding=1)


def _ref(conv64, r, res, relu):
    ref = conv64 + (r.cpu().double() if res else 0)
    return F.relu(ref) if relu else ref


def _fp32_conv(x, w, b, r, relu):
    B, C = x.shape[0], x.shape[1]
    w9 = w.permute(2, 3, 0, 1).reshape(9, C, C).contiguous()
    y = torch.empty_like(x, memory_format=torch.channels_last)
    nat.check(nat.lib.az_conv3x3_gpu(nat.ptr(x), nat.ptr(w9), nat.ptr(b),
                                     None if r is None else nat.ptr(r), nat.ptr(y), B, C,
                                     int(relu), nat.stream_ptr()), "az_conv3x3_gpu")
    torch.cuda.synchronize()
    return y


def _run(form, x, w, b, r, relu, monkeypatch, in_absmax=None):
    """One FP16X2 conv in the given form: (y, out_absmax or None, the consumed in_absmax)."""
    if form.startswith("mx"):
        return _mx_conv(x, w, b, r, relu, nat.AZ_CONV_FP16X2), None, None
    monkeypatch.setenv("AZ_W4_BOARDS", "4" if form == "w4x4" else "2")
    splits = int(form[2:]) if form.startswith("sk") else 0
    if in_absmax is None:
        in_absmax = board_absmax(x)
    amax = torch.zeros(x.shape[0], dtype=torch.float32, device="cuda")
    y = _wino_conv(x, w, b, r, relu, nat.AZ_CONV_FP16X2, fn="az_conv3x3_wino4_gpu",
                   out_absmax=amax, splits=splits, in_absmax=in_absmax)
    return y, amax, in_absmax


def _bad_boards(t):
    return (~torch.isfinite(t)).flatten(1).any(1).nonzero().flatten().tolist()


def _assert_bar(y, y32, ref, tag=""):
    """The file's bar: `ref` (fp64) representable in fp32, `y` finite, and y's error per board
    (normalised by the board's max |ref|) within 2x the fp32 kernel's."""
    assert torch.isfinite(ref.float()).all(), (tag, "reference not finite in fp32")
    assert torch.isfinite(y).all(), (tag, "non-finite boards", _bad_boards(y))
    assert torch.isfinite(y32).all(), (tag, "fp32 kernel non-finite boards", _bad_boards(y32))
    scale = ref.abs().amax(dim=(1, 2, 3), keepdim=True).clamp_min(1e-300)
    e_h = (y.cpu().double() - ref).abs() / scale
    e_32 = (y32.cpu().double() - ref).abs() / scale
    per_board = [(bi, float(e_h[bi].max()), float(e_32[bi].max())) for bi in range(y.shape[0])]
    print(tag, "max", float(e_h.max()), float(e_32.max()), "mean", float(e_h.mean()),
          float(e_32.mean()), "per board", per_board)
    assert e_h.max() <= 2 * e_32.max() + 1e-7, (tag, e_h.max(), e_32.max(), per_board)
    assert e_h.mean() <= 2 * e_32.mean() + 1e-9, (tag, e_h.mean(), e_32.mean())


@functools.lru_cache(maxsize=None)
def _ladder(C):
    """The range ladder at C channels (shared, never written): x, w, b, r and conv(x) in fp64."""
    x, w, b, r, _ = _case(C, len(LADDER), C * 43 + 9)
    x = _cl(x.cpu() * torch.tensor(LADDER, dtype=torch.float32).view(-1, 1, 1, 1))
    assert (x[1] == 0).all() and (x[4].abs() < 1.18e-38).all() and (x[4] != 0).any()
    assert 1.18e-38 < x[6].abs().max() < 1e-37
    return x, w, b, r, _conv64(x, w, b)


@pytest.mark.parametrize("res,relu", RES_RELU)
@pytest.mark.parametrize("form", FORMS)
def test_range_ladder(form, res, relu, monkeypatch):
    """Boards from all-zero and all-subnormal to 1e30 in one batch, randn bias, a residual of
    order 1.  The wino4 forms also: the per-board max |y| output exact, in_absmax consumed, and
    a second conv fed that max |y| (the chained-range path of the tower) within the same bar."""
    x, w, b, r, c64 = _ladder(_channels(form))
    rr = r if res else None
    y, amax, in_amax = _run(form, x, w, b, rr, relu, monkeypatch)
    _assert_bar(y, _fp32_conv(x, w, b, rr, relu), _ref(c64, r, res, relu), form)
    if amax is None:
        return
    assert torch.equal(amax, y.abs().amax(dim=(1, 2, 3)))
    assert (in_amax == 0).all()
    y2, amax2, _ = _run(form, y, w, b, rr, relu, monkeypatch, in_absmax=amax)
    _assert_bar(y2, _fp32_conv(y, w, b, rr, relu), _ref(_conv64(y, w, b), r, res, relu),
                form + " chained")
    assert torch.equal(amax2, y2.abs().amax(dim=(1, 2, 3)))
    assert (amax == 0).all()


@functools.lru_cache(maxsize=None)
def _relative(C):
    x, w, _, _, _ = _case(C, 5, C * 47 + 5)
    s = torch.tensor([2.0 ** k for k in (-60, -30, 0, 30, 60)]).view(-1, 1, 1, 1)
    x = _cl(x.cpu() * s)
    b = torch.zeros(C, device="cuda")
    return x, w, b, _conv64(x, w, b)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("form", FORMS)
def test_relative_accuracy_without_bias_floor(form, relu, monkeypatch):
    """Zero bias, no residual, boards times 2^-60 .. 2^60 (every intermediate a normal fp32):
    each board's error relative to its own magnitude -- a kernel that scaled a small board by
    its neighbour's range would lose it entirely."""
    x, w, b, c64 = _relative(_channels(form))
    y, amax, _ = _run(form, x, w, b, None, relu, monkeypatch)
    _assert_bar(y, _fp32_conv(x, w, b, None, relu), _ref(c64, None, False, relu), form)
    if amax is not None:
        assert torch.equal(amax, y.abs().amax(dim=(1, 2, 3)))


# (weight exponent, board exponent): the weights and the boards times these powers of two; None
# = an all-zero weight tensor.  (-40, -40): products near 1e-25 under a bias of order 1 -- the
# two scale exponents add in the epilogue.  -120: the weights' max (about 2^-123, most of them
# subnormal) is under 2^-112, where an unclamped weight scale 2^(15 - e) is inf (at -100 the max
# is about 2^-103 and the scale 2^118)
WEIGHTS = [(-120, 0), (-100, 0), (-40, 0), (0, 0), (40, 0), (None, 0), (-40, -40)]


@pytest.mark.parametrize("wexp,xexp", WEIGHTS)
@pytest.mark.parametrize("form", ["mx64", "mx128", "w4", "sk4"])
def test_weight_ladder(form, wexp, xexp, monkeypatch):
    """The weight scale of az_conv3x3_mx_prep_gpu / az_conv3x3_wino_prep_gpu (FP16X2) from tiny
    to large weights, then the conv: the same bar; all-zero weights give relu(bias + res)
    exactly."""
    C = _channels(form)
    x, w, b, r, _ = _case(C, 3, C * 53 + 3)
    w = torch.zeros_like(w) if wexp is None else w * 2.0 ** wexp
    x = (x * 2.0 ** xexp).contiguous(memory_format=torch.channels_last)
    y, _, _ = _run(form, x, w, b, r, True, monkeypatch)
    _assert_bar(y, _fp32_conv(x, w, b, r, True), _ref(_conv64(x, w, b), r, True, True),
                f"{form} w*2^{wexp} x*2^{xexp}")
    if wexp is None:
        assert torch.equal(y, F.relu(b.view(1, -1, 1, 1) + r))


@pytest.mark.parametrize("wexp", [0, -100])
@pytest.mark.parametrize("tile,splits", [(32, 8), (64, 16)])
def test_heads_fast_gemm_range(tile, splits, wexp):
    """az_heads_fast_gemm_gpu's per-(board, K-slice) feature scale: single slices all zero,
    subnormal (x 1e-41), tiny-normal (x 1e-35) and large (x 1e20) next to ordinary slices of
    the same board, a ragged last row tile, and the weights times 2^-100 (wshift as Models.py
    computes it): test_heads_fast_gemm_is_fp32_accurate's bar against fp64."""
    B, K = 33, 4096
    ks = K // splits
    g = torch.Generator().manual_seed(tile * 3 + splits)
    x = torch.randn(B, K, generator=g).relu()
    blocks = {(0, 0): 0.0, (1, 1): 1e-41, (2, 2): 1e-35, (3, 3): 1e20, (4, 0): 1e-35,
              (4, splits - 1): 1e20, (31, splits - 1): 1e-41, (32, 0): 0.0,
              (32, splits - 1): 1e-35}
    for (bi, sl), f in blocks.items():
        x[bi, sl * ks:(sl + 1) * ks] *= f
    x[5] = 0.0  # a whole board of zeros
    w = torch.randn(K, 129, generator=g) / 64.0 * 2.0 ** wexp
    ref = x.double() @ w.double()
    xd, wd = x.cuda().contiguous(), w.cuda()
    wshift = 15 - fp16x2_scale_exp(wd[:, :128].abs().max())
    assert -126 < wshift < 126
    ws = wd[:, :128] * (2.0 ** wshift)
    hi = ws.half()
    lo = (ws - hi.float()).half()
    wq = torch.stack([p.view(256, 16, 128).permute(0, 2, 1) for p in (hi, lo)], 1).contiguous()
    w128 = wd[:, 128].contiguous()
    ld = 132
    part = torch.full((splits, B, ld), float("nan"), device="cuda")
    nat.check(nat.lib.az_heads_fast_gemm_gpu(nat.ptr(xd), nat.ptr(wq.view(torch.int16)),
                                             nat.ptr(w128), wshift, nat.ptr(part), ld, splits,
                                             tile, B, nat.stream_ptr()), "az_heads_fast_gemm_gpu")
    torch.cuda.synchronize()
    bad = (~torch.isfinite(part)).any(2).nonzero().tolist()
    assert not bad, ("non-finite partials at (slice, board)", bad)
    assert (part[:, :, 129:] == 0).all()
    got = part.double().sum(0)[:, :129].cpu()
    f32 = (xd @ wd).double().cpu()
    e_g, e_32 = (got - ref).abs(), (f32 - ref).abs()
    print("max", float(e_g.max()), float(e_32.max()))
    assert e_g.max() <= 2 * e_32.max() + 1e-6, (e_g.max(), e_32.max())
    for bi in range(B):
        assert e_g[bi].max() <= 2 * e_32[bi].max() + 1e-7 * (1 + ref[bi].abs().max()), (
            bi, e_g[bi].max(), e_32[bi].max())


def _net(kind, variant):
    """A net whose tower meets the range ends.  "dead": a middle block's second BatchNorm bias
    at -1e6, so that block hands an all-zero board to every later layer, for every input;
    "tiny": the stem's BatchNorm weight and bias times 1e-36, so every board enters the tower
    with a max near 1e-36."""
    torch.manual_seed(13)
    net = AlphaZeroNet(8, 65, 3, 128) if kind == "az" else FastOthelloNet(8, 65)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.5, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.2, 0.2)
    if variant == "dead":
        (net.res[1] if kind == "az" else net.res_block).bn2.bias.data.fill_(-1e6)
    else:
        bn = net.bn0 if kind == "az" else net.initial_conv[1]
        bn.weight.data.mul_(1e-36)
        bn.bias.data.mul_(1e-36)
    return net.cuda().eval()


def _planes(B):
    g = torch.Generator().manual_seed(B)
    x = torch.randint(-1, 2, (B, 64), generator=g).float()
    x[0] = 0.0  # the all-empty board
    return x.cuda()


def _evaluate(fused, x):
    pr = torch.full((x.shape[0], 65), float("nan"), device="cuda")
    va = torch.full((x.shape[0],), float("nan"), device="cuda")
    with torch.no_grad():
        fused.evaluate_into(x, pr, va)
    torch.cuda.synchronize()
    return pr, va


def _assert_matches_module(net, x, pr, va):
    assert torch.isfinite(pr).all() and torch.isfinite(va).all(), (
        "non-finite boards", _bad_boards(pr), (~torch.isfinite(va)).nonzero().flatten().tolist())
    torch.testing.assert_close(pr.sum(1), torch.ones_like(va), atol=1e-5, rtol=0)
    with torch.no_grad():
        logits, v = net(x.view(-1, 1, 8, 8))
    torch.testing.assert_close(pr, torch.softmax(logits, -1), atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(va, v.reshape(-1), atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("B", [257, 9])
@pytest.mark.parametrize("variant", ["dead", "tiny"])
def test_inference_copy_az_range(variant, B, monkeypatch):
    """AlphaZeroNet(8, 65, 3, 128) through the default inference copy: B = 257 runs the
    persistent trunk (its stem, its LDS range hand-off between layers, the heads in its
    launch), B = 9 the split-K convs.  Priors and values finite, normalised and equal to the
    eval-mode module's at this suite's tolerance; the three head placements and the per-layer
    launches bit-identical on these inputs too."""
    net = _net("az", variant)
    fused = inference_copy(net, "cuda")
    assert fused.precision == "fp16x2"
    assert FusedInferenceNet.splitk_for(B) == (0 if B == 257 else 8)
    x = _planes(B)
    out = {}
    for name, fh, th in (("separate", False, False), ("conv", True, False), ("trunk", True, True)):
        monkeypatch.setattr(FusedInferenceNet, "fuse_heads", fh)
        monkeypatch.setattr(FusedInferenceNet, "trunk_heads", th)
        out[name] = _evaluate(fused, x)
    monkeypatch.setattr(FusedInferenceNet, "fuse_trunk4", False)
    out["layers"] = _evaluate(fused, x)
    _assert_matches_module(net, x, *out["trunk"])
    for name in ("separate", "conv", "layers"):
        assert torch.equal(out[name][0], out["trunk"][0]), name
        assert torch.equal(out[name][1], out["trunk"][1]), name


@pytest.mark.parametrize("variant", ["dead", "tiny"])
def test_inference_copy_fast_range(variant, monkeypatch):
    """FastOthelloNet at B = 33 through the default inference copy: the fast trunk (stem,
    residual block and conv_add in one launch, the ranges handed on in LDS) and the heads
    GEMM; the three stem-fused / plain direct conv launches bit-identical."""
    net = _net("fast", variant)
    fused = inference_copy(net, "cuda")
    assert fused._fast_trunk_ready() and fused._fast_heads_ready()
    x = _planes(33)
    pr, va = _evaluate(fused, x)
    _assert_matches_module(net, x, pr, va)
    with torch.no_grad():
        a = fused._fast_trunk(x)
        b = fused.tail(fused._trunk(x.view(-1, 1, 8, 8)))
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    monkeypatch.setattr(FusedInferenceNet, "fuse_fast_trunk", False)
    pr3, va3 = _evaluate(fused, x)
    assert torch.equal(pr3, pr) and torch.equal(va3, va)
