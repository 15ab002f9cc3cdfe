"""The heads kernels at peaked inputs: logits spread over about +-80 inside a board, two equal
maxima, pre-tanh values from 0.01 to 40 in both signs.  Random-init nets give near-uniform
priors and values near 0, where `atol=1e-5` passes a prior of 1e-6 that is wholly wrong; here
every prior is judged in log space and every value against tanh's slope.

The reference of each case is the same operation in float64 on the CPU, from the same float32
inputs and weights.  The bounds are forward-error bounds computed in float64 from magnitudes,
never from what a kernel returned.  With u = 2^-24 (float32 unit roundoff):

  * a K-term float32 dot product plus its bias, summed in any order, errs by at most
    (K + 4) u sum|terms| to first order (gamma_K of the standard analysis; the 4 covers the
    bias add and the regrouping into quarters / partial sums).  Through a chain of layers the
    bound of a layer's input is carried by the next layer's |weights| (ReLU is 1-Lipschitz)
    and that layer's own term is added.  D = the largest such bound over a board's 65 logits,
    Dv = the bound of its pre-tanh value.
  * softmax: log p_j = l_j - logsumexp(l).  logsumexp is 1-Lipschitz in the sup norm (its
    gradient is the softmax: non-negative, summing to 1), so with every logit within D of the
    reference's, l_j moves by at most D and logsumexp(l) by at most D: 2 D in all.  The
    float32 evaluation adds: the subtraction (u |l - m|), the scaling of the exponent's
    argument by log2(e) in the fast exponential (u |l - m|), the hardware exponential (1 ulp),
    the 65-term tree sum of non-negative terms (7 u), the reciprocal or division (1 ulp) and
    the product (u): under 16 u (1 + |l_ref - m_ref|).  Hence
        |log p - log p_ref| <= 2 D + 16 u (1 + |l_ref - m_ref|).
    Below p_ref = 2^-120 the exponential may flush to zero: only p <= 2^-119 is required.
  * row sum: each p_j = e_j * inv with sum e_j * inv within 65 u of 1 (the tree sum, the
    reciprocal and 65 product roundings, all relative to terms that sum to 1).
  * value: tanh's slope at x is 1 - tanh(x)^2, so
        |v - tanh(x_ref)| <= (1 - tanh(x_ref)^2) Dv + 4 u
    (4 u: tanhf within 2 ulp of a result below 1, and the final rounding).  This is first
    order in Dv: the dropped term is at most 0.39 Dv^2 (|tanh''| <= 0.77), a few per cent of
    the first-order one where Dv is below a hundredth; where the scaled weights cancel
    harder, Dv -- a worst case over all roundings that no evaluation comes near -- grows past
    that, and the bound asserted stays the first-order one: the tighter of the two.  For
    |x| >= 10, 1 - tanh(x) < 2^-27: the float32 nearest to tanh(x) is exactly +-1.  The
    check is made where |x_ref| >= 10 + min(Dv, 1): the pre-activation the kernel itself
    forms may lie inside x_ref by its error.  The margin is capped at 1 because Dv, a worst
    case, runs to several units on some boards while real roundings stay a hundredth of it
    (see the statistical assertion below); uncapped it would excuse most boards between 10
    and 16.
  * argmax: logits further apart than 2 D cannot swap.

What each test can see.  D and Dv are worst cases carried through every layer.  For the
finish kernel (one float32 add before the softmax) D is about 2e-5, and that test holds each
prior to a few 1e-5 in log space.  For az_heads_az_gpu the chain is conv (C terms) -> FC (128
or 64 terms) -> FC (256 terms) with weights scaled up to reach the spread: D reaches 0.24 at
C = 128 and Dv several units on boards that are not the scaling target, so there the direct
test catches what is grossly wrong -- NaN, a row or a word from another board, a wrong argmax,
an unequal pair of equal logits, a write past n_boards, a value that is not +-1 when saturated
-- and a subtle error only through the second assertion below.  The tight hold on heads_az.h
is the whole-net test: within 2x the float32 torch module's own error, bit-identical across
its three callers.

A second, statistical assertion narrows the direct tests: the roundings of a K-term chain are
independent and of either sign, so the error behaves as a random walk of standard deviation
about u sqrt(K) sum|terms| / sqrt(K) against the worst case's K u sum|terms|: a correct kernel
sits near 1 / sqrt(K) of the bound (K >= 64 here, so 1/8), not near 1.  Each case asserts its
worst error / bound ratio below 1/2: four such standard deviations, far beyond any run of
correct roundings over the few thousand outputs of the file, and a quarter of what the
worst-case bound alone would let pass.  (The finish kernel's logits are a single add, not a
chain; there the factor comes from the constants -- 5 u for one rounding, 16 u for the
softmax's five -- and the same 1/2 holds.)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("az_native")

U = 2.0 ** -24
NAN = float("nan")
PAD = 3  # rows past n_boards in every output buffer: they must stay NaN


def _dot_bound(aw, ax_bound, terms_abs, bias_abs, K):
    """Error bound of y = x @ w + b in float32: the input's own bound carried by |w|, plus
    (K + 4) u (sum |x w| + |b|)."""
    return ax_bound @ aw + (K + 4) * U * (terms_abs + bias_abs)


def _check_softmax(pr, logits_ref, D, where):
    """pr float32 [n, 65] against float64 reference logits [n, 65] with per-board logit error
    bound D [n] (see the module docstring)."""
    pr = pr.astype(np.float64)
    assert np.isfinite(pr).all(), where
    assert (pr >= 0).all(), where
    rs = pr.sum(1)
    print(f"{where}: max |row sum - 1| / u = {np.abs(rs - 1).max() / U:.2f} (bound 65)")
    assert (np.abs(rs - 1) <= 65 * U).all(), where
    m = logits_ref.max(1, keepdims=True)
    z = logits_ref - m
    logp_ref = z - np.log(np.exp(z).sum(1, keepdims=True))
    tiny = logp_ref < -120 * np.log(2)
    assert (pr[tiny] <= 2.0 ** -119).all(), where
    with np.errstate(divide="ignore"):
        err = np.abs(np.log(pr) - logp_ref)
    bound = 2 * D[:, None] + 16 * U * (1 + np.abs(z))
    ratio = np.where(tiny, 0.0, err / bound)
    print(f"{where}: spread {np.ptp(logits_ref, axis=1).min():.1f}..{np.ptp(logits_ref, axis=1).max():.1f}, "
          f"max D = {D.max():.3g}, worst log-prior error / bound = {ratio.max():.3f}")
    assert (ratio <= 0.5).all(), (where, float(ratio.max()))
    top = np.sort(logits_ref, 1)
    clear = top[:, -1] - top[:, -2] > 2 * D
    assert (pr.argmax(1)[clear] == logits_ref.argmax(1)[clear]).all(), where
    return clear


def _check_values(va, x_ref, Dv, where):
    va = va.astype(np.float64)
    assert np.isfinite(va).all() and (np.abs(va) <= 1).all(), where
    sat = np.abs(x_ref) >= 10 + np.minimum(Dv, 1.0)
    assert (va[sat] == np.sign(x_ref[sat])).all(), where
    t = np.tanh(x_ref)
    bound = (1 - t * t) * Dv + 4 * U
    ratio = np.abs(va - t) / bound
    print(f"{where}: x_ref {np.round(x_ref, 3)}, max Dv = {Dv.max():.3g}, "
          f"worst value error / bound = {ratio.max():.3f}")
    assert (ratio <= 0.5).all(), (where, float(ratio.max()))


# ---- az_heads_az_gpu ---------------------------------------------------------------------

def _az_case(C, n, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    gain = torch.linspace(0.5, 1.5, n).view(n, 1, 1) if n > 1 else 1.0  # boards that differ
    W = {"h": torch.rand(n, 64, C, generator=g) * gain, "wpv": r(3, C) / C ** 0.5, "bpv": r(3) * 0.1,
         "wpolT": r(128, 65), "bpol": r(65), "w1T": r(64, 256) / 8.0, "b1": r(256) * 0.1,
         "w2": r(256) / 16.0, "b2": r(1) * 0.1}
    return {k: v.float().contiguous() for k, v in W.items()}


def _az_reference(W):
    """float64 heads from the float32 tensors: logits [n, 65], pre-tanh [n], and the forward
    error bounds D [n], Dv [n] of a float32 evaluation."""
    d = {k: v.double().numpy() for k, v in W.items()}
    h, wpv, C = d["h"], d["wpv"], d["h"].shape[2]
    conv = h @ wpv.T + d["bpv"]                                   # [n, 64, 3]
    conv_b = _dot_bound(np.abs(wpv.T), np.zeros_like(h), np.abs(h) @ np.abs(wpv.T),
                        np.abs(d["bpv"]), C)
    act = np.maximum(conv, 0)
    p = np.concatenate([act[:, :, 0], act[:, :, 1]], 1)          # NCHW-flat [n, 128]
    p_b = np.concatenate([conv_b[:, :, 0], conv_b[:, :, 1]], 1)
    logits = p @ d["wpolT"] + d["bpol"]
    logits_b = _dot_bound(np.abs(d["wpolT"]), p_b, np.abs(p) @ np.abs(d["wpolT"]),
                          np.abs(d["bpol"]), 128)
    v, v_b = act[:, :, 2], conv_b[:, :, 2]
    hid = v @ d["w1T"] + d["b1"]
    hid_b = _dot_bound(np.abs(d["w1T"]), v_b, np.abs(v) @ np.abs(d["w1T"]), np.abs(d["b1"]), 64)
    rh = np.maximum(hid, 0)
    x = rh @ d["w2"] + d["b2"][0]
    x_b = _dot_bound(np.abs(d["w2"]), hid_b, np.abs(rh) @ np.abs(d["w2"]), np.abs(d["b2"][0]), 256)
    return logits, x, logits_b.max(1), x_b


def _run_az(W):
    n, C = W["h"].shape[0], W["h"].shape[2]
    dev = {k: v.cuda() for k, v in W.items()}
    pr = torch.full((n + PAD, 65), NAN, device="cuda")
    va = torch.full((n + PAD,), NAN, device="cuda")
    nat.check(nat.lib.az_heads_az_gpu(
        nat.ptr(dev["h"]), nat.ptr(dev["wpv"]), nat.ptr(dev["bpv"]), nat.ptr(dev["wpolT"]),
        nat.ptr(dev["bpol"]), nat.ptr(dev["w1T"]), nat.ptr(dev["b1"]), nat.ptr(dev["w2"]),
        nat.ptr(dev["b2"]), nat.ptr(pr), nat.ptr(va), n, C, nat.stream_ptr()), "az_heads_az_gpu")
    torch.cuda.synchronize()
    pr, va = pr.cpu().numpy(), va.cpu().numpy()
    assert np.isnan(pr[n:]).all() and np.isnan(va[n:]).all()  # nothing written past n_boards
    return pr[:n], va[:n]


def _sharpen_policy(W, logits, tie):
    """Scale the policy FC so board 0's logits spread over 160; tie: column j2 becomes a copy
    of j1, board 0's best column below 64 (two lanes running the same instructions), and
    column 64 a copy with its bias one lower, so the pair is board 0's maximum."""
    s = 160.0 / np.ptp(logits[0])
    W["wpolT"] = (W["wpolT"] * s).float()
    W["bpol"] = (W["bpol"] * s).float()
    j1 = int(np.argmax(logits[0, :64]))
    j2 = (j1 + 17) % 64
    if tie:
        for j, drop in ((j2, 0.0), (64, 1.0)):
            W["wpolT"][:, j] = W["wpolT"][:, j1]
            W["bpol"][j] = W["bpol"][j1] - drop
    return j1, j2


def _scale_value(W, x, target, centre):
    """Scale the last value FC so the pre-tanh value of the board where it is largest is
    `target` (to float32 rounding; the largest, so the scaling adds the least cancellation);
    with several boards the bias first centres them, so both signs occur.  Returns that
    board."""
    if centre:
        W["b2"] = (W["b2"] - float(np.mean(x)) + 0.37 * float(np.std(x))).float()
        x = x - float(np.mean(x)) + 0.37 * float(np.std(x))
    ib = int(np.argmax(np.abs(x)))
    t = target / x[ib]
    W["w2"] = (W["w2"] * t).float()
    W["b2"] = (W["b2"] * t).float()
    return ib


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("C", [64, 128])
def test_heads_az_kernel_at_peaked_inputs(C, n, tie):
    base = _az_case(C, n, 1000 * C + 10 * n + tie)
    logits0, x0, _, _ = _az_reference(base)
    for target in (0.01, -0.01, 3.0, -3.0, 40.0, -40.0):
        W = {k: v.clone() for k, v in base.items()}
        j1, j2 = _sharpen_policy(W, logits0, tie)
        ib = _scale_value(W, x0, target, n > 1)
        logits, x, D, Dv = _az_reference(W)
        assert 120 < np.ptp(logits[0]) < 170 and abs(x[ib] / target - 1) < 1e-3
        where = f"C={C} n={n} tie={tie} target={target}"
        pr, va = _run_az(W)
        clear = _check_softmax(pr, logits, D, where)
        _check_values(va, x, Dv, where)
        if tie:
            assert logits[0, j1] == logits[0, j2] == logits[0].max()
            assert (pr[:, j1] == pr[:, j2]).all(), where  # the same instructions on the same words
            assert 0.25 < pr[0, j1] <= 0.5
        else:
            assert clear[0], where


# ---- az_heads_fast_finish_gpu -----------------------------------------------------------

def _finish_case(parts, ld, n, tie, seed):
    """Partial sums that cancel: parts 0 .. P-2 are large (about 1e4) with mixed signs, the
    last one brings the ordered float32 sum back to a small target.  Any other order of the
    float32 additions misses the target by ulps of 1e4 (1e-3), far outside the bounds."""
    rng = np.random.default_rng(seed)
    target = np.zeros((n, ld), np.float32)
    target[:, :65] = rng.uniform(-80, 80, (n, 65))
    target[:, 65:129] = rng.normal(0, 1, (n, 64))
    part = np.zeros((parts, n, ld), np.float32)
    acc = np.zeros((n, ld), np.float32)
    for p in range(parts - 1):
        part[p] = rng.normal(0, 1e4, (n, ld)).astype(np.float32)
        acc = acc + part[p]  # float32, in part order
    part[parts - 1] = target - acc
    bias = np.zeros(ld, np.float32)
    bias[:129] = rng.normal(0, 1, 129)
    if tie:  # as _sharpen_policy: columns j1 = j2 are board 0's maximum, column 64 one below
        j1 = int(np.argmax((target + bias)[0, :64]))
        j2 = (j1 + 17) % 64
        for j, drop in ((j2, 0.0), (64, 1.0)):
            part[:, :, j] = part[:, :, j1]
            bias[j] = bias[j1] - np.float32(drop)
    else:
        j1 = j2 = None
    w2 = rng.normal(0, 0.25, 64).astype(np.float32)
    b2 = rng.normal(0, 0.1, 1).astype(np.float32)
    return part, bias, w2, b2, j1, j2


def _finish_reference(part, bias, w2, b2):
    """The parts added in order in float32 (the kernel's contract), the rest in float64."""
    acc = part[0].copy()
    for p in range(1, len(part)):
        acc = acc + part[p]
    assert acc.dtype == np.float32
    s = acc.astype(np.float64)[:, :129]
    b = bias.astype(np.float64)[:129]
    y = s + b
    y_b = (1 + 4) * U * (np.abs(s) + np.abs(b))  # one float32 add
    logits = y[:, :65]
    hid, hid_b = y[:, 65:], y_b[:, 65:]
    rh = np.maximum(hid, 0)
    w = w2.astype(np.float64)
    x = rh @ w + float(b2[0])
    x_b = _dot_bound(np.abs(w), hid_b, np.abs(rh) @ np.abs(w), abs(float(b2[0])), 64)
    return logits, x, y_b[:, :65].max(1), x_b


def _run_finish(part, bias, w2, b2):
    parts, n, ld = part.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_part, d_bias, d_w2, d_b2 = t(part), t(bias), t(w2), t(b2)
    pr = torch.full((n + PAD, 65), NAN, device="cuda")
    va = torch.full((n + PAD,), NAN, device="cuda")
    nat.check(nat.lib.az_heads_fast_finish_gpu(
        nat.ptr(d_part), ld, parts, nat.ptr(d_bias), nat.ptr(d_w2), nat.ptr(d_b2), nat.ptr(pr),
        nat.ptr(va), n, nat.stream_ptr()), "az_heads_fast_finish_gpu")
    torch.cuda.synchronize()
    pr, va = pr.cpu().numpy(), va.cpu().numpy()
    assert np.isnan(pr[n:]).all() and np.isnan(va[n:]).all()
    return pr[:n], va[:n]


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("ld", [129, 132])
@pytest.mark.parametrize("parts", [1, 3, 4, 8, 16])
def test_heads_fast_finish_kernel_at_peaked_inputs(parts, ld, n, tie):
    part, bias, w2u, b2u, j1, j2 = _finish_case(parts, ld, n, tie, 100 * parts + ld + 7 * n + tie)
    _, x0, _, _ = _finish_reference(part, bias, w2u, b2u)
    if parts > 1:
        assert np.abs(part[:-1]).max() > 1e4  # the cancellation is there
    for target in (0.01, -0.01, 3.0, -3.0, 40.0, -40.0):
        W = {"w2": torch.from_numpy(w2u.copy()), "b2": torch.from_numpy(b2u.copy())}
        ib = _scale_value(W, x0, target, n > 1)
        w2, b2 = W["w2"].numpy(), W["b2"].numpy()
        logits, x, D, Dv = _finish_reference(part, bias, w2, b2)
        assert np.ptp(logits[0]) > 120 and abs(x[ib] / target - 1) < 1e-3
        where = f"parts={parts} ld={ld} n={n} tie={tie} target={target}"
        pr, va = _run_finish(part, bias, w2, b2)
        clear = _check_softmax(pr, logits, D, where)
        _check_values(va, x, Dv, where)
        if tie:
            assert logits[0, j1] == logits[0, j2] == logits[0].max()
            assert (pr[:, j1] == pr[:, j2]).all(), where
        else:
            assert clear.all(), where


# ---- sharpened whole nets ----------------------------------------------------------------
# The module's policy FC scaled by s and its last value FC by t (weights and biases), so that
# the logits of a board spread over about +-60 and about half the values pass |v| = 0.999:
# what training does to a net and random initialisation never shows.

B_NET = 257  # ragged for the four-board and the two-board workgroups


def _sharp_net(kind):
    """(net float32 on the device, its float64 copy on the CPU, planes, s, t, the unsharpened
    float64 outputs)."""
    import copy

    from Models import AlphaZeroNet, FastOthelloNet

    torch.manual_seed(0)
    net = AlphaZeroNet(8, 65, 5, 128) if kind == "az" else FastOthelloNet(8, 65)
    for m in net.modules():  # non-trivial BatchNorm statistics so the folding is exercised
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.5, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.2, 0.2)
    net = net.eval()
    x = torch.randint(-1, 2, (B_NET, 64), generator=torch.Generator().manual_seed(5)).float()
    with torch.no_grad():
        l0, v0 = copy.deepcopy(net).double()(x.double().view(-1, 1, 8, 8))
    l0, pre0 = l0.numpy(), np.arctanh(v0.reshape(-1).numpy())
    s = 120.0 / float(np.median(np.ptp(l0, axis=1)))
    t = float(np.arctanh(0.999)) / float(np.median(np.abs(pre0)))
    pol, val = (net.pol_fc, net.val_fc2) if kind == "az" else (net.fc_policy, net.fc_value2)
    with torch.no_grad():
        for lin, k in ((pol, s), (val, t)):
            lin.weight.mul_(k)
            lin.bias.mul_(k)
    net64 = copy.deepcopy(net).double()
    return net.cuda(), net64, x, s, t, (l0, pre0)


def _ref64(net64, x):
    with torch.no_grad():
        l, v = net64(x.double().view(-1, 1, 8, 8))
    return torch.log_softmax(l, -1).numpy(), v.reshape(-1).numpy()


def _evaluate(fused, x):
    pr = torch.full((B_NET, 65), NAN, device="cuda")
    va = torch.full((B_NET,), NAN, device="cuda")
    with torch.no_grad():
        fused.evaluate_into(x.cuda(), pr, va)
    torch.cuda.synchronize()
    pr, va = pr.cpu().numpy(), va.cpu().numpy()
    assert np.isfinite(pr).all() and (pr >= 0).all() and (np.abs(va) <= 1).all()
    assert (np.abs(pr.astype(np.float64).sum(1) - 1) <= 65 * U).all()
    return pr, va


def _log_err(pr, logp64):
    keep = logp64 > -120 * np.log(2)
    with np.errstate(divide="ignore"):
        return np.abs(np.log(pr.astype(np.float64)) - logp64)[keep].max()


@pytest.mark.parametrize("kind", ["az", "fast"])
def test_sharpened_net_paths_agree_and_are_fp32_accurate(kind, monkeypatch):
    """Every HIP evaluation path of a sharpened net: the paths that share numerics are
    bit-identical (AlphaZeroNet: separate heads, heads fused into the last conv, the persistent
    trunk_heads launch; FastOthelloNet: the one-launch trunk and the three launches), and the
    error against the float64 module is within 2x the float32 torch module's own error plus one
    float32 ulp of the quantity (test_heads_fast_gemm_is_fp32_accurate's margin: the trunk is
    specified as fp32-accurate, and s and t multiply both errors alike).  Log priors above
    2^-120, values in absolute terms."""
    from Models import FusedInferenceNet, inference_copy

    net, net64, x, s, t, _ = _sharp_net(kind)
    logp64, v64 = _ref64(net64, x)
    spread = -logp64.min(1)
    assert np.median(spread) > 100 and 0.3 < (np.abs(v64) > 0.999).mean() < 0.7
    fused = inference_copy(net, "cuda")
    assert fused.precision == "fp16x2"
    out = {}
    if kind == "az":
        for name, fh, th in (("separate", False, False), ("conv", True, False),
                             ("trunk", True, True)):
            monkeypatch.setattr(FusedInferenceNet, "fuse_heads", fh)
            monkeypatch.setattr(FusedInferenceNet, "trunk_heads", th)
            out[name] = _evaluate(fused, x)
    else:
        assert fused._fast_trunk_ready()
        for name, flag in (("fused", True), ("unfused", False)):
            monkeypatch.setattr(FusedInferenceNet, "fuse_fast_trunk", flag)
            out[name] = _evaluate(fused, x)
    first = next(iter(out))
    for name, (pr, va) in out.items():
        assert np.array_equal(pr, out[first][0]) and np.array_equal(va, out[first][1]), name
    pr, va = out[first]
    with torch.no_grad():
        l32, v32 = net(x.cuda().view(-1, 1, 8, 8))
    keep = logp64 > -120 * np.log(2)
    e32_p = np.abs(torch.log_softmax(l32, -1).double().cpu().numpy() - logp64)[keep].max()
    e32_v = np.abs(v32.reshape(-1).double().cpu().numpy() - v64).max()
    e_p, e_v = _log_err(pr, logp64), np.abs(va.astype(np.float64) - v64).max()
    print(f"{kind}: s = {s:.1f}, t = {t:.1f}, log-prior error {e_p:.3g} (torch fp32 {e32_p:.3g}, "
          f"ratio {e_p / e32_p:.2f}), value error {e_v:.3g} (torch fp32 {e32_v:.3g}, "
          f"ratio {e_v / e32_v:.2f})")
    assert e_p <= 2 * e32_p + 2.0 ** -23 * np.abs(logp64[keep]).max()
    assert e_v <= 2 * e32_v + 2.0 ** -23
    sat = np.abs(np.arctanh(np.clip(v64, -1 + 1e-16, 1 - 1e-16))) >= 10.5
    assert (va[sat] == np.sign(v64[sat])).all()


@pytest.mark.parametrize("kind", ["az", "fast"])
def test_sharpened_net_on_the_fp16_trunk(kind, monkeypatch):
    """AlphaZeroNet's fp16 tower runs as one persistent launch with the stem and the heads
    (az_trunk_wino4_heads_fp16_gpu, a third caller of heads_az.h): its priors and values must
    be bit-identical to the per-layer fp16 launches followed by the separate heads kernel.

    Accuracy: the fp16 trunk (fp16 operands, fp32 accumulation and heads) feeds the heads logits that
    are off by fp16 rounding, d_j, and the sharpening multiplies them by s.  Unsharpened, the
    log-prior error of logit j is d_j - sum_i p_i d_i, at most e0 over the batch; sharpened it
    is s (d_j - sum_i p'_i d_i) with other weights p', and |d_j - sum_i p'_i d_i| <=
    max_i |d_j - d_i| <= 2 e0 to first order.  So the sharpened log-prior error is at most
    2 s e0, plus the float32 softmax's own ulp; likewise the value's, with tanh's slope at most
    1, is at most t times the unsharpened pre-tanh error."""
    import copy

    from Models import FusedInferenceNet, inference_copy

    algo = {"conv_algo": "wino4"} if kind == "az" else {}
    net, net64, x, s, t, (l0, pre0) = _sharp_net(kind)
    plain = copy.deepcopy(net)
    pol, val = ((plain.pol_fc, plain.val_fc2) if kind == "az"
                else (plain.fc_policy, plain.fc_value2))
    with torch.no_grad():  # the same net before the scaling
        for lin, k in ((pol, s), (val, t)):
            lin.weight.div_(k)
            lin.bias.div_(k)
    f0 = inference_copy(plain, "cuda", dtype=torch.float16, **algo)
    assert f0.precision == "fp16"
    pr0, va0 = _evaluate(f0, x)
    logp0 = l0 - np.log(np.exp(l0 - l0.max(1, keepdims=True)).sum(1, keepdims=True)) \
        - l0.max(1, keepdims=True)
    e0_p = np.abs(np.log(pr0.astype(np.float64)) - logp0).max()
    e0_v = np.abs(np.arctanh(va0.astype(np.float64)) - pre0).max()
    logp64, v64 = _ref64(net64, x)
    fused = inference_copy(net, "cuda", dtype=torch.float16, **algo)
    pr, va = _evaluate(fused, x)
    if kind == "az":
        assert fused._trunk4_fp16_ready(list(fused.c1), list(fused.c2))  # what just ran
        monkeypatch.setattr(FusedInferenceNet, "trunk_fp16", False)
        assert not fused._trunk4_fp16_ready(list(fused.c1), list(fused.c2))
        lp, lv = _evaluate(fused, x)
        monkeypatch.setattr(FusedInferenceNet, "trunk_fp16", True)
        for _ in range(3):
            pr, va = _evaluate(fused, x)
            assert np.array_equal(pr, lp) and np.array_equal(va, lv)
    e_p, e_v = _log_err(pr, logp64), np.abs(va.astype(np.float64) - v64).max()
    print(f"{kind} fp16: unsharpened log-prior error {e0_p:.3g}, pre-tanh error {e0_v:.3g}; "
          f"sharpened (s = {s:.1f}, t = {t:.1f}) log-prior error {e_p:.3g} = "
          f"{e_p / (s * e0_p):.2f} s e0, value error {e_v:.3g} = {e_v / (t * e0_v):.2f} t e0")
    keep = logp64 > -120 * np.log(2)
    assert e_p <= 2 * s * e0_p + 2.0 ** -23 * np.abs(logp64[keep]).max()
    assert e_v <= t * e0_v + 2.0 ** -23
