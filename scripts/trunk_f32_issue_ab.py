"""A/B of builds of libaz_othello.so on the leaf-evaluation launches, all in one process on one
device, the builds interleaved round by round, their order rotating from round to round
(profiles/trunk_f32_issue_ab.json):
    python scripts/trunk_f32_issue_ab.py [--rounds 5] [--boards 1024] name=path [name=path ...]
Each build is loaded with ctypes beside the others and swapped in as az_native.lib; the weights
are prepared once (the prepared layout is the same in every build).  Per build and round, after
`--warm` untimed launches, the mean of `--reps` launches (one device event pair around them):
  trunk_fp16x2  az_trunk_wino4_heads_gpu, AlphaZeroNet 5 x 128 (configs[2]'s evaluation)
  trunk_fp16    az_trunk_wino4_heads_fp16_gpu (configs[4]'s fp16 inference)
  conv_fp16x2   one az_conv3x3_wino4_gpu launch with a residual (the per-layer kernel)
and the sha256 of priors / values / conv output, so equal results show as equal digests.
The first named build is the baseline of the summary: median and min per build, the baseline's
round-to-round range, and whether a build's median gain exceeds three times that range."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd")]
import az_native as nat  # noqa: E402
from Models import AlphaZeroNet, board_absmax, inference_copy  # noqa: E402


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("az_last_error", "az_build_id"):
        getattr(lib, name).argtypes = []
        getattr(lib, name).restype = ctypes.c_char_p
    for name, args in nat.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    lib.az_conv3x3_wino_prep_bytes.restype = ctypes.c_int64
    lib.az_conv3x3_mx_prep_bytes.restype = ctypes.c_int64
    return lib


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us per launch


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--boards", type=int, default=1024)
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    libs = {}
    for spec in a.libs:
        name, path = spec.split("=", 1)
        libs[name] = load(path)
    B = a.boards
    torch.manual_seed(0)
    net = AlphaZeroNet(8, 65, 5, 128).cuda().eval()
    os.environ["AZ_CONV_ALGO"] = "wino4"  # the fp16 net on the persistent trunk too
    nets = {"trunk_fp16x2": inference_copy(net, "cuda"),
            "trunk_fp16": inference_copy(net, "cuda", precision="fp16")}
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randint(-1, 2, (B, 64), generator=g).float().cuda()
    pr = torch.empty(B, 65, device="cuda")
    va = torch.empty(B, device="cuda")
    # the per-layer conv: one residual layer of the fp16x2 net on post-ReLU inputs
    conv = nets["trunk_fp16x2"].c2[0]
    cx = torch.randn(B, 128, 8, 8, generator=g).relu().cuda().contiguous(memory_format=torch.channels_last)
    cr = torch.randn(B, 128, 8, 8, generator=g).relu().cuda().contiguous(memory_format=torch.channels_last)
    cy = torch.empty_like(cx, memory_format=torch.channels_last)
    amax = board_absmax(cx)
    work, oamax = amax.clone(), torch.zeros_like(amax)

    def run_net(k):
        with torch.no_grad():
            nets[k].evaluate_into(x, pr, va)

    def run_conv():
        work.copy_(amax)  # in_absmax is consumed by the launch
        nat.check(nat.lib.az_conv3x3_wino4_gpu(
            nat.ptr(cx), nat.ptr(conv.wq), nat.ptr(conv.bias), nat.ptr(cr), nat.ptr(cy), B, 128, 1,
            conv.mode, nat.ptr(work), nat.ptr(oamax), nat.stream_ptr()), "az_conv3x3_wino4_gpu")

    cases = {"trunk_fp16x2": lambda: run_net("trunk_fp16x2"), "trunk_fp16": lambda: run_net("trunk_fp16"),
             "conv_fp16x2": run_conv}
    out = {"boards": B, "rounds": a.rounds, "warm": a.warm, "reps": a.reps,
           "device": torch.cuda.get_device_name(0),
           "builds": {n: {"path": dict(s.split("=", 1) for s in a.libs)[n],
                          "build_id": libs[n].az_build_id().decode()} for n in libs},
           "us_per_launch": {c: {n: [] for n in libs} for c in cases}, "sha": {c: {} for c in cases}}
    names = list(libs)
    for r in range(a.rounds):
        for c, fn in cases.items():
            for n in names[r % len(names):] + names[:r % len(names)]:  # the order rotates by round
                nat.lib = libs[n]
                out["us_per_launch"][c][n].append(round(timed(fn, a.warm, a.reps), 2))
                out["sha"][c][n] = sha(cy) if c == "conv_fp16x2" else sha(pr, va)
    base = next(iter(libs))
    out["summary"] = {}
    for c in cases:
        t = out["us_per_launch"][c]
        rng = max(t[base]) - min(t[base])
        out["summary"][c] = {
            "baseline": base, "baseline_round_range_us": round(rng, 2),
            **{n: {"median_us": round(statistics.median(v), 2), "min_us": min(v),
                   "median_gain_us": round(statistics.median(t[base]) - statistics.median(v), 2),
                   "gain_over_3x_baseline_range": statistics.median(t[base]) - statistics.median(v) > 3 * rng,
                   "same_bits_as_baseline": out["sha"][c][n] == out["sha"][c][base]}
               for n, v in t.items()}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
