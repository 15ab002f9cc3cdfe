"""Generate tests/golden/trunk_bits.npz: the fp16x2 trunk's outputs on the seeded cases of
tests/trunk_cases.py, recorded on an MI355X with the library of the commit BEFORE the
single-issue fp32 forms of csrc/conv_wino4.hip (the input transform's col_comb / combine_kx), so
tests/test_trunk_f32_issue_gpu.py pins every later build to those bits.

    AZ_LIB_PATH=<that commit's libaz_othello.so> python tests/golden/make_trunk_bits.py [out.npz]

Per case (kind, blocks, boards): priors [B, 65] and values [B] in full, the tower output
[B, 128, 8, 8] as the sha256 of its bits (-0 stored as +0), and the recording library's
build id.

The persistent trunk's contract is the per-layer launches' bits (tests/test_nn_gpu.py).  That
commit's persistent trunk broke it at B = 5: board 4, alone in the last workgroup with an
input range >= 64, got NaN into its top-left windows (an off-board window word x coefficient
overflowed before the edge mask's x 0; fixed by combine_kx's column masks in the
coefficients).  Where the recorded trunk
outputs differ from the recorded per-layer ones, the per-layer ones are stored for the trunk
case too and the case is named in `trunk_cases_from_layers`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alphazero-othello_amd"), os.path.dirname(HERE)]

import az_native as nat  # noqa: E402
import trunk_cases as tc  # noqa: E402
from Models import inference_copy  # noqa: E402


def main():
    out = {"build_id": np.array(nat.build_id()), "planes": tc.planes5().numpy()}
    x5 = tc.planes5().cuda()
    for nb in tc.BLOCKS:
        fused = inference_copy(tc.make_net(nb), "cuda")
        assert fused.precision == "fp16x2"
        for kind in tc.KINDS:
            for B in tc.BATCHES:
                pr, va, h = tc.run(fused, x5[:B].contiguous(), kind)
                assert np.isfinite(pr).all() and np.isfinite(va).all() and np.isfinite(h).all()
                out[tc.key(kind, nb, B, "pr")] = pr
                out[tc.key(kind, nb, B, "va")] = va
                out[tc.key(kind, nb, B, "h_sha")] = np.array(tc.bits_sha(h))
    patched = []
    for nb in tc.BLOCKS:
        for B in tc.BATCHES:
            kt, kl = [[tc.key(k, nb, B, w) for w in ("pr", "va", "h_sha")] for k in tc.KINDS]
            if not all(np.array_equal(out[a], out[b]) for a, b in zip(kt, kl)):
                patched.append(f"nb{nb}_B{B}")
                for a, b in zip(kt, kl):
                    out[a] = out[b]
    out["trunk_cases_from_layers"] = np.array(patched)
    print("trunk cases stored from the per-layer outputs:", patched)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "trunk_bits.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays, recorded with build", nat.build_id()[:16])


if __name__ == "__main__":
    main()
