"""Record what a build's decode attention kernel computes for the cases of
tests/decode_golden_cases.py, as the fixtures tests/test_decode_lds_gpu.py
compares later builds with.

Run it on a GPU against the build whose bytes are the reference (a checkout
of the parent commit, built, first on PYTHONPATH):

    PYTHONPATH=<parent checkout> python scripts/record_decode_golden.py \
        --out tests/golden/decode_parent

It imports kubeai_amd from PYTHONPATH if it is there and from this checkout
otherwise, and prints which one it took.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))

import decode_golden_cases as cases  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden",
                                                 "decode_parent"))
    args = p.parse_args()
    import kubeai_amd
    import kubeai_amd.ops as ops

    assert ops.have_hip_ext(), "needs the built HIP extension"
    print("recording from", os.path.dirname(kubeai_amd.__file__))
    os.makedirs(args.out, exist_ok=True)
    total = 0
    for name, c in cases.CASES.items():
        inp = cases.build_inputs(name, "cuda")
        for raw, fp8_out in c["variants"]:
            sections, _, _ = cases.run_variant(ops, inp, raw, fp8_out)
            arr = cases.pack(sections)
            path = os.path.join(
                args.out, f"{name}_{cases.variant_name(raw, fp8_out)}.npy"
            )
            np.save(path, arr)
            total += os.path.getsize(path)
            print(f"{path}: {arr.size} bytes")
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
