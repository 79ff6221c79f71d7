"""Convert a compressed scene (.npz, GaussianModel.save_npz) to the standard 3DGS PLY that every viewer reads.

    python -m c3dgs_amd.npz2ply FILE.npz [--ply_file OUT.ply]      (default OUT: FILE with the extension .ply)

Same arguments as the reference's npz2ply.py. The model is built for the file: quantisation-aware when the file holds
int8 codes, factor scaling when it has a scaling_factor. The observers keep the ranges the file stores (they are not
updated while the getters run), so the PLY holds exactly the values the .npz decodes to, expanded to dense per-Gaussian
attributes.
"""
import argparse
import os


def convert(npz_file, ply_file=None):
    import numpy as np
    from .model import SLOTS, GaussianModel
    if ply_file is None:
        ply_file = os.path.splitext(npz_file)[0] + ".ply"
    with np.load(npz_file) as sd:
        quantization = bool(sd["quantization"])
        factor = "scaling_factor" in sd
    model = GaussianModel(3, quantization=quantization, use_factor_scaling=factor)
    print(f"loading '{npz_file}'")
    model.load_npz(npz_file)
    for slot in SLOTS:
        model._modules_qa[slot].disable_observer()
    print(f"saving to '{ply_file}'")
    model.save_ply(ply_file)
    print("done")
    return ply_file


def main(argv=None):
    parser = argparse.ArgumentParser("npz2ply", description=__doc__.split("\n")[0])
    parser.add_argument("npz_file", type=str)
    parser.add_argument("--ply_file", type=str, default=None, required=False)
    args = parser.parse_args(argv)
    convert(args.npz_file, args.ply_file)


if __name__ == "__main__":
    main()
