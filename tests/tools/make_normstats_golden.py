"""Fixture for the dataset-wide band statistics (TEST INFRASTRUCTURE; needs a checkout of the reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/tools/make_normstats_golden.py <reference checkout>

The reference's `compute_dataset_normalization_parameters` (st_water_seg/misc/compute_dataset_normalization_parameters.py:
12-91) lives in a module that imports tqdm and the whole dataset package, so the one function is compiled out of the
file's syntax tree (as oracle/make_assemble_golden.py does with BaseDataset's methods) and run on a stub data set.  Two
facts about it shape the stub: it only runs with dataset.dem and dataset.slope both true (`dem_pixels` / `slope_pixels`
are unbound otherwise), and it draws with np.random.choice(..., replace=False) -- so the stub carries dem and slope planes
and the function is called with subsample_pct = 1.0, which takes every unmasked pixel, in permuted order.

-> tests/golden/loader_normstats_golden.npz (the loader_ prefix keeps it out of the training-step fixture list): the inputs (12 tiles of 3 + 1 + 1 bands, 64 x 64, values k / 4096 stored as uint16 k;
zero padding outside each tile's valid crop and a few zero pixels inside), the reference's means / stds (image, dem,
slope) and numpy's fp64 values over the same pixels."""
import ast
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "loader_normstats_golden.npz")
REL = os.path.join("st_water_seg", "misc", "compute_dataset_normalization_parameters.py")
VALID = [(64, 64)] * 5 + [(64, 40), (37, 64), (37, 45), (20, 64), (64, 13), (50, 50), (1, 64)]
Q = 4096


def load_function(path, name):
    tree = ast.parse(open(path).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(fns) == 1
    ns = {"np": np, "tqdm": lambda it: it}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def make_inputs(seed=20):
    g = np.random.default_rng(seed)
    n = len(VALID)
    image = np.round((0.15 + 0.7 * g.random((n, 3, 64, 64))) * Q).astype(np.uint16)           # mean ~0.5, std ~0.2
    image[:, 1] = np.round((0.05 + 0.5 * g.random((n, 64, 64)) ** 2) * Q).astype(np.uint16)   # a skewed band
    dem = np.round((0.1 + 0.8 * g.random((n, 1, 64, 64))) * Q).astype(np.uint16)
    slope = np.round((0.02 + 0.9 * g.random((n, 1, 64, 64)) ** 3) * Q).astype(np.uint16)
    for b, (h, w) in enumerate(VALID):                      # zero padding of edge crops (the image only: the auxiliary
        image[b, :, h:, :] = 0                              # planes keep values there, the image's mask leaves them out)
        image[b, :, :, w:] = 0
    holes = g.integers(0, 64, size=(40, 3))
    for b, y, x in holes:                                   # no-data pixels inside the crops
        image[b % n, :, y, x] = 0
    return image, dem, slope


class Stub:
    dem = slope = True
    sensor = "S1"

    def __init__(self, image, dem, slope):
        self.arrays = [(a.astype(np.float32) / np.float32(Q)) for a in (image, dem, slope)]

    def __len__(self):
        return self.arrays[0].shape[0]

    def __getitem__(self, i):
        return {"image": self.arrays[0][i], "dem": self.arrays[1][i], "slope": self.arrays[2][i]}


def main():
    ref_root = sys.argv[1]
    fn = load_function(os.path.join(ref_root, REL), "compute_dataset_normalization_parameters")
    image, dem, slope = make_inputs()
    stub = Stub(image, dem, slope)
    np.random.seed(0)
    ref = fn(stub, 1.0)
    x = np.concatenate(stub.arrays, axis=1)                              # [n, 5, 64, 64]
    mask = stub.arrays[0].mean(axis=1) != 0                              # the function's own rule, per item
    pix = np.transpose(x, (1, 0, 2, 3))[:, mask].astype(np.float64)      # [5, n_pixels]
    out = dict(image_q=image, dem_q=dem, slope_q=slope, q=np.int64(Q),
               valid_h=np.array([v[0] for v in VALID], np.int32), valid_w=np.array([v[1] for v in VALID], np.int32),
               ref_mean=np.concatenate([np.asarray(ref[k]["mean"], np.float64).reshape(-1) for k in ("S1", "dem", "slope")]),
               ref_std=np.concatenate([np.asarray(ref[k]["std"], np.float64).reshape(-1) for k in ("S1", "dem", "slope")]),
               f64_count=np.int64(pix.shape[1]), f64_mean=pix.mean(axis=1), f64_std=pix.std(axis=1),
               f64_min=pix.min(axis=1), f64_max=pix.max(axis=1))
    np.savez_compressed(OUT, **out)
    print("pixels", pix.shape[1], "mean", out["f64_mean"], "std", out["f64_std"])
    print("ref vs f64 mean", np.abs(out["ref_mean"] / out["f64_mean"] - 1).max(), "std",
          np.abs(out["ref_std"] / out["f64_std"] - 1).max(), "bytes", os.path.getsize(OUT))


if __name__ == "__main__":
    main()
