"""Dataset-wide band statistics and the parameter file of norm_mode 'global'.

The reference computes them with st_water_seg/misc/compute_dataset_normalization_parameters.py: per item it gathers the
pixels whose channel mean is not 0 (`:19-24`), keeps 10 % of them (`--subsample_pct`, because the host gather re-copies
everything collected so far with np.concatenate for every item) and takes numpy's float32 mean / std at the end; the result
is pickled as {dset_name: {sensor: {"mean", "std"}}} (`:146-163`), read back by datasets/utils.py:215-230 and applied by
base_dataset.py:91-94.  Here the tiles are already in HBM (TileLoader's raw / window views), so EVERY pixel is streamed
once through the C ABI `fu_band_stats` (one pass, fp64 sums, bit-reproducible) -- no subsampling; that is the one
difference in the numbers, besides fp64 against float32 accumulation.

    python -m floodplanet_code_amd.datasets.stats DATA_ROOT SENSOR [--dataset_name floodplanet] [--channels ALL]
        [--crop_size 512] [--norm_save_path P] [--batch_size N] [--n_workers N] [--device cuda:0] [--device_resize]

builds the data set as the reference's main() does (split 'all', norm_mode None), prints count / mean / std / min / p5 /
p95 / max per band and, with --norm_save_path, merges the parameters into that file.  The percentiles are those of the
whole data set (from a 4096-bin histogram over [0, 1], the range every sensor is scaled to), not the median of per-item
percentiles that misc/compute_input_feature_stats.py prints for the `image` feature.

`BandStats` owns the device accumulators; `band_stats_host` states the same contract in numpy fp64 -- it is what the
tests compare the device against, NOT a fallback: the device path raises without a ROCm GPU."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import pickle
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

MASK_MODES = {None: 0, "nonzero": 1}
MAX_CHANNELS = 16

__all__ = ["BandStats", "band_stats_host", "compute_norm_params", "save_norm_params", "load_norm_params",
           "percentile_from_hist", "finalize"]


# ------------------------------------------------------------------------------------------------------ shared pieces
def finalize(count, total, total_sq):
    """fp64: mean = sum / n, population std = sqrt(max(sumsq / n - mean^2, 0)); NaN where nothing was counted."""
    n = np.asarray(count, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.asarray(total, np.float64) / n
        var = np.asarray(total_sq, np.float64) / n - mean * mean
    return mean, np.sqrt(np.maximum(var, 0.0))


def percentile_from_hist(hist: np.ndarray, q: float, lo: float, hi: float) -> np.ndarray:
    """Per channel, numpy's 'linear' percentile read off an equal-bin histogram [C, n_bins] over [lo, hi]: the rank
    q / 100 * (n - 1) is located in the cumulative counts and placed linearly inside its bin.  It is within one bin width
    of np.percentile on the pixels whenever the two order statistics around that rank fall into the same or neighbouring
    bins (values outside [lo, hi] sit in the edge bins)."""
    hist = np.asarray(hist, dtype=np.int64)
    n_bins = hist.shape[1]
    width = (float(hi) - float(lo)) / n_bins
    out = np.full(hist.shape[0], np.nan)
    for c, h in enumerate(hist):
        n = int(h.sum())
        if n == 0:
            continue
        rank = q / 100.0 * (n - 1)
        cum = np.cumsum(h)
        b = int(np.searchsorted(cum, rank, side="right"))
        b = min(b, n_bins - 1)
        before = int(cum[b - 1]) if b > 0 else 0
        frac = (rank - before + 0.5) / max(int(h[b]), 1)
        out[c] = float(lo) + (b + min(max(frac, 0.0), 1.0)) * width
    return out


def _bin_index(x: np.ndarray, lo: float, hi: float, n_bins: int) -> np.ndarray:
    """The kernel's bin rule in float32: floor((x - lo) * (n_bins / (hi - lo))), clamped to the edge bins."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    scale = np.float32(n_bins) / (hi32 - lo32)
    t = (x.astype(np.float32) - lo32) * scale
    return np.clip(np.floor(t), 0, n_bins - 1).astype(np.int64)


def _as_numpy(s) -> np.ndarray:
    if torch.is_tensor(s):
        s = s.detach().cpu().numpy()
    return np.ascontiguousarray(s, dtype=np.float32)


def band_stats_host(sources: Sequence, valid_hw=None, bins: Optional[int] = 4096,
                    value_range: Tuple[float, float] = (0.0, 1.0), mask: Optional[str] = "nonzero",
                    return_pixels: bool = False) -> dict:
    """The contract of fu_band_stats in numpy: sources fp32 [B, C_k, H, W] side by side along C, valid_hw = (valid_h [B],
    valid_w [B]) or None.  mask None: every pixel of the valid crop; 'nonzero': the fp32 sum, in channel order, of the FIRST
    source's channels is not 0 (the reference's `image.mean(axis=0) != 0`), applied to every source.  A pixel with a NaN /
    Inf in any channel is left out and counted.  -> count, n_nonfinite [C] int64; sum, sumsq, mean, std, min, max [C]
    float64 (std: population); hist [C, bins] int64 (bins None: absent); with return_pixels also pixels [C, n] float32."""
    if mask not in MASK_MODES:
        raise ValueError(f"mask must be None or 'nonzero', got {mask!r}")
    srcs = [_as_numpy(s) for s in sources]
    B, _, H, W = srcs[0].shape
    x = np.concatenate(srcs, axis=1)                                   # [B, C, H, W]
    Cc = x.shape[1]
    vh = np.full(B, H) if valid_hw is None else np.clip(np.asarray(valid_hw[0]).astype(np.int64), 0, H)
    vw = np.full(B, W) if valid_hw is None else np.clip(np.asarray(valid_hw[1]).astype(np.int64), 0, W)
    inside = (np.arange(H)[None, :, None] < vh[:, None, None]) & (np.arange(W)[None, None, :] < vw[:, None, None])
    finite = np.isfinite(x).all(axis=1)
    take = inside & finite
    if mask == "nonzero":
        first = srcs[0]
        with np.errstate(invalid="ignore", over="ignore"):
            m = first[:, 0].copy()
            for c in range(1, first.shape[1]):
                m = m + first[:, c]                                    # float32, channel order
        take &= m != 0
    pix = np.ascontiguousarray(np.transpose(x, (1, 0, 2, 3))[:, take])  # [C, n], batch-major order
    d = pix.astype(np.float64)
    n = pix.shape[1]
    out = {"count": np.full(Cc, n, np.int64), "n_nonfinite": np.full(Cc, int((inside & ~finite).sum()), np.int64),
           "sum": d.sum(axis=1), "sumsq": (d * d).sum(axis=1),
           "min": d.min(axis=1) if n else np.full(Cc, np.inf), "max": d.max(axis=1) if n else np.full(Cc, -np.inf)}
    out["mean"], out["std"] = finalize(out["count"], out["sum"], out["sumsq"])
    if bins is not None:
        idx = _bin_index(pix, value_range[0], value_range[1], int(bins))
        out["hist"] = np.stack([np.bincount(idx[c], minlength=int(bins)) for c in range(Cc)]).astype(np.int64)
    if return_pixels:
        out["pixels"] = pix
    return out


# ------------------------------------------------------------------------------------------------------ device side
class BandStats:
    """Device accumulators of fu_band_stats for `n_channels` channels in all: update() adds a batch, result() finalises on
    the host in fp64.  bins None = no histogram (percentile() then raises)."""

    def __init__(self, n_channels: int, device, bins: Optional[int] = 4096, value_range: Tuple[float, float] = (0.0, 1.0),
                 mask: Optional[str] = "nonzero"):
        if mask not in MASK_MODES:
            raise ValueError(f"mask must be None or 'nonzero', got {mask!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BandStats runs fu_band_stats on a ROCm GPU; there is no CPU fallback "
                               "(band_stats_host states the contract in numpy)")
        from .. import _lib
        self.n_channels, self.bins, self.mask = int(n_channels), (None if bins is None else int(bins)), mask
        self.lo, self.hi = float(value_range[0]), float(value_range[1])
        dev, Cc = self.device, self.n_channels
        self.count = torch.zeros(Cc, dtype=torch.int64, device=dev)
        self.n_nonfinite = torch.zeros(Cc, dtype=torch.int64, device=dev)
        self.sum = torch.zeros(Cc, dtype=torch.float64, device=dev)
        self.sumsq = torch.zeros(Cc, dtype=torch.float64, device=dev)
        self.vmin = torch.full((Cc,), float("inf"), dtype=torch.float32, device=dev)
        self.vmax = torch.full((Cc,), float("-inf"), dtype=torch.float32, device=dev)
        self.hist = None if self.bins is None else torch.zeros(Cc, self.bins, dtype=torch.int64, device=dev)
        nbytes = int(_lib.load().fu_band_stats_workspace_bytes(Cc, self.bins or 0))
        self._workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        self._acc = _lib.FuBandAccum(self.count.data_ptr(), self.sum.data_ptr(), self.sumsq.data_ptr(),
                                     self.vmin.data_ptr(), self.vmax.data_ptr(), self.n_nonfinite.data_ptr(),
                                     None if self.hist is None else self.hist.data_ptr(), self.bins or 0, self.lo, self.hi)

    def update(self, sources: Sequence[torch.Tensor], valid_hw=None) -> "BandStats":
        """sources: fp32 NCHW [B, C_k, H, W] on the device (sum C_k = n_channels); valid_hw = (valid_h, valid_w) [B]."""
        from .. import _lib
        if torch.is_tensor(sources):
            sources = [sources]
        dev = self.device
        srcs = [s.to(dev).contiguous().float() for s in sources]
        B, _, H, W = srcs[0].shape
        for s in srcs:
            if s.dim() != 4 or s.shape[0] != B or tuple(s.shape[2:]) != (H, W):
                raise ValueError("all sources must be [B, C_k, H, W] with one batch and tile size")
        if sum(s.shape[1] for s in srcs) != self.n_channels:
            raise ValueError(f"sources hold {sum(s.shape[1] for s in srcs)} channels, the accumulators {self.n_channels}")
        vh = vw = None
        if valid_hw is not None:
            vh, vw = (torch.as_tensor(t).to(dev).to(torch.int32).contiguous() for t in valid_hw)
        arr = (C.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
        chs = (C.c_int32 * len(srcs))(*[s.shape[1] for s in srcs])
        _lib.check(_lib.load().fu_band_stats(arr, chs, len(srcs), B, H, W, _lib.ptr(vh), _lib.ptr(vw),
                                             MASK_MODES[self.mask], C.byref(self._acc), self._workspace.data_ptr(),
                                             self._workspace.numel(), torch.cuda.current_stream(dev).cuda_stream))
        return self

    def state_bytes(self) -> bytes:
        """Every accumulator, byte for byte (one device-to-host read each): equal bytes = bit-identical statistics."""
        parts = [self.count, self.n_nonfinite, self.sum, self.sumsq, self.vmin, self.vmax]
        if self.hist is not None:
            parts.append(self.hist)
        return b"".join(t.cpu().numpy().tobytes() for t in parts)

    def result(self) -> Dict[str, np.ndarray]:
        """count, mean, std (population), min, max, n_nonfinite per channel as float64 numpy (+ sum, sumsq)."""
        count = self.count.cpu().numpy()
        total, total_sq = self.sum.cpu().numpy(), self.sumsq.cpu().numpy()
        mean, std = finalize(count, total, total_sq)
        return {"count": count.astype(np.float64), "mean": mean, "std": std,
                "min": self.vmin.cpu().numpy().astype(np.float64), "max": self.vmax.cpu().numpy().astype(np.float64),
                "n_nonfinite": self.n_nonfinite.cpu().numpy().astype(np.float64), "sum": total, "sumsq": total_sq}

    def histogram(self) -> np.ndarray:
        if self.hist is None:
            raise RuntimeError("BandStats was built without a histogram (bins=None)")
        return self.hist.cpu().numpy()

    def percentile(self, q: float) -> np.ndarray:
        return percentile_from_hist(self.histogram(), q, self.lo, self.hi)


def compute_norm_params(dataset, device, batch_size: int = 16, num_workers: int = 0, device_resize: bool = False,
                        return_stats: bool = False):
    """{dataset.sensor: {"mean": float64 [C], "std": float64 [C]}} over EVERY unmasked pixel of every example of `dataset`
    (a FloodplanetTiles): the raw crops -- or, with device_resize, the source windows resampled on the device -- go to HBM
    batch by batch as TileLoader ships them and through BandStats(mask='nonzero').  No subsampling (module docstring)."""
    from .assemble import resize_lanczos4_tiles
    from .floodplanet import RawTileView, WindowTileView, collate_raw_tiles, collate_window_tiles
    dev = torch.device(device)
    view, coll = (WindowTileView, collate_window_tiles) if device_resize else (RawTileView, collate_raw_tiles)
    dl = torch.utils.data.DataLoader(view(dataset), batch_size=batch_size, shuffle=False, num_workers=num_workers,
                                     collate_fn=coll, pin_memory=dev.type == "cuda")
    stats = BandStats(dataset.n_channels["ms_image"], dev, mask="nonzero")
    for batch in dl:
        if device_resize:
            raw = resize_lanczos4_tiles(*(batch[k].to(dev, non_blocking=True) for k in ("window", "iy", "wy", "ix", "wx")),
                                        batch["scale_mode"])
        else:
            raw = batch["raw"].to(dev, non_blocking=True)
        stats.update([raw], (batch["valid_h"], batch["valid_w"]))
    r = stats.result()
    params = {dataset.sensor: {"mean": r["mean"], "std": r["std"]}}
    return (params, stats) if return_stats else params


# ------------------------------------------------------------------------------------------------------ parameter file
def save_norm_params(path: str, dset_name: str, params: dict) -> dict:
    """Merge {sensor: {"mean", "std"}} into the pickle at `path` under `dset_name`, as the reference's main() does
    (compute_dataset_normalization_parameters.py:146-163: the data set's entry is replaced, other data sets stay)."""
    all_params = {}
    if os.path.exists(path):
        with open(path, "rb") as fh:
            all_params = pickle.load(fh)
    all_params[dset_name] = {k: {"mean": np.asarray(v["mean"], dtype=np.float64), "std": np.asarray(v["std"], dtype=np.float64)}
                             for k, v in params.items()}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        pickle.dump(all_params, fh)
    return all_params


def load_norm_params(path_or_dict, dset_name: str) -> dict:
    """{input type: {"mean": ndarray, "std": ndarray}} of `dset_name` from the reference's parameter file (or from the
    dict such a file holds), datasets/utils.py:215-230."""
    if isinstance(path_or_dict, dict):
        all_params = path_or_dict
    else:
        with open(os.fspath(path_or_dict), "rb") as fh:
            all_params = pickle.load(fh)
    if dset_name not in all_params:
        raise KeyError(f'Normalization parameters is not available for dataset name "{dset_name}"')
    return all_params[dset_name]


def sensor_norm_params(path_or_dict, dset_name: str, sensor: str, n_channels: int):
    """(mean, std) float64 [n_channels] of one sensor; other keys of the file (dem, slope, ...) are ignored."""
    params = load_norm_params(path_or_dict, dset_name)
    if sensor not in params:
        raise KeyError(f'no normalization parameters for sensor "{sensor}" of dataset "{dset_name}" '
                       f"(the file has {sorted(params)})")
    mean = np.asarray(params[sensor]["mean"], dtype=np.float64).reshape(-1)
    std = np.asarray(params[sensor]["std"], dtype=np.float64).reshape(-1)
    if len(mean) != n_channels or len(std) != n_channels:
        raise ValueError(f'normalization parameters of "{sensor}" have {len(mean)} means / {len(std)} stds, the input has '
                         f"{n_channels} channels")
    return mean, std


# ------------------------------------------------------------------------------------------------------ command line
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Dataset-wide band statistics / norm_mode 'global' parameters on the GPU.")
    ap.add_argument("data_root", type=str, help="directory that holds CSDAP_complete/")
    ap.add_argument("sensor_name", type=str, help="S1, S2, PS or L8")
    ap.add_argument("--dataset_name", type=str, default="floodplanet")
    ap.add_argument("--channels", type=str, default="ALL")
    ap.add_argument("--crop_size", type=int, default=512, help="height and width (and stride) of the loaded crops")
    ap.add_argument("--norm_save_path", type=str, default=None, help="merge the parameters into this pickle")
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--n_workers", type=int, default=0)
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--device_resize", action="store_true", help="resample the tiles on the device as well")
    return ap


def main(argv=None) -> None:
    from .floodplanet import FloodplanetTiles
    from .tiles import generate_image_slice_object
    args = build_parser().parse_args(argv)
    sp = generate_image_slice_object(args.crop_size, args.crop_size, args.crop_size)
    ds = FloodplanetTiles(args.data_root, "all", sp, sensor=args.sensor_name, channels=args.channels,
                          dset_name=args.dataset_name, norm_mode=None)
    params, stats = compute_norm_params(ds, args.device, args.batch_size, args.n_workers, args.device_resize,
                                        return_stats=True)
    r, p5, p95 = stats.result(), stats.percentile(5), stats.percentile(95)
    print(f"{args.dataset_name} / {args.sensor_name}: {len(ds)} crops, {int(r['n_nonfinite'][0])} non-finite pixels left out")
    print(f"{'band':>4} {'count':>12} {'mean':>12} {'std':>12} {'min':>12} {'p5':>12} {'p95':>12} {'max':>12}")
    for c in range(stats.n_channels):
        print(f"{c:>4} {int(r['count'][c]):>12} {r['mean'][c]:>12.6g} {r['std'][c]:>12.6g} {r['min'][c]:>12.6g} "
              f"{p5[c]:>12.6g} {p95[c]:>12.6g} {r['max'][c]:>12.6g}")
    if args.norm_save_path:
        save_norm_params(args.norm_save_path, args.dataset_name, params)
        print(f"saved to {args.norm_save_path}")


if __name__ == "__main__":
    main()
