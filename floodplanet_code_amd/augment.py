"""On-GPU tile augmentation: the hflip / vflip / rotate transforms of the reference's BaseDataset
(st_water_seg/datasets/base_dataset.py:494-555, driven by conf/config.yaml:41-52) applied to a whole batch that is
already resident in HBM, instead of per item in DataLoader workers.

``sample_transforms`` mirrors the reference's draws (one uniform coin per transform, uniform angle); ``apply``
runs the single HIP gather kernel behind ``fu_augment`` on image and target together."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

HFLIP, VFLIP, ROTATE = 1, 2, 4


def sample_transforms(batch_size: int, cfg: Optional[dict] = None,
                      rng: Optional[np.random.RandomState] = None) -> Tuple[np.ndarray, np.ndarray]:
    """flags int32 [B], angles float32 [B] drawn like BaseDataset.sample_transforms (defaults: conf/config.yaml:41-52)."""
    rng = rng or np.random
    cfg = cfg or {}
    h = cfg.get("hflip", {"active": True, "likelihood": 0.5})
    v = cfg.get("vflip", {"active": True, "likelihood": 0.5})
    r = cfg.get("rotate", {"active": True, "likelihood": 0.5, "min_rot_angle": 0, "max_rot_angle": 360})
    flags = np.zeros(batch_size, dtype=np.int32)
    angles = np.zeros(batch_size, dtype=np.float32)
    for b in range(batch_size):
        if h.get("active") and rng.rand() < h["likelihood"]:
            flags[b] |= HFLIP
        if v.get("active") and rng.rand() < v["likelihood"]:
            flags[b] |= VFLIP
        if r.get("active") and rng.rand() < r["likelihood"]:
            flags[b] |= ROTATE
            angles[b] = rng.uniform(r["min_rot_angle"], r["max_rot_angle"], size=1)[0]
    return flags, angles


# ------------------------------------------------------------------------------------------------- radiometric part
# The numpy statements of the radiometric part of fu_scene_train_tiles_ex (include/floodunet.h).  They are the
# specification the device is compared against bit for bit, NOT a fallback for it.
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF
NOISE_K = np.float32(1.0 / np.sqrt(32.0 * (65536.0 ** 2 - 1.0) / 12.0))      # 9.344062e-06
PHOTOMETRIC_KEYS = ("gain", "band_gain", "brightness", "noise", "band_drop", "likelihood")


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123): counter = four uint32 values or arrays (broadcast together), key = two uint32 values
    -> the four uint32 output words, arrays of the broadcast shape."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(_M32) for v in np.broadcast_arrays(*[np.asarray(v) for v in counter])]
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]              # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(_M32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(_M32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return tuple(v.astype(np.uint32) for v in c)


def noise_host(H: int, W: int, C: int, noise_key: int, noise_stream: int) -> np.ndarray:
    """The unit-variance draws of one sample: float32 [C, H, W].  Counter = (oy * W + ox, channel, low and high word of
    noise_stream), key = (low, high word of noise_key); S = the sum of the eight 16-bit halves of the four output words;
    z = float32(2 * S - 524280) * NOISE_K -- the integer is below 2^24, so the convert is exact."""
    key, stream = int(noise_key) & (2 ** 64 - 1), int(noise_stream) & (2 ** 64 - 1)
    pixel = np.arange(H * W, dtype=np.uint32).reshape(1, H, W)
    channel = np.arange(C, dtype=np.uint32).reshape(C, 1, 1)
    words = philox4x32_10((pixel, channel, stream & _M32, stream >> 32), (key & _M32, key >> 32))
    S = np.zeros((C, H, W), dtype=np.int64)
    for w in words:
        S += (w & np.uint32(0xFFFF)).astype(np.int64) + (w >> np.uint32(16)).astype(np.int64)
    return (2 * S - 524280).astype(np.float32) * NOISE_K


def _term(v, n: int, C: int, name: str):
    if v is None:
        return None
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    if a.size != n * C:
        raise ValueError(f"photometric {name}: {a.size} values for {n} samples of {C} channels")
    return a.reshape(n, C)


def photometric_host(image, gain, bias, sigma, noise_key: int = 0, noise_stream=None) -> np.ndarray:
    """image float32 [n, C, H, W] (the normalised batch) -> t = v * gain; t = t + bias; t = t + sigma * z at EVERY pixel,
    each operation rounded on its own in float32; gain / bias / sigma: [n, C] (or flat [n * C]) or None = that term is
    skipped.  The device applies it to the pixels that come from the scene only (pad pixels and rotation corners stay):
    the caller selects those."""
    t = np.array(image, dtype=np.float32, copy=True)
    n, C, H, W = t.shape
    gain, bias, sigma = (_term(v, n, C, k) for v, k in ((gain, "gain"), (bias, "bias"), (sigma, "sigma")))
    if gain is not None:
        t = t * gain[:, :, None, None]
    if bias is not None:
        t = t + bias[:, :, None, None]
    if sigma is not None:
        if noise_stream is None or len(noise_stream) != n:
            raise ValueError("photometric sigma needs one noise_stream per sample")
        for b in range(n):
            e = sigma[b][:, None, None] * noise_host(H, W, C, noise_key, int(noise_stream[b]))
            t[b] = t[b] + e
    return t


def check_photometric(cfg: Optional[dict], spoken_as: str = "photometric"):
    """sample_photometric's config, checked without a draw: -> (active, (gain, band_gain, brightness, noise, band_drop,
    likelihood)) as floats, the defaults for what the config leaves out.  ValueError for a key that is not one of
    PHOTOMETRIC_KEYS (or `active`) and for a value outside its range; spoken_as opens the message (the command line says
    "--aug_*")."""
    cfg = dict(cfg or {})
    active = cfg.pop("active", True)
    unknown = sorted(set(cfg) - set(PHOTOMETRIC_KEYS))
    if unknown:
        raise ValueError(f"{spoken_as}: unknown keys {unknown} (known: {list(PHOTOMETRIC_KEYS)})")
    G, Gb, B, S, P = (float(cfg.get(k, 0.0)) for k in ("gain", "band_gain", "brightness", "noise", "band_drop"))
    L = float(cfg.get("likelihood", 1.0))
    if not (0.0 <= G <= 1.0 and 0.0 <= Gb <= 1.0 and B >= 0.0 and S >= 0.0 and 0.0 <= P < 1.0 and 0.0 <= L <= 1.0):
        raise ValueError(f"{spoken_as}: need 0 <= gain, band_gain <= 1, brightness, noise >= 0, 0 <= band_drop < 1 and "
                         f"0 <= likelihood <= 1, got {cfg}")
    return active, (G, Gb, B, S, P, L)


def sample_photometric(n: int, C: int, cfg: Optional[dict], rng: np.random.RandomState) -> Optional[dict]:
    """The radiometric draws of n samples of C bands from a config dict, in units of the batch the net sees (after
    normalisation): `gain` G -- one factor per sample, uniform in [1 - G, 1 + G]; `band_gain` Gb -- one more factor per
    band, uniform in [1 - Gb, 1 + Gb]; `brightness` B -- one bias per sample, uniform in [-B, B]; `noise` S -- sigma per
    sample, uniform in [0, S]; `band_drop` P -- each band independently gets gain = bias = sigma = 0 with probability P,
    never all bands of a sample (the band with the largest draw stays); `likelihood` L (default 1) -- one coin per sample
    for the whole group: a sample that loses it keeps gain 1, bias 0, sigma 0.  Every draw is made whatever the values, in
    a fixed order, so one option does not move another's stream.  -> {"gain", "bias", "sigma"}: float32 [n, C] each, or
    None for a term the config cannot move; None when the group is inactive ({"active": False}, or nothing to vary)."""
    active, (G, Gb, B, S, P, L) = check_photometric(cfg)
    if not active or (G == 0.0 and Gb == 0.0 and B == 0.0 and S == 0.0 and P == 0.0) or L == 0.0:
        return None
    on = rng.rand(n) < L
    g = rng.uniform(1.0 - G, 1.0 + G, size=n)
    gb = rng.uniform(1.0 - Gb, 1.0 + Gb, size=(n, C))
    b = rng.uniform(-B, B, size=n)
    s = rng.uniform(0.0, S, size=n)
    u = rng.rand(n, C)
    drop = u < P
    drop[np.arange(n), np.argmax(u, axis=1)] &= ~drop.all(axis=1)        # never every band of a sample
    keep = ~(drop & on[:, None])
    gain = np.where(on[:, None], g[:, None] * gb, 1.0) * keep
    bias = np.where(on, b, 0.0)[:, None] * keep
    sigma = np.where(on, s, 0.0)[:, None] * keep
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"gain": f32(gain) if (G or Gb or P) else None, "bias": f32(bias) if B else None,
            "sigma": f32(sigma) if S else None}


def apply(image: torch.Tensor, target: Optional[torch.Tensor], flags, angles, target_fill: int = 0):
    """image f32 [B,C,H,W] and target i64 [B,H,W] on a ROCm device -> augmented copies."""
    if image.device.type != "cuda":
        raise RuntimeError("augment.apply runs only on a ROCm GPU; there is no CPU fallback")
    image = image.contiguous().float()
    B, C, H, W = image.shape
    dev = image.device
    f = torch.as_tensor(np.asarray(flags, dtype=np.int32), device=dev)
    a = torch.as_tensor(np.asarray(angles, dtype=np.float32), device=dev)
    out = torch.empty_like(image)
    tgt = target.contiguous().long() if target is not None else None
    tout = torch.empty_like(tgt) if tgt is not None else None
    check(_lib.load().fu_augment(ptr(image), ptr(tgt), ptr(out), ptr(tout), ptr(f), ptr(a), B, C, H, W,
                                 int(target_fill), torch.cuda.current_stream(dev).cuda_stream))
    return out, tout
