"""Writes tests/golden/tiff/: small TIFFs encoded by PIL's libtiff -- an encoder that is not ours -- and expected.npz with
the arrays they hold.  Needs PIL built with libtiff; reading the fixtures (tests/test_geotiff_cpu.py) needs neither.

    python tests/tools/make_geotiff_fixtures.py

PIL's writer drops the tile tags (322 / 323), so it cannot produce a tiled file; tiles are covered the other way round,
by PIL's libtiff decoding the files of tests/tools/geotiff_writer.py."""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "tiff")
H, W = 61, 83


def arrays():
    g = np.random.default_rng(20)
    yy, xx = np.mgrid[:H, :W]
    ramp = (yy * 3 + xx * 5).astype(np.int64)
    u8 = ((ramp // 4 + g.integers(0, 3, (H, W))) % 256).astype(np.uint8)
    flat = np.where((yy // 9 + xx // 14) % 2 == 0, 17, 200).astype(np.uint8)       # long runs for PackBits
    u16 = ((ramp * 97 + g.integers(0, 40, (H, W))) % 65536).astype(np.uint16)      # wraps more than once
    f32 = (np.sin(yy / 7.0) * np.cos(xx / 5.0) * 40 - 20).astype(np.float32)
    f32[3, 4], f32[5, 6], f32[7, 8], f32[9, 10] = np.nan, np.inf, -np.inf, np.float32(1e-41)
    return {"lzw_u8": (u8, "tiff_lzw", None), "deflate_u16": (u16, "tiff_adobe_deflate", None),
            "packbits_u8": (flat, "packbits", None), "lzw_p2_u16": (u16, "tiff_lzw", 2),
            "deflate_p3_f32": (f32, "tiff_adobe_deflate", 3)}


def main():
    from PIL import Image, features
    assert features.check("libtiff"), "PIL without libtiff cannot write compressed TIFFs"
    os.makedirs(OUT, exist_ok=True)
    expected = {}
    for name, (a, compression, predictor) in arrays().items():
        path = os.path.join(OUT, name + ".tif")
        Image.fromarray(a).save(path, compression=compression, **({"tiffinfo": {317: predictor}} if predictor else {}))
        back = Image.open(path)
        assert back.tag_v2.get(317, 1) == (predictor or 1), (name, back.tag_v2.get(317))
        assert np.array_equal(np.array(back), a, equal_nan=a.dtype.kind == "f"), name
        expected[name] = a
        print(f"{name}: {os.path.getsize(path)} bytes")
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)


if __name__ == "__main__":
    main()
