"""GPU: radiometric and zoom augmentation inside the fused scene-tile kernel (fu_scene_train_tiles_ex) against the numpy
statements (augment.photometric_host, sampling.zoom_tile_host) composed with the kernels it extends, bit for bit; the
rejections; SceneTileLoader's photometric / zoom options."""
import ctypes

import numpy as np
import pytest
import torch

from floodplanet_code_amd import _lib, augment
from floodplanet_code_amd.datasets import FloodplanetTiles, SceneTileLoader, generate_image_slice_object, sampling
from floodplanet_code_amd.datasets.assemble import scene_crops, scene_train_tiles
from floodplanet_code_amd.unet import HipUNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_ = 3
N = 6
TILES = [(20, 24), (19, 21)]                     # 16-byte stores / element-wise stores
NORMS = [None, "local", "global"]
SCENE_SIZES = ((50, 60), (47, 61))
FLAGS = [0, 1, 2, 4, 7, 0]                       # none, hflip, vflip, rotate, all three, none (the edge box)
ANGLES = [0.0, 0.0, 0.0, 37.0, 37.0, 0.0]
PAD, NODATA, FILL = -3.0, 2, 5
KEY = 0xC0FFEE1234567890
STREAMS = np.array([11, (7 << 32) + 3, 11, 2 ** 63 + 5, 0, 12345678901234], dtype=np.uint64)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                      b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def net():
    net = HipUNet(2, 3, base_channels=8).to(DEV).eval()
    net._get_ctx(torch.device(DEV), 1, 32, 32)
    return net                                   # keep the module alive: it owns the context


@pytest.fixture(scope="module")
def scenes():
    """(scenes on the device, raw label rasters on the device): labels hold 0, 1, 2 and a stray value."""
    g = torch.Generator().manual_seed(4)
    out_s, out_l = [], []
    for h, w in SCENE_SIZES:
        out_s.append((torch.rand(C_, h, w, generator=g) * 5 - 1).to(DEV))
        lab = torch.randint(0, 3, (h, w), generator=g, dtype=torch.uint8)
        lab[h // 2, w // 3] = 7
        out_l.append(lab.to(DEV))
    return out_s, out_l


def _plain_boxes(th, tw):
    """(scene, h0, w0, hE, wE): five tile-sized boxes at odd and aligned origins, then an edge box smaller than the tile."""
    return [(0, 3, 5, 3 + th, 5 + tw), (1, 0, 0, th, tw), (0, 30, 36, 30 + th, 36 + tw), (1, 7, 12, 7 + th, 12 + tw),
            (0, 11, 1, 11 + th, 1 + tw), (1, 47 - (th - 6), 61 - (tw - 7), 47, 61)]


def _entries(scenes, boxes, flags=FLAGS, angles=ANGLES, with_label=True):
    sc, lb = scenes
    return [(sc[b[0]], lb[b[0]] if with_label else None, tuple(b[1:]), int(f), float(a))
            for b, f, a in zip(boxes, flags, angles)]


def _global(norm_mode):
    return (torch.linspace(-0.5, 0.7, C_), torch.linspace(0.5, 2.0, C_)) if norm_mode == "global" else None


def _scene_mask(valid_hw, tile, flags=FLAGS, angles=ANGLES):
    """bool [n, th, tw]: the output pixels that come from the scene -- the valid region of each un-augmented tile carried
    through fu_augment (nearest, fill 0)."""
    th, tw = tile
    m = torch.zeros(len(valid_hw), 1, th, tw, device=DEV)
    for i, (vh, vw) in enumerate(valid_hw):
        m[i, :, :vh, :vw] = 1.0
    return (augment.apply(m, None, flags, angles)[0][:, 0] == 1.0).cpu().numpy()


def _photo(n=N, seed=0, terms=("gain", "bias", "sigma")):
    rng = np.random.RandomState(seed)
    p = {"gain": (rng.rand(n, C_) * 0.6 + 0.7).astype(np.float32), "bias": (rng.rand(n, C_) - 0.5).astype(np.float32),
         "sigma": (rng.rand(n, C_) * 0.3).astype(np.float32)}
    p["gain"][1, 2] = p["bias"][1, 2] = p["sigma"][1, 2] = 0.0           # a dropped band
    p = {k: (v if k in terms else None) for k, v in p.items()}
    p["noise_key"], p["noise_stream"] = KEY, STREAMS[:n].copy()
    return p


def _photo_want(plain_image, mask, p):
    """The host statement applied to the plain output at the pixels that come from the scene."""
    x = plain_image.cpu().numpy()
    t = augment.photometric_host(x, p["gain"], p["bias"], p["sigma"], p["noise_key"], p["noise_stream"])
    return torch.from_numpy(np.where(mask[:, None], t, x))


# ------------------------------------------------------------------------------------------------------------ all off
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("norm_mode", NORMS)
def test_null_or_all_off_struct_is_the_plain_call(net, scenes, norm_mode, tile):
    th, tw = tile
    entries = _entries(scenes, _plain_boxes(th, tw))
    kw = dict(pad_value=PAD, nodata_value=NODATA, target_fill=FILL)
    want = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), **kw)
    off = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), photometric={}, **kw)
    keyed = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode),                # a key and streams alone
                              photometric={"noise_key": KEY, "noise_stream": STREAMS}, **kw)         # switch nothing on
    # a NULL struct, through the C ABI itself
    table = (_lib.FuSceneTrainEntry * N)(*[_lib.FuSceneTrainEntry(s.data_ptr(), l.data_ptr(), s.shape[1], s.shape[2], *box,
                                                                  f, a) for s, l, box, f, a in entries])
    image = torch.full((N, C_, th, tw), 9.0, device=DEV)
    target = torch.full((N, th, tw), 9, dtype=torch.int64, device=DEV)
    mean, std = torch.zeros(N, C_, device=DEV), torch.ones(N, C_, device=DEV)
    gp = _global(norm_mode)
    gm, gs = (None, None) if gp is None else (gp[0].to(DEV), gp[1].to(DEV))
    mode = {None: 0, "local": 1, "global": 2}[norm_mode]
    if mode == 2:
        mean[:], std[:] = gm, gs
    _lib.check(_lib.load().fu_scene_train_tiles_ex(net._ctx, N, table, C_, th, tw, mode, _lib.ptr(gm), _lib.ptr(gs), PAD, NODATA,
                                                   FILL, image.data_ptr(), target.data_ptr(),
                                                   mean.data_ptr() if mode == 1 else None,
                                                   std.data_ptr() if mode == 1 else None, None,
                                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    null = (image, target, mean.view(N, C_, 1, 1), std.view(N, C_, 1, 1))
    for got in (off, keyed, null):
        for key, g_, w_ in zip(("image", "target", "mean", "std"), got, want):
            assert g_.dtype == w_.dtype and torch.equal(g_, w_), (key, norm_mode, tile)


# ------------------------------------------------------------------------------------------------------------ radiometric
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("norm_mode", NORMS)
def test_radiometric_output_is_the_host_statement_on_the_plain_output(net, scenes, norm_mode, tile):
    th, tw = tile
    boxes = _plain_boxes(th, tw)
    entries = _entries(scenes, boxes)
    kw = dict(pad_value=PAD, nodata_value=NODATA, target_fill=FILL)
    plain = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), **kw)
    mask = _scene_mask([(b[3] - b[1], b[4] - b[2]) for b in boxes], tile)
    assert mask.any() and not mask.all()
    for terms in (("gain", "bias", "sigma"), ("gain",), ("bias",), ("sigma",)):
        p = _photo(terms=terms)
        got = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), photometric=p, **kw)
        torch.cuda.synchronize()
        assert _bits_equal(got[0].cpu(), _photo_want(plain[0], mask, p)), (terms, norm_mode, tile)
        assert torch.equal(got[1], plain[1])                                    # targets are untouched
        assert _bits_equal(got[2], plain[2]) and _bits_equal(got[3], plain[3])  # so are the statistics
        img = got[0].cpu().numpy()
        if terms != ("gain",):                                                  # (a gain alone keeps a zero pixel zero)
            assert (img[np.broadcast_to(mask[:, None], img.shape)] != plain[0].cpu().numpy()[
                np.broadcast_to(mask[:, None], img.shape)]).mean() > 0.6
    # pad pixels keep pad_value, rotation corners 0
    out = np.broadcast_to(~mask[:, None], img.shape)
    assert set(np.unique(img[out])) == {np.float32(PAD), np.float32(0.0)}
    assert (img[5][:, th - 6:, :] == PAD).all() and (img[5][:, :, tw - 7:] == PAD).all()      # the edge box's padding
    assert (img[3][:, 0, 0] == 0.0).all() and (img[4][:, -1, -1] == 0.0).all()                # rotation corners


def test_noise_follows_the_stream_not_the_batch_position(net, scenes):
    """gain 0, sigma 1: the output IS the noise field.  Samples 0 and 2 share a stream, sample 1 differs in the high word."""
    tile = (20, 24)
    box = (0, 3, 5, 23, 29)
    entries = _entries(scenes, [box] * N, flags=[0] * N, angles=[0.0] * N)
    p = {"gain": np.zeros((N, C_), np.float32), "sigma": np.ones((N, C_), np.float32), "noise_key": KEY, "noise_stream": STREAMS}
    got = scene_train_tiles(net._ctx, entries, tile, None, photometric=p)[0].cpu().numpy()
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[3])
    for b in range(N):
        assert np.array_equal(got[b], augment.noise_host(20, 24, C_, KEY, int(STREAMS[b]))), b
    other_key = dict(p, noise_key=KEY ^ (1 << 40))
    assert not np.array_equal(scene_train_tiles(net._ctx, entries, tile, None, photometric=other_key)[0].cpu().numpy(), got)
    # the noise of a sample does not depend on the batch around it
    alone = scene_train_tiles(net._ctx, entries[3:4], tile, None,
                              photometric={k: (v[3:4] if isinstance(v, np.ndarray) else v) for k, v in p.items()})
    assert np.array_equal(alone[0].cpu().numpy()[0], got[3])


# ------------------------------------------------------------------------------------------------------------ zoom
def _zoom_boxes(th, tw):
    """(scene, box, (out_h, out_w)): magnified (11 x 13), reduced (37 x 41, larger than the tile), identity, the same three
    onto a region smaller than the tile."""
    return [((0, 4, 7, 15, 20), (th, tw)), ((1, 5, 9, 42, 50), (th, tw)), ((0, 21, 30, 21 + th, 30 + tw), (th, tw)),
            ((1, 30, 40, 41, 53), (th - 3, tw - 5)), ((0, 13, 3, 50, 44), (th - 1, tw - 7)),
            ((1, 47 - (th - 6), 61 - (tw - 7), 47, 61), (th - 6, tw - 7))]


def _zoom_want(net, scenes, zb, flags, angles, tile, norm_mode):
    """zoom_tile_host of every source box, normalised, padded into the tile, then fu_augment; under 'local' the statistics
    of the source box from the stats kernel of fu_scene_crops."""
    th, tw = tile
    sc, lb = scenes
    n = len(zb)
    gp = _global(norm_mode)
    mean = np.zeros((n, C_), np.float32)
    std = np.ones((n, C_), np.float32)
    if norm_mode == "local":
        _, m, s = scene_crops(net._ctx, [(sc[b[0]], b[1:]) for b, _ in zb], (48, 48), "local")
        mean, std = m.view(n, C_).cpu().numpy(), s.view(n, C_).cpu().numpy()
    elif norm_mode == "global":
        mean[:], std[:] = gp[0].numpy(), gp[1].numpy()
    image = np.full((n, C_, th, tw), PAD, np.float32)
    target = np.full((n, th, tw), FILL, np.int64)
    for i, ((s, h0, w0, hE, wE), (oh, ow)) in enumerate(zb):
        zi, zl = sampling.zoom_tile_host(sc[s][:, h0:hE, w0:wE].cpu().numpy(), lb[s][h0:hE, w0:wE].cpu().numpy(), (oh, ow))
        if norm_mode is not None:
            zi = zi - mean[i][:, None, None]
            zi = zi / std[i][:, None, None]
        image[i, :, :oh, :ow] = zi
        dec = np.zeros(zl.shape, np.int64)
        dec[zl == 2] = 1
        dec[zl == 0] = NODATA
        target[i, :oh, :ow] = dec
    img, tgt = augment.apply(torch.from_numpy(image).to(DEV), torch.from_numpy(target).to(DEV), flags, angles, target_fill=FILL)
    return img, tgt, torch.from_numpy(mean).view(n, C_, 1, 1), torch.from_numpy(std).view(n, C_, 1, 1)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("norm_mode", NORMS)
def test_zoom_equals_the_host_resize_then_normalise_then_augment(net, scenes, norm_mode, tile):
    th, tw = tile
    base = _zoom_boxes(th, tw)
    kw = dict(pad_value=PAD, nodata_value=NODATA, target_fill=FILL)
    for shift in (0, 1, 2):                      # every kind of zoom meets the flips and the rotation
        zb = base[shift:] + base[:shift]
        entries = _entries(scenes, [b for b, _ in zb])
        zoom = ([o[0] for _, o in zb], [o[1] for _, o in zb])
        got = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), zoom=zoom, **kw)
        want = _zoom_want(net, scenes, zb, FLAGS, ANGLES, tile, norm_mode)
        torch.cuda.synchronize()
        assert _bits_equal(got[0], want[0]), ("image", shift, norm_mode, tile)
        assert got[1].dtype == torch.int64 and torch.equal(got[1], want[1]), ("target", shift, norm_mode, tile)
        assert _bits_equal(got[2].cpu(), want[2]) and _bits_equal(got[3].cpu(), want[3]), ("stats", shift, norm_mode, tile)
        # without labels: the image alone, the same bits
        img_only = scene_train_tiles(net._ctx, _entries(scenes, [b for b, _ in zb], with_label=False), tile, norm_mode,
                                     _global(norm_mode), zoom=zoom, **kw)
        assert img_only[1] is None and _bits_equal(img_only[0], want[0])
    assert (got[1] == 1).any() and (got[1] == NODATA).any() and (got[1] == FILL).any()


@pytest.mark.parametrize("norm_mode", NORMS)
def test_identity_zoom_is_the_plain_call(net, scenes, norm_mode):
    for tile in TILES:
        boxes = _plain_boxes(*tile)
        entries = _entries(scenes, boxes)
        kw = dict(pad_value=PAD, nodata_value=NODATA, target_fill=FILL)
        zoom = ([b[3] - b[1] for b in boxes], [b[4] - b[2] for b in boxes])
        got = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), zoom=zoom, **kw)
        want = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), **kw)
        for g_, w_ in zip(got, want):
            assert torch.equal(g_, w_), (norm_mode, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("norm_mode", NORMS)
def test_combined_path_is_zoom_followed_by_radiometric(net, scenes, norm_mode, tile):
    th, tw = tile
    zb = _zoom_boxes(th, tw)
    entries = _entries(scenes, [b for b, _ in zb])
    zoom = ([o[0] for _, o in zb], [o[1] for _, o in zb])
    kw = dict(pad_value=PAD, nodata_value=NODATA, target_fill=FILL)
    p = _photo(seed=1)
    zoomed = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), zoom=zoom, **kw)
    got = scene_train_tiles(net._ctx, entries, tile, norm_mode, _global(norm_mode), zoom=zoom, photometric=p, **kw)
    mask = _scene_mask([o for _, o in zb], tile)
    torch.cuda.synchronize()
    assert _bits_equal(got[0].cpu(), _photo_want(zoomed[0], mask, p)), (norm_mode, tile)
    assert torch.equal(got[1], zoomed[1]) and _bits_equal(got[2], zoomed[2]) and _bits_equal(got[3], zoomed[3])


@pytest.mark.parametrize("norm_mode", [None, "local"])
def test_vector_and_scalar_stores_give_the_same_values(net, scenes, norm_mode):
    """Tile 20 x 24 into aligned buffers (16-byte stores) and into views that start 4 / 8 bytes past an aligned address
    (element-wise stores): the same values, noise included."""
    tile = th, tw = 20, 24
    zb = _zoom_boxes(th, tw)
    entries = _entries(scenes, [b for b, _ in zb])
    zoom = ([o[0] for _, o in zb], [o[1] for _, o in zb])
    kw = dict(pad_value=PAD, nodata_value=NODATA, target_fill=FILL)
    for options in (dict(photometric=_photo(seed=2)), dict(zoom=zoom), dict(zoom=zoom, photometric=_photo(seed=2)), {}):
        ent = entries if "zoom" in options else _entries(scenes, _plain_boxes(th, tw))
        want = scene_train_tiles(net._ctx, ent, tile, norm_mode, **options, **kw)
        image = torch.full((N * C_ * th * tw + 4,), 9.0, device=DEV)
        target = torch.full((N * th * tw + 2,), 9, dtype=torch.int64, device=DEV)
        assert image.data_ptr() % 16 == 0 and target.data_ptr() % 16 == 0
        out = (image[1:-3].view(N, C_, th, tw), target[1:-1].view(N, th, tw), torch.zeros(N, C_, device=DEV),
               torch.ones(N, C_, device=DEV))
        assert out[0].data_ptr() % 16 == 4 and out[1].data_ptr() % 16 == 8
        got = scene_train_tiles(net._ctx, ent, tile, norm_mode, out=out, **options, **kw)
        torch.cuda.synchronize()
        assert _bits_equal(got[0], want[0]) and torch.equal(got[1], want[1]), (sorted(options), norm_mode)
        assert _bits_equal(got[2], want[2]) and _bits_equal(got[3], want[3])
        assert float(image[0]) == 9.0 and bool((image[-3:] == 9.0).all()) and int(target[0]) == 9 and int(target[-1]) == 9


# ------------------------------------------------------------------------------------------------------------ rejections
def test_rejected_calls_launch_nothing(net, scenes):
    lib = _lib.load()
    sc, lb = scenes
    scene, label = sc[0], lb[0]                                              # [3, 50, 60]
    n, th, tw = 2, 20, 24
    image = torch.full((n, C_, th, tw), -7.0, device=DEV)
    target = torch.full((n, th, tw), -7, dtype=torch.int64, device=DEV)
    mean = torch.full((n, C_), -7.0, device=DEV)
    std = torch.full((n, C_), -7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    nan, inf = float("nan"), float("inf")

    def entry(h0=0, w0=0, hE=20, wE=24):
        return _lib.FuSceneTrainEntry(scene.data_ptr(), label.data_ptr(), 50, 60, h0, w0, hE, wE, 0, 0.0)

    def call(entries, gain=None, bias=None, sigma=None, streams=None, out_h=None, out_w=None, mode=1):
        keep = []

        def host(v, dtype):
            if v is None:
                return None
            keep.append(np.ascontiguousarray(v, dtype=dtype))
            return keep[-1].ctypes.data
        aug = _lib.FuSceneAug(host(gain, np.float32), host(bias, np.float32), host(sigma, np.float32), host(streams, np.uint64),
                              KEY, host(out_h, np.int32), host(out_w, np.int32))
        table = (_lib.FuSceneTrainEntry * len(entries))(*entries)
        return lib.fu_scene_train_tiles_ex(net._ctx, len(entries), table, C_, th, tw, mode, None, None, 0.0, 0, 0,
                                           image.data_ptr(), target.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                           ctypes.byref(aug), stream)

    good = [entry(), entry(5, 9, 42, 50)]                                    # the second: 37 x 41, larger than the tile
    ones, full = np.ones(n * C_, np.float32), dict(out_h=[20, 20], out_w=[24, 24])

    def arr(value, at=4):
        a = ones.copy()
        a[at] = value
        return a
    bad = {
        "box outside the scene (zoom)": lambda: call([entry(), entry(20, 30, 51, 50)], **full),
        "box outside the scene (right, zoom)": lambda: call([entry(), entry(0, 30, 20, 61)], **full),
        "empty box (zoom)": lambda: call([entry(), entry(10, 10, 10, 20)], **full),
        "out_h above the tile": lambda: call(good, out_h=[20, 21], out_w=[24, 24]),
        "out_w above the tile": lambda: call(good, out_h=[20, 20], out_w=[25, 24]),
        "out size 0": lambda: call(good, out_h=[0, 20], out_w=[24, 24]),
        "out_h without out_w": lambda: call(good, out_h=[20, 20]),
        "box larger than the tile without zoom": lambda: call(good, gain=ones),
        "NaN gain": lambda: call(good[:1] * 2, gain=arr(nan)),
        "infinite gain": lambda: call(good[:1] * 2, gain=arr(inf)),
        "NaN bias": lambda: call(good[:1] * 2, bias=arr(nan, 5)),
        "negative sigma": lambda: call(good[:1] * 2, sigma=arr(-0.5), streams=[1, 2]),
        "NaN sigma": lambda: call(good[:1] * 2, sigma=arr(nan, 0), streams=[1, 2]),
        "sigma without noise_stream": lambda: call(good[:1] * 2, sigma=ones),
        "NaN gain with a valid zoom": lambda: call(good, gain=arr(nan), **full),
    }
    for what, fn in bad.items():
        assert fn() == _lib.FU_ERR_INVALID, what
        assert lib.fu_last_error(), what
    torch.cuda.synchronize()
    for buf in (image, mean, std):
        assert bool((buf == -7.0).all())
    assert bool((target == -7).all())
    # and the same table, valid, does run
    assert call(good, gain=ones, sigma=ones * 0.5, streams=[1, 2], **full) == _lib.FU_OK
    torch.cuda.synchronize()
    assert not bool((image == -7.0).any()) and not bool((target == -7).any()) and not bool((mean == -7.0).any())


# ------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from tools.tiff_writer import make_floodplanet_tree
    root = str(tmp_path_factory.mktemp("aug_tree"))
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=2, label_size=90, s1_size=37)
    return FloodplanetTiles(root, "test", generate_image_slice_object(32, 32, 24), eval_region=["RegA", "RegB"], sensor="S1",
                            ignore_index=0, norm_mode="local")


PHOTO_CFG = dict(gain=0.2, band_gain=0.1, brightness=0.3, noise=0.1, band_drop=0.2, likelihood=0.8)


def _epoch(loader):
    out = list(loader)
    torch.cuda.synchronize()
    return out


def test_loader_defaults_deliver_the_batches_of_the_plain_call(net, dataset):
    """With the new options off a batch is what it always was: the transforms drawn from RandomState(seed), batch after
    batch, and one plain fu_scene_train_tiles call on the grid's boxes -- and it carries no new key."""
    seed = 5
    loader = SceneTileLoader(dataset, 7, DEV, net, shuffle=False, transforms={}, seed=seed, photometric=None, zoom=None)
    rng = np.random.RandomState(seed)
    n = 0
    for epoch in range(2):
        for batch in loader:
            flags, angles = augment.sample_transforms(len(batch["index"]), {}, rng)
            entries = [loader._items[i] + (int(f), float(a)) for i, f, a in zip(batch["index"], flags, angles)]
            want = scene_train_tiles(net._ctx, entries, (32, 32), "local", nodata_value=0, target_fill=0)
            torch.cuda.synchronize()
            assert np.array_equal(batch["flags"], flags) and np.array_equal(batch["angles"], angles)
            assert _bits_equal(batch["image"], want[0]) and torch.equal(batch["target"], want[1])
            assert _bits_equal(batch["mean"], want[2]) and _bits_equal(batch["std"], want[3])
            assert not {"photometric", "src_boxes", "boxes"} & set(batch)
            n += len(batch["index"])
    assert n == 2 * len(dataset)


def test_loader_augments_deterministically_and_the_batch_says_how(net, dataset):
    seed = 5
    make = lambda **k: SceneTileLoader(dataset, 7, DEV, net, shuffle=True, transforms={}, seed=seed, **k)
    plain, a, b = make(), make(photometric=PHOTO_CFG), make(photometric=PHOTO_CFG)
    first, changed = {}, []
    for epoch in range(2):
        for k, (p_, a_, b_) in enumerate(zip(_epoch(plain), _epoch(a), _epoch(b))):
            # the transforms' stream is not consumed differently: the same order, flags and angles as the plain loader
            assert a_["index"] == p_["index"] and np.array_equal(a_["flags"], p_["flags"])
            assert np.array_equal(a_["angles"], p_["angles"])
            assert _bits_equal(a_["image"], b_["image"]) and torch.equal(a_["target"], p_["target"])      # same seed
            assert _bits_equal(a_["mean"], p_["mean"]) and _bits_equal(a_["std"], p_["std"])
            ph = a_["photometric"]
            assert ph["noise_key"] == a.noise_key
            assert ph["noise_stream"].dtype == np.uint64
            assert ph["noise_stream"].tolist() == [epoch * len(dataset) + i for i in a_["index"]]      # epoch-major
            # the batch's own record reproduces the image from the un-augmented batch
            valid = [(hE - h0, wE - w0) for h0, w0, hE, wE in (a._items[i][2] for i in a_["index"])]
            mask = _scene_mask(valid, (32, 32), a_["flags"], a_["angles"])
            assert _bits_equal(a_["image"].cpu(), _photo_want(p_["image"], mask, ph)), (epoch, k)
            changed.append(not _bits_equal(a_["image"], p_["image"]))
            for i, row in zip(a_["index"], range(len(a_["index"]))):
                first.setdefault(epoch, {})[i] = (a_["image"][row].cpu(), ph["gain"][row].copy())
    assert sum(changed) >= len(changed) - 2          # (a batch of one sample that lost the coin stays as it was)
    # a new epoch draws anew and keys its noise anew
    assert sorted(first[0]) == sorted(first[1]) == list(range(len(dataset)))
    assert sum(np.array_equal(first[0][i][1], first[1][i][1]) for i in first[0]) < len(dataset) // 2


def test_loader_zoom_reads_the_zoomed_boxes_and_reports_them(net, dataset):
    seed = 3
    loader = SceneTileLoader(dataset, 7, DEV, net, shuffle=False, transforms={}, seed=seed, zoom=(0.6, 1.7),
                             photometric=dict(noise=0.05))
    again = SceneTileLoader(dataset, 7, DEV, net, shuffle=False, transforms={}, seed=seed, zoom=(0.6, 1.7),
                            photometric=dict(noise=0.05))
    epochs = []
    for epoch in range(2):
        got = _epoch(loader)
        for batch, same in zip(got, _epoch(again)):
            assert _bits_equal(batch["image"], same["image"]) and torch.equal(batch["target"], same["target"])
            grid = [loader._items[i][2] for i in batch["index"]]
            assert batch["boxes"] == grid and len(batch["src_boxes"]) == len(grid)
            assert any(s != g for s, g in zip(batch["src_boxes"], grid))
            entries = [loader._items[i][:2] + (src, int(f), float(a))
                       for i, src, f, a in zip(batch["index"], batch["src_boxes"], batch["flags"], batch["angles"])]
            zoom = ([g[2] - g[0] for g in grid], [g[3] - g[1] for g in grid])
            want = scene_train_tiles(net._ctx, entries, (32, 32), "local", nodata_value=0, target_fill=0, zoom=zoom,
                                     photometric=batch["photometric"])
            torch.cuda.synchronize()
            assert _bits_equal(batch["image"], want[0]) and torch.equal(batch["target"], want[1])
            assert batch["photometric"]["gain"] is None and batch["photometric"]["sigma"].shape == (len(grid), 2)
        epochs.append([b["src_boxes"] for b in got])
    assert epochs[0] != epochs[1]


def test_fit_cli_trains_with_the_options_and_records_them(tmp_path, capsys):
    import json
    import os

    from floodplanet_code_amd import fit
    from tools.tiff_writer import make_floodplanet_tree
    root = str(tmp_path / "tree")
    make_floodplanet_tree(root, regions=("RegA", "RegB"), images_per_region=1, label_size=100, s1_size=40)
    out = fit.main([root, "--exp_dir", str(tmp_path / "exp"), "--sensor", "S1", "--eval_region", "RegB", "--crop", "64", "64",
                    "--stride", "32", "--batch_size", "4", "--n_epochs", "1", "--lr", "2e-3", "--base_channels", "8",
                    "--n_workers", "0", "--seed", "0", "--save_topk_models", "1", "--device", DEV, "--norm_mode", "local",
                    "--aug_gain", "0.2", "--aug_noise", "0.05", "--aug_band_drop", "0.1", "--aug_zoom", "0.7", "1.4"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = {"photometric": {"gain": 0.2, "noise": 0.05, "band_drop": 0.1}, "zoom": [0.7, 1.4]}
    assert line["augmentation"] == want and os.path.exists(out["checkpoint"])
    assert np.isfinite(out["history"][0]["train_loss"]) and 0.0 <= out["history"][0]["val_MulticlassJaccardIndex"] <= 1.0
    hyper = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)["hyper_parameters"]
    assert hyper["augmentation"] == want


def test_loader_rejects_bad_options(net, dataset):
    for bad in (dict(zoom=(0.4, 1.0)), dict(zoom=(1.5, 1.2)), dict(photometric=dict(gain=-1.0)),
                dict(photometric=dict(gamma=0.5))):
        with pytest.raises(ValueError):
            SceneTileLoader(dataset, 7, DEV, net, **bad)
