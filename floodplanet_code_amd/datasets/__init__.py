"""Host-side data path for the bundled FloodPlanet rasters: TIFF decoding, tile grid, dataset."""
from .assemble import assemble_tiles
from .class_weights import balanced_class_weights, label_class_counts, label_class_counts_host
from .floodplanet import FloodplanetTiles, collate_tiles
from .geotiff import raster_info, raster_size, read_raster, read_raster_encoded
from .loader import TileLoader
from .scene_loader import SceneResidencyError, SceneTileLoader
from .resize import resize_image, resize_lanczos4, resize_nearest
from .tiff import TiffError, read_tiff, tiff_info, tiff_size
from .tiles import CropParams, generate_image_slice_object, get_crop_slices

__all__ = ["assemble_tiles", "balanced_class_weights", "label_class_counts", "label_class_counts_host", "FloodplanetTiles", "collate_tiles", "TileLoader", "SceneTileLoader", "SceneResidencyError", "resize_image", "resize_lanczos4", "resize_nearest", "TiffError",
           "read_tiff", "tiff_info", "tiff_size", "raster_info", "raster_size", "read_raster", "read_raster_encoded", "CropParams", "generate_image_slice_object", "get_crop_slices"]
