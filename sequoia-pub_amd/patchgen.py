"""WSI -> patches: host-side counterpart of /root/reference/pre_processing/patch_gen_hdf5.py --
``get_mask_image`` (:25-39), ``get_mask`` (:41-50) and ``extract_patches`` (:51-137): Otsu tissue mask on the lowest
pyramid level, 3 x dilation + 3 x erosion, seed-5 shuffled grid of level-0 tiles, per-tile tissue / contrast filter,
one uint8 ``"{x}_{y}"`` dataset per kept tile in ``<patch_path>/<slide>/<slide>.hdf5`` + ``complete.txt``.

This stage sits in front of the accelerated path.  Its per-tile filter in numpy (float64, one core) takes 8.5 ms per
256 x 256 candidate tile and 28 ms per 512 x 512 one -- up to minutes per slide, against tens of milliseconds for everything
behind it -- so the filter also has a device form: ``filter_patches`` (``sq_patch_filter``, csrc/patchfilter.hip) and
``extract_patches(..., device=...)``, which keeps the slide mask, the visiting order and every written byte of the host
path and takes 4.25 / 17.8 us per tile with the upload from pinned memory (tools/patch_filter_rate.py measures both
filters side by side: profiles/patch_filter_rate.txt).  The whole-slide mask in front of it (``get_mask`` on the lowest
level and the closing: seconds per slide in numpy / scipy on one core) has a device form as well: ``slide_mask``
(``sq_slide_mask``, csrc/slidemask.hip) and ``extract_patches(..., device=..., slide_mask="device")``, every mask bit and
the bytes of ``mask.npy`` the host's (tools/slide_mask_rate.py, profiles/slide_mask_rate.txt).  With both, what is left of
the stage is reading the regions: ``wsi.TiffSlide`` decodes JPEG-tiled TIFF / SVS slides on the device and hands whole batches of
regions over as device tensors (``read_regions``; profiles/slide_read_rate.txt), other slide objects are read region by region.
The device forms take RGBA as OpenSlide's ``read_region`` returns it (the kernels skip the fourth byte, so the host copies a
region whole instead of repacking it: 4.3 against 171 us per 256 x 256 region, profiles/region_path_rate.txt), and
``embed_slide`` runs the same walk with the kept tiles staying on the device -- order, ``random.sample`` cut, extractor and
k-Means as the patch file, cli.compute_features and cli.kmean_features would have them -- so that no patch store is written.
What is restated here are the scikit-image functions the reference calls (scikit-image is not installed in this image):
``rgb2hsv`` (saturation channel), ``threshold_otsu`` (integer and float histograms), ``is_low_contrast`` -- pinned
against scikit-image 0.18.3 itself by tests/golden/patchgen.npz (made with the image's conda interpreter,
tests/golden/make_patchgen_golden.py).  ``binary_dilation`` / ``binary_erosion`` are scipy's, as in the reference.

A slide is anything with OpenSlide's interface subset (``level_dimensions``, ``read_region(location, level, size)``,
``properties``); ``ArraySlide`` provides it over numpy arrays so the whole flow runs without openslide."""
import os

import numpy as np
from scipy.ndimage import binary_dilation, binary_erosion

from . import _lib, store
from ._abi import CONSTANTS as _C

FILTER_MIN_DIM, FILTER_MAX_DIM = _C["SQ_PATCH_FILTER_MIN_DIM"], _C["SQ_PATCH_FILTER_MAX_DIM"]
SLIDE_MASK_MAX_DIM, SLIDE_MASK_MAX_PIXELS = _C["SQ_SLIDE_MASK_MAX_DIM"], 1 << 30      # h w <= 2^30
SLIDE_MASK_MAX_ITERATIONS = _C["SQ_SLIDE_MASK_MAX_ITERATIONS"]
SLIDE_MASK_TILE = (_C["SQ_SLIDE_MASK_TILE_ROWS"], _C["SQ_SLIDE_MASK_TILE_COLS"])      # the closing kernel's tile
TILE_GRID_MAX_WINDOW, TILE_GRID_PACKED_MAX_WINDOW = _C["SQ_TILE_GRID_MAX_WINDOW"], _C["SQ_TILE_GRID_PACKED_MAX_WINDOW"]
TILE_GRID_MAX_ITERATIONS = _C["SQ_TILE_GRID_MAX_ITERATIONS"]


# ---- scikit-image restatements ---------------------------------------------------------------------------------
def saturation(img_rgb_u8):
    """skimage.color.rgb2hsv(img)[..., 1] for a uint8 RGB image: delta / max on img_as_float(img) (float64; scikit-image
    scales by MULTIPLYING with 1/255), 0 where delta == 0."""
    arr = np.asarray(img_rgb_u8).astype(np.float64) * (1.0 / 255.0)
    v = arr.max(-1)
    delta = np.ptp(arr, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = delta / v
    s[delta == 0.0] = 0.0
    return s


def threshold_otsu(image, nbins=256):
    """skimage.filters.threshold_otsu: integer images -> one bin per integer value in [min, max]; float images -> `nbins`
    equal bins over [min, max], thresholds at bin centres; the class-separability maximum (first one) wins."""
    image = np.asarray(image)
    first = image.ravel()[0]
    if np.all(image == first):
        return first
    flat = image.ravel()
    if np.issubdtype(flat.dtype, np.integer):
        lo, hi = int(flat.min()), int(flat.max())
        counts = np.bincount(flat.astype(np.int64) - lo, minlength=hi - lo + 1)
        centers = np.arange(lo, hi + 1)
    else:
        counts, edges = np.histogram(flat, bins=nbins, range=(flat.min(), flat.max()))
        centers = (edges[:-1] + edges[1:]) / 2.0
    counts = counts.astype(float)
    weight1 = np.cumsum(counts)
    weight2 = np.cumsum(counts[::-1])[::-1]
    mean1 = np.cumsum(counts * centers) / weight1
    mean2 = (np.cumsum((counts * centers)[::-1]) / weight2[::-1])[::-1]
    variance12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    return centers[int(np.argmax(variance12))]


def is_low_contrast(image_rgb_u8, fraction_threshold=0.05, lower_percentile=1, upper_percentile=99):
    """skimage.exposure.is_low_contrast on an RGB uint8 image: luminance 0.2125 R + 0.7154 G + 0.0721 B of img / 255,
    percentile spread relative to the float dtype range (-1, 1)."""
    arr = np.asarray(image_rgb_u8).astype(np.float64) * (1.0 / 255.0)
    gray = arr @ np.array([0.2125, 0.7154, 0.0721])
    lo, hi = np.percentile(gray, [lower_percentile, upper_percentile])
    return bool((hi - lo) / 2.0 < fraction_threshold)


# ---- patch_gen_hdf5.py -----------------------------------------------------------------------------------------
def get_mask_image(img_rgb, rgb_min=50):
    """patch_gen_hdf5.py:25-39: tissue = saturated AND not (bright in all three channels) AND every channel > rgb_min."""
    img = np.asarray(img_rgb)
    bright = np.ones(img.shape[:2], dtype=bool)
    for c in range(3):
        bright &= img[:, :, c] > threshold_otsu(img[:, :, c])
    s = saturation(img)
    return (s > threshold_otsu(s)) & ~bright & (img > rgb_min).all(-1)


def get_mask(slide, level='max', rgb_min=50):
    """patch_gen_hdf5.py:41-50: Otsu mask of the whole slide at pyramid level `level`; the array is indexed [x, y]."""
    if level == 'max':
        level = len(slide.level_dimensions) - 1
    img = np.transpose(np.asarray(slide.read_region((0, 0), level, slide.level_dimensions[level]))[:, :, :3], axes=[1, 0, 2])
    return get_mask_image(img, rgb_min), level


class ArraySlide:
    """OpenSlide's interface subset over in-memory pyramid levels (each [height, width, 3] uint8, level 0 first)."""

    def __init__(self, levels, properties=None):
        self.levels = [np.asarray(a) for a in levels]
        self.level_dimensions = [(a.shape[1], a.shape[0]) for a in self.levels]       # (width, height) like OpenSlide
        self.dimensions = self.level_dimensions[0]
        self.properties = dict(properties or {})

    def read_region(self, location, level, size):
        """location = level-0 (x, y) of the top-left corner, size = (width, height) at `level`; outside the slide: white."""
        a = self.levels[level]
        sx = self.level_dimensions[0][0] / self.level_dimensions[level][0]
        sy = self.level_dimensions[0][1] / self.level_dimensions[level][1]
        x0, y0 = int(location[0] / sx), int(location[1] / sy)
        out = np.full((size[1], size[0], 3), 255, dtype=np.uint8)
        h, w = max(0, min(size[1], a.shape[0] - y0)), max(0, min(size[0], a.shape[1] - x0))
        out[:h, :w] = a[y0:y0 + h, x0:x0 + w, :3]
        return out


def _resize_like_reference(patch, size):
    """patch_gen_hdf5.py:117 ``patch.resize(patch_size)`` on the PIL image of a 40x region: Pillow's default filter
    (BICUBIC since Pillow 2.7; requirements.txt pins pillow==10.3.0).  Pillow is the reference's own resampler, so the
    stored pixels are the reference's; without it there is no faithful substitute and the call fails loudly."""
    try:
        from PIL import Image
    except ImportError as e:                         # pragma: no cover
        raise RuntimeError("40x slides are shrunk with PIL.Image.resize (bicubic) as the reference does: Pillow is required") from e
    return np.asarray(Image.fromarray(np.ascontiguousarray(patch)).resize((int(size[0]), int(size[1]))))


def filter_patches(patches_u8, rgb_min=50, background_threshold=0.2, fraction_threshold=0.05, return_stats=False,
                   return_masks=False):
    """The per-tile filter of extract_patches (patch_gen_hdf5.py:110-115) for a uint8 [n, H, W, 3] CUDA tensor (or
    [n, H, W, 4]: RGBA as a slide reader returns it, the fourth channel ignored, every result that of the RGB values), 8 <= H,
    W <= 512: bool [n], True where ``binary_dilation(get_mask_image(tile, rgb_min), iterations=3).sum() > background_threshold *
    H * W and not is_low_contrast(tile, fraction_threshold)``.  ``return_stats``: also float64 [n, 8] = thr_R, thr_G, thr_B,
    thr_S, mask count, dilated count, contrast ratio, 0 -- thresholds and counts equal to the host functions' bit for bit,
    the ratio to 1e-12 (include/sequoia_hip.h).  ``return_masks``: also the bool [n, H, W] masks before and after the
    dilation.  Asynchronous on the current stream; no CPU fallback."""
    import torch
    if torch.is_tensor(patches_u8) and (patches_u8.dtype != torch.uint8 or patches_u8.dim() != 4 or patches_u8.shape[3] not in (3, 4)):
        raise ValueError(f"filter_patches takes uint8 [n, H, W, 3 or 4], got {patches_u8.dtype} {tuple(patches_u8.shape)}")
    _lib.require_gpu()
    if not (torch.is_tensor(patches_u8) and patches_u8.is_cuda):
        raise _lib.SequoiaHipError("filter_patches needs a CUDA tensor (no CPU fallback)")
    x = patches_u8.contiguous()
    n, H, W, C = x.shape
    dev = x.device
    need = _lib.need(_lib.lib().sq_patch_filter_workspace_bytes, max(n, 1), H, W)       # refuses a bad size with the library's message
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    stats = torch.empty(n, 8, dtype=torch.float64, device=dev) if return_stats else None
    raw = torch.empty(n, H, W, dtype=torch.uint8, device=dev) if return_masks else None
    dil = torch.empty(n, H, W, dtype=torch.uint8, device=dev) if return_masks else None
    if n:
        _lib.call("sq_patch_filter_px", dev, x, n, H, W, C, int(rgb_min), float(background_threshold), float(fraction_threshold),
                  keep, stats, raw, dil, workspace=need)
    out = (keep.bool(),)
    if return_stats:
        out += (stats,)
    if return_masks:
        out += (raw.bool(), dil.bool())
    return out[0] if len(out) == 1 else out


def slide_mask(img_u8, rgb_min=50, iterations=3, transpose=False, return_raw=False, return_stats=False):
    """The whole-slide mask of extract_patches (patch_gen_hdf5.py:25-50,69-72) for ONE uint8 [H, W, 3] CUDA tensor (or
    [H, W, 4], the fourth channel ignored) of any size up to 32768 x 32768 and 2^30 pixels: bool [H, W] = ``binary_erosion(binary_dilation(get_mask_image(img, rgb_min),
    iterations=iterations), iterations=iterations)``, every bit the host's; ``iterations`` in 0..8, 0 leaves the mask as it
    is.  ``transpose``: the results as C-contiguous [W, H], equal to the host's on the transposed image (the layout of the
    reference's mask.npy) without a transposing copy.  ``return_raw``: also the mask before the closing.  ``return_stats``:
    also float64 [8] = thr_R, thr_G, thr_B, thr_S, raw count, closed count, min and max of the saturation, all exact.
    Asynchronous on the current stream; no CPU fallback."""
    import torch
    if torch.is_tensor(img_u8) and (img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] not in (3, 4)):
        raise ValueError(f"slide_mask takes uint8 [H, W, 3 or 4], got {img_u8.dtype} {tuple(img_u8.shape)}")
    _lib.require_gpu()
    if not (torch.is_tensor(img_u8) and img_u8.is_cuda):
        raise _lib.SequoiaHipError("slide_mask needs a CUDA tensor (no CPU fallback)")
    x = img_u8.contiguous()
    H, W, C = x.shape
    dev = x.device
    need = _lib.need(_lib.lib().sq_slide_mask_workspace_bytes, H, W)                    # refuses a bad size with the library's message
    shape = (W, H) if transpose else (H, W)
    closed = torch.empty(shape, dtype=torch.uint8, device=dev)
    raw = torch.empty(shape, dtype=torch.uint8, device=dev) if return_raw else None
    stats = torch.empty(8, dtype=torch.float64, device=dev) if return_stats else None
    _lib.call("sq_slide_mask_px", dev, x, H, W, C, int(rgb_min), int(iterations), int(bool(transpose)), raw, closed, stats, workspace=need)
    out = (closed.view(torch.bool),)
    if return_raw:
        out += (raw.view(torch.bool),)
    if return_stats:
        out += (stats,)
    return out[0] if len(out) == 1 else out


def tile_grid_geometry(mask_shape, slide_dims, patch_size_resized):
    """(downsample_factor, patch_size_in_mask, n_col, n_row) of the valid-tile grid as cli.visualize.valid_tiles derives them
    (visualize.py:181-189) from the [mask_w, mask_h] shape of the mask, the slide's level-0 (width, height) and the read
    size.  ValueError for what the device form does not take: a factor below 1 (a mask wider than the slide, where the host
    divides by zero) and a window above 512."""
    p = int(patch_size_resized)
    if p < 1:
        raise ValueError(f"patch_size_resized={patch_size_resized}: at least 1")
    if len(mask_shape) != 2 or int(mask_shape[0]) < 1 or int(mask_shape[1]) < 1:
        raise ValueError(f"valid-tile grid: a mask of shape {tuple(mask_shape)}, [mask_w, mask_h] with both extents at least 1 is needed")
    downsample_factor = int(slide_dims[0] / mask_shape[0])
    if downsample_factor < 1:
        raise ValueError(f"valid-tile grid: slide width {slide_dims[0]} over mask width {mask_shape[0]} gives a downsample factor of "
                         f"{downsample_factor}, below 1")
    patch_size_in_mask = int(p / downsample_factor)
    if patch_size_in_mask > TILE_GRID_MAX_WINDOW:
        raise ValueError(f"valid-tile grid: a window of {patch_size_in_mask} mask pixels (read size {p}, downsample factor "
                         f"{downsample_factor}): at most {TILE_GRID_MAX_WINDOW}")
    n_col, n_row = len(range(0, int(slide_dims[0]) - p, p)), len(range(0, int(slide_dims[1]) - p, p))
    return downsample_factor, patch_size_in_mask, n_col, n_row


def valid_tile_grid(mask, slide_dims, patch_size_resized, iterations=3, threshold=0.5, return_counts=False):
    """The valid-tile grid of the spatial maps (spatial_vis/visualize.py:174-205; cli.visualize.valid_tiles on the host) for a
    bool or uint8 CUDA tensor ``mask`` [mask_w, mask_h] in the layout of mask.npy (indexed [x, y], any non-zero byte is
    tissue): bool [n_col, n_row], True where ``binary_dilation(window, iterations=iterations).sum() >= threshold *
    window.size`` for the tile's window ``mask[c:c + pm, r:r + pm]`` -- clipped as numpy clips it, possibly empty (then
    valid), nothing from outside the window entering the dilation.  Row-major order of the result is the host loop's visiting
    order.  ``return_counts``: also the int32 [n_col, n_row] dilated counts and clipped window sizes.  The downsample factor
    and the window come from ``tile_grid_geometry`` exactly as the host derives them; a factor below 1 or a window above 512
    is a ValueError.  ``iterations`` in 0..8 (0: the window as it is).  An empty grid returns an empty tensor without a launch.
    Asynchronous on the current stream; no CPU fallback."""
    import torch
    shape = tuple(mask.shape) if hasattr(mask, "shape") else ()
    ds, pm, n_col, n_row = tile_grid_geometry(shape, slide_dims, patch_size_resized)
    _lib.require_gpu()
    if not (torch.is_tensor(mask) and mask.is_cuda):
        raise _lib.SequoiaHipError("valid_tile_grid needs a CUDA tensor (no CPU fallback)")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"valid_tile_grid takes a bool or uint8 mask [mask_w, mask_h], got {mask.dtype}")
    x = mask.contiguous()
    x = x.view(torch.uint8) if x.dtype == torch.bool else x
    dev = x.device
    valid = torch.empty((n_col, n_row), dtype=torch.uint8, device=dev)
    counts = torch.empty((n_col, n_row), dtype=torch.int32, device=dev) if return_counts else None
    sizes = torch.empty((n_col, n_row), dtype=torch.int32, device=dev) if return_counts else None
    if n_col and n_row:
        _lib.call("sq_tile_grid_valid", dev, x, x.shape[0], x.shape[1], n_col, n_row, int(patch_size_resized), ds, pm,
                  int(iterations), float(threshold), valid, counts, sizes)
    return (valid.view(torch.bool), counts, sizes) if return_counts else valid.view(torch.bool)


def _mask_level_size(slide):
    """(level, (width, height)) of the image get_mask reads."""
    level = len(slide.level_dimensions) - 1
    return level, tuple(int(v) for v in slide.level_dimensions[level])


def _closed_mask_on_device(slide, device):
    """get_mask + the closing of extract_patches on `device`: the level image as get_mask reads it (RGB, or RGBA as
    OpenSlide returns it: ``sq_slide_mask_px`` reads 4-byte pixels, so the host does not repack them), uploaded through pinned
    memory, ``slide_mask(transpose=True)``, and the bool [W, H] array back on the host."""
    import torch
    level, size = _mask_level_size(slide)
    if hasattr(slide, "read_regions"):       # wsi.TiffSlide: the level image is decoded on the device and never leaves it
        mask = slide_mask(slide.read_regions([(0, 0)], level, size)[0].to(device), transpose=True)
        return mask.cpu().numpy(), level
    img = np.asarray(slide.read_region((0, 0), level, size))
    if img.shape[2] != 4:                    # RGBA goes up whole, one contiguous copy: the kernels skip the fourth byte
        img = img[:, :, :3]
    pinned = torch.empty(img.shape, dtype=torch.uint8).pin_memory()
    pinned.numpy()[...] = img
    mask = slide_mask(pinned.to(device, non_blocking=True), transpose=True)
    return mask.cpu().numpy(), level


def _filtered_on_host(slide, candidates, size_read, patch_size, resize_factor, background_threshold):
    """The kept tiles of `candidates` (visiting order) as ((x, y), uint8 array) pairs: patch_gen_hdf5.py:108-118, one region
    read, filtered and, for a 40x slide, shrunk per step of the generator."""
    for xy in candidates:
        patch = np.asarray(slide.read_region(xy, 0, size_read))[:, :, :3]
        tissue = binary_dilation(get_mask_image(patch), iterations=3)
        if tissue.sum() > background_threshold * tissue.size and not is_low_contrast(patch):
            if resize_factor != 1.0:
                patch = _resize_like_reference(patch, patch_size)
            yield xy, patch


def _as_layout(region, channels):
    """One region as read (RGB or RGBA) in the layout of a pinned buffer of `channels` channels: as it is when the channel
    counts agree, else converted on the host."""
    if region.shape[2] == channels:
        return region
    if channels == 3:
        return region[:, :, :3]
    out = np.full(region.shape[:2] + (4,), 255, dtype=np.uint8)
    out[:, :, :3] = region[:, :, :3]
    return out


def _read_batch(slide, chunk, size_read):
    """``slide.read_regions`` of a chunk of level-0 corners as (uint8 [k, h, w, 4] device tensor or None, k, error): k is the
    whole chunk and the error None when every region was read; else the regions in front of the first one that fails, as the
    per-region loop would have read them, and the error of that one.  Only the reader's own two errors are taken apart that
    way -- tiles that did not decode, and a tile the container parser refuses when it is read; any other error (a device out
    of memory, a library error) ends the reading at once with nothing of the chunk."""
    from .wsi import TileDecodeError, WsiFormatError
    try:
        return slide.read_regions(chunk, 0, size_read), len(chunk), None
    except TileDecodeError as e:             # every other region of the batch is there
        k = e.first_failed_region
        return (e.regions[:k] if k else None), k, e
    except WsiFormatError as e:              # refused on the host before anything ran: a tile's header, its range in the file
        k = 0
        for xy in chunk:
            try:
                slide.read_regions([xy], 0, size_read)
            except WsiFormatError:
                break
            k += 1
        return (slide.read_regions(chunk[:k], 0, size_read) if k else None), k, e
    except Exception as e:
        return None, 0, e


def _kept_on_device(slide, candidates, size_read, patch_size, resize_factor, background_threshold, budget, device, batch):
    """The kept tiles of `candidates` (visiting order), at most `budget` of them, chunk by chunk as (list of (x, y), uint8
    [k, patch_h, patch_w, 3] tensor on `device`) pairs: regions are read in chunks of `batch` into pinned memory, filtered on
    `device` and the kept ones gathered there -- for a 40x slide through the Pillow-exact bicubic shrink
    (``resize_u8_pil(index=)``), else as they are (``pack_rgb(index=)``).  The first region read decides the buffer's layout:
    an RGBA region (what OpenSlide returns) is copied whole, one contiguous copy, and the kernels skip the fourth byte; a
    later region with the other channel count is converted on the host.  No chunk is read once the budget is met.  A read
    error ends the reading; the tiles read before it are still filtered and yielded, then the error is raised -- unless
    the budget was met by then, where the host loop would not have reached the failing read.  A slide with ``read_regions``
    (``wsi.TiffSlide``) hands each chunk over as a device tensor instead -- every tile the chunk touches decoded once, no
    pixel on the host -- with the same order, budget and read-error rule."""
    import torch
    from . import imgproc
    pinned = view = channels = None
    batched = hasattr(slide, "read_regions")
    pos, error = 0, None
    while pos < len(candidates) and budget > 0 and error is None:
        chunk = candidates[pos:pos + batch]
        pos += len(chunk)
        k = 0
        if batched:
            tiles, k, error = _read_batch(slide, chunk, size_read)
        else:
            for xy in chunk:
                try:
                    region = np.asarray(slide.read_region(xy, 0, size_read))
                    if pinned is None:
                        channels = 4 if region.shape[2] == 4 else 3
                        pinned = torch.empty((batch, size_read[1], size_read[0], channels), dtype=torch.uint8).pin_memory()
                        view = pinned.numpy()
                    view[k] = _as_layout(region, channels)
                except Exception as e:
                    error = e
                    break
                k += 1
        if k == 0:
            break
        tiles = tiles.to(device) if batched else pinned[:k].to(device, non_blocking=True)
        kept = torch.nonzero(filter_patches(tiles, background_threshold=background_threshold)).flatten()[:budget].to(torch.int32)
        n_kept = int(kept.numel())            # nonzero has waited for the upload and the filter: `pinned` may be written again
        if n_kept:
            if resize_factor != 1.0:
                out = imgproc.resize_u8_pil(tiles, (int(patch_size[1]), int(patch_size[0])), "bicubic", index=kept)
            else:
                out = imgproc.pack_rgb(tiles, index=kept)
            yield [chunk[j] for j in kept.tolist()], out
            budget -= n_kept
    if error is not None and budget > 0:
        raise error


def _filtered_on_device(slide, candidates, size_read, patch_size, resize_factor, background_threshold, budget, device, batch):
    """``_kept_on_device`` as ((x, y), uint8 array) pairs on the host, the form ``_filtered_on_host`` yields."""
    for coords, tiles in _kept_on_device(slide, candidates, size_read, patch_size, resize_factor, background_threshold, budget,
                                         device, batch):
        yield from zip(coords, tiles.cpu().numpy())


def _check_device_request(slide, patch_size, device, batch, slide_mask):
    """What extract_patches and embed_slide refuse before they touch a file."""
    if slide_mask not in ("host", "device"):
        raise ValueError(f"slide_mask={slide_mask!r}: 'host' or 'device'")
    if slide_mask == "device" and device is None:
        raise ValueError("slide_mask='device' needs device=")
    if device is not None:
        if int(batch) < 1:
            raise ValueError(f"batch={batch}: at least 1")
        _lib.require_gpu()
        factor = float(slide.properties.get('aperio.AppMag', 20)) / 20.0
        region = (int(factor * patch_size[0]), int(factor * patch_size[1]))
        if not all(FILTER_MIN_DIM <= v <= FILTER_MAX_DIM for v in region):
            raise ValueError(f"device filter: regions of {region} pixels, every extent must be in {FILTER_MIN_DIM}..{FILTER_MAX_DIM}")
        if slide_mask == "device":
            level, (lw, lh) = _mask_level_size(slide)
            if not (1 <= lw <= SLIDE_MASK_MAX_DIM and 1 <= lh <= SLIDE_MASK_MAX_DIM and lw * lh <= SLIDE_MASK_MAX_PIXELS):
                raise ValueError(f"device slide mask: level {level} is {lw} x {lh} pixels, every extent must be in 1..{SLIDE_MASK_MAX_DIM} "
                                 f"and the image at most 2^30 pixels")


def _candidate_walk(slide, slide_id, patch_size, slide_mask, device, mask_file):
    """patch_gen_hdf5.py:65-107: the closed slide mask (saved to `mask_file` unless that is None) and the seed-5 shuffled grid
    of level-0 tiles.  Returns (candidates, size_read, resize_factor, n_grid): `candidates` generates the (x, y) that lie on
    the mask, looked up as they are visited; n_grid is the size of the whole grid (the cap when none is given)."""
    if slide_mask == "device":
        mask, mask_level = _closed_mask_on_device(slide, device)
    else:
        mask, mask_level = get_mask(slide)
        mask = binary_erosion(binary_dilation(mask, iterations=3), iterations=3)
    if mask_file is not None:
        np.save(mask_file, mask)
    ratio_x = slide.level_dimensions[0][0] / slide.level_dimensions[mask_level][0]
    ratio_y = slide.level_dimensions[0][1] / slide.level_dimensions[mask_level][1]
    xmax, ymax = slide.level_dimensions[0]
    resize_factor = float(slide.properties.get('aperio.AppMag', 20)) / 20.0          # 40x slides: read 2x the size, shrink
    size_read = (int(resize_factor * patch_size[0]), int(resize_factor * patch_size[1]))
    print(f"patch size for {slide_id}: {size_read}")
    indices = [(x, y) for x in range(0, xmax, size_read[0]) for y in range(0, ymax, size_read[0])]
    np.random.seed(5)
    np.random.shuffle(indices)
    candidates = ((x, y) for x, y in indices if mask[int(x / ratio_x), int(y / ratio_y)] == 1)      # looked up as they are visited
    return candidates, size_read, resize_factor, len(indices)


def embed_slide(slide, model, *, patch_size, max_patches_per_slide, max_patch_number, n_clusters, random_state=0, feat_type,
                resize, device, batch=256, slide_mask="host", background_threshold=0.2, mask_path=None, slide_id=None):
    """Slide regions -> patch features -> cluster tokens without a patch store: what ``extract_patches(device=...)``,
    ``cli.compute_features`` and ``cli.kmean_features`` compute one after another through two sets of files, with the kept
    tiles staying on `device`.  The candidate walk is extract_patches's (same mask, seed-5 order, cap and read-error rule: a
    failing read prints the error and the tiles kept before it still count); the kept tiles are put in the order in which
    the patch file's ``keys()`` would list their ``"{x}_{y}"`` datasets (``store.key_order``), cut to ``max_patch_number`` by
    ``random.sample`` on that list exactly where cli.compute_features cuts (``features.sample_keys``: seed ``random`` as that
    CLI does to get its rows), embedded by ``model.extract_patches_u8`` (``features.patch_features``; `feat_type`, `resize`
    as the CLI's flags) and clustered by ``kmeans_fit`` when there are at least `n_clusters` of them.
    ``patch_size``: an int or (w, h) as extract_patches takes it; ``max_patches_per_slide`` may be None (no cap).
    Returns a dict: ``coords`` int32 [n, 2] numpy (x, y of each row), ``features`` f32 [n, D], ``labels`` i32 [n] and
    ``cluster_features`` f32 [n_clusters, D] device tensors -- the last two None below `n_clusters` rows, ``features`` None
    when no tile was kept.  Writes ``<mask_path>/<slide_id>/mask.npy`` when ``mask_path`` is given and nothing else."""
    import torch
    from . import features as steps, imgproc
    if device is None:
        raise ValueError("embed_slide needs device=")
    if mask_path is not None and slide_id is None:
        raise ValueError("embed_slide: mask_path needs slide_id (the mask goes to <mask_path>/<slide_id>/mask.npy)")
    patch_size = (int(patch_size), int(patch_size)) if isinstance(patch_size, int) else tuple(patch_size)
    _check_device_request(slide, patch_size, device, batch, slide_mask)
    mask_file = None
    if mask_path is not None:
        os.makedirs(os.path.join(mask_path, slide_id), exist_ok=True)
        mask_file = os.path.join(mask_path, slide_id, "mask.npy")
    coords, chunks = [], []
    try:          # as extract_patches: an unreadable slide prints its error; what was kept before it stays
        candidates, size_read, resize_factor, n_grid = _candidate_walk(slide, slide_id, patch_size, slide_mask, device, mask_file)
        budget = n_grid if max_patches_per_slide is None else int(max_patches_per_slide)
        for xy, tiles in _kept_on_device(slide, list(candidates), size_read, patch_size, resize_factor, background_threshold, budget,
                                         device, int(batch)):
            coords += xy
            chunks.append(tiles)
    except Exception as e:
        print("error with slide id {} patch {}".format(slide_id, len(coords)))
        print(e)
    names = [f"{x}_{y}" for x, y in coords]
    row_of = {name: i for i, name in enumerate(names)}
    order = [row_of[key] for key in steps.sample_keys(store.key_order(names), max_patch_number)]
    out = dict(coords=np.array([coords[i] for i in order], dtype=np.int32).reshape(-1, 2), features=None, labels=None,
               cluster_features=None)
    if not order:
        return out
    tiles = chunks[0] if len(chunks) == 1 else torch.cat(chunks)
    patches = imgproc.pack_rgb(tiles, index=torch.tensor(order, dtype=torch.int32, device=tiles.device))
    del tiles, chunks
    out["features"] = steps.patch_features(model, patches, feat_type, resize, device)
    if out["features"].shape[0] >= n_clusters:
        r = steps.cluster(out["features"], n_clusters, random_state=random_state)
        out["labels"], out["cluster_features"] = r["labels"][0], r["cluster_features"][0]
    return out


def extract_patches(slide, mask_path, patch_size, patches_output_dir, slide_id, max_patches_per_slide=2000,
                    background_threshold=0.2, device=None, batch=256, slide_mask="host"):
    """patch_gen_hdf5.py:51-137 for an already opened slide.  Returns the number of patches written (None when the slide
    had been completed before).  ``device`` (a CUDA device) runs the per-tile filter and the 40x shrink there, `batch`
    candidate tiles at a time (``filter_patches``, ``imgproc.resize_u8_pil``); the slide mask and the visiting order stay
    on the host, and the datasets, ``mask.npy`` and ``complete.txt`` are the host path's byte for byte.  Up to batch - 1
    more regions than the host path may be read near the cap; none of them is written.  ``slide_mask="device"`` (needs
    ``device``) also computes the slide mask and its closing there (``slide_mask``, ``sq_slide_mask``) from the same level
    image; ``mask.npy`` keeps the host path's header and bytes.  The level image must be within the library's bounds
    (extents up to 32768, 2^30 pixels)."""
    _check_device_request(slide, patch_size, device, batch, slide_mask)
    patch_folder = os.path.join(patches_output_dir, slide_id)
    os.makedirs(patch_folder, exist_ok=True)
    mask_folder = os.path.join(mask_path, slide_id)
    os.makedirs(mask_folder, exist_ok=True)
    if os.path.exists(os.path.join(patch_folder, "complete.txt")):
        print(f'{slide_id}: patches have already been extreacted')
        return None
    hdf = store.File(os.path.join(patch_folder, f"{slide_id}.hdf5"), 'w')
    n_written = 0
    try:          # patch_gen_hdf5.py:78,135-137: one unreadable slide prints its error and must not end the whole run
        candidates, size_read, resize_factor, n_grid = _candidate_walk(slide, slide_id, patch_size, slide_mask, device,
                                                                       os.path.join(mask_folder, "mask.npy"))
        if max_patches_per_slide is None:
            max_patches_per_slide = n_grid
        if device is None:
            kept = _filtered_on_host(slide, candidates, size_read, patch_size, resize_factor, background_threshold)
        else:
            kept = _filtered_on_device(slide, list(candidates), size_read, patch_size, resize_factor, background_threshold,
                                       max_patches_per_slide, device, int(batch))
        while n_written < max_patches_per_slide:           # the host path reads no region once the cap is met
            found = next(kept, None)
            if found is None:
                break
            (x, y), patch = found
            hdf.create_dataset(f"{x}_{y}", data=np.ascontiguousarray(patch))
            n_written += 1
    except Exception as e:
        print("error with slide id {} patch {}".format(slide_id, n_written))
        print(e)
        return None
    finally:
        hdf.close()
    if n_written == 0:
        print("no patch extracted for slide {}".format(slide_id))
    else:
        with open(os.path.join(patch_folder, "complete.txt"), 'w') as f:
            f.write('Process complete!\n')
            f.write(f"Total n patch = {n_written}")
        print(f"{slide_id} complete, total n patch = {n_written}")
    return n_written
