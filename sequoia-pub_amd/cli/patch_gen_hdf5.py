"""WSI -> patch HDF5 files -- counterpart of /root/reference/pre_processing/patch_gen_hdf5.py:148-208 (same flags,
same outputs: ``<patch_path>/<slide>/<slide>.hdf5`` + ``complete.txt``, ``<mask_path>/<slide>/mask.npy``).  Reading
real ``.svs`` / ``.tiff`` slides needs openslide-python, exactly like the reference, or ``--reader tiff`` (``wsi.TiffSlide``:
JPEG-tiled TIFF / SVS without openslide, decoded on the GPU, with ``--filter device``); the mask / tiling / filter logic is
sequoia-pub_amd/patchgen.py.  ``--filter device`` runs the per-tile tissue / contrast filter (and the 40x shrink) on the
GPU, ``--filter_batch`` candidate tiles at a time, with the same files as a result; the slides then go through the calling
process one after another -- forked pool workers must not share a process's GPU state -- and ``--parallel`` only prints
that.  ``--slide_mask device`` (with ``--filter device``) also computes the whole-slide tissue mask and its closing on the
GPU (``patchgen.slide_mask``); ``mask.npy`` stays the host's byte for byte."""
import argparse
import os
from multiprocessing import Pool

import pandas as pd

from ..patchgen import extract_patches
from ..wsi import open_slide


def get_slide_id(slide_name):
    return slide_name.split('.')[0]


def process(opts):
    slide_path, patch_size, patches_output_dir, mask_path, slide_id, max_patches_per_slide = opts[:6]
    device, batch, slide_mask = opts[6:9] if len(opts) > 6 else (None, 256, "host")
    slide = open_slide(slide_path, opts[9] if len(opts) > 9 else "openslide", device or "cuda:0",
                       entropy=opts[10] if len(opts) > 10 else "serial")
    extract_patches(slide, mask_path, patch_size, patches_output_dir, slide_id, max_patches_per_slide,
                    device=device, batch=batch, slide_mask=slide_mask)


def build_parser():
    p = argparse.ArgumentParser(description='Generate patches from a given folder of images')
    p.add_argument('--ref_file', default="examples/ref_file.csv", required=False, metavar='ref_file', type=str)
    p.add_argument('--wsi_path', default="examples/HE", metavar='WSI_PATH', type=str)
    p.add_argument('--patch_path', default="examples/Patches_hdf5", metavar='PATCH_PATH', type=str)
    p.add_argument('--mask_path', default="examples/Patches_hdf5", metavar='MASK_PATH', type=str)
    p.add_argument('--patch_size', default=256, type=int)
    p.add_argument('--start', type=int, default=0)
    p.add_argument('--end', type=int, default=None)
    p.add_argument('--max_patches_per_slide', default=None, type=int)
    p.add_argument('--debug', default=0, type=int)
    p.add_argument('--parallel', default=1, type=int)
    p.add_argument('--filter', default='host', choices=['host', 'device'],
                   help="where the per-tile tissue / contrast filter runs: host = numpy as in the reference; device = sq_patch_filter on the GPU "
                        "(always cuda:0; choose another card with HIP_VISIBLE_DEVICES)")
    p.add_argument('--filter_batch', default=256, type=int, help="--filter device: candidate tiles read, uploaded and filtered at a time")
    p.add_argument('--slide_mask', default='host', choices=['host', 'device'],
                   help="where the whole-slide tissue mask and its closing are computed: host = numpy / scipy as in the reference; "
                        "device = sq_slide_mask on the GPU (needs --filter device)")
    p.add_argument('--reader', default='openslide', choices=['openslide', 'tiff'],
                   help="what opens a slide: openslide = openslide-python; tiff = wsi.TiffSlide (JPEG-tiled TIFF / Aperio SVS without "
                        "openslide; the tiles are decoded on the GPU, so it needs --filter device)")
    p.add_argument('--jpeg_entropy', default='serial', choices=['serial', 'split'],
                   help="JPEG tiles of --reader tiff: serial = one lane per tile (sq_jpeg_decode_tiles); split = the 64 lanes of a wave on one tile's scan (sq_jpeg_decode_tiles_split), the same bytes; JPEG 2000 levels and the openslide reader ignore it")
    return p


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.slide_mask == 'device' and args.filter != 'device':
        p.error("--slide_mask device needs --filter device")
    if args.reader == 'tiff' and args.filter != 'device':
        p.error("--reader tiff decodes on the GPU: it needs --filter device")

    slide_list = [s for s in os.listdir(args.wsi_path) if s.endswith('.svs') or s.endswith('.tiff')]
    if args.ref_file:
        wanted = {f'{s}.svs' for s in pd.read_csv(args.ref_file)['wsi_file_name']}
        slide_list = sorted(set(slide_list) & wanted)
    slide_list = slide_list[args.start:args.end] if args.end is not None else slide_list[args.start:]
    if args.debug:
        slide_list = slide_list[0:5]
        args.max_patches_per_slide = 20
    print(f"Found {len(slide_list)} slides")
    opts = [(os.path.join(args.wsi_path, s), (args.patch_size, args.patch_size), args.patch_path, args.mask_path,
             get_slide_id(s), args.max_patches_per_slide) for s in slide_list]
    if args.filter == 'device':
        if args.filter_batch < 1:
            p.error("--filter_batch must be at least 1")
        if args.parallel:
            print("--filter device: slides are processed one after another in this process (--parallel is not used)")
        for o in opts:
            process(o + ("cuda:0", args.filter_batch, args.slide_mask, args.reader, args.jpeg_entropy))
    elif args.parallel:
        with Pool(processes=4) as pool:
            pool.map(process, opts)
    else:
        for o in opts:
            process(o)


if __name__ == '__main__':
    main()
