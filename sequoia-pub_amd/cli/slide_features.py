"""WSI -> patch features -> cluster tokens in one pass, without a patch store: what ``cli.patch_gen_hdf5 --filter device``,
``cli.compute_features`` and ``cli.kmean_features`` leave under ``--feature_path`` when run one after another --
``<feature_path>/<project>/<WSI>/<WSI>.h5`` with ``"{feat_type}_features"`` [n, D] and ``cluster_features``
[num_clusters, D], and ``complete_tile.txt`` -- plus an int32 ``coords`` [n, 2] dataset (the level-0 x, y of every row).
The kept tiles never leave the GPU (``patchgen.embed_slide``): no ``<patch_path>/<slide>/<slide>.hdf5`` is written, read
back and uploaded again.  The datasets are byte for byte the chain's: same candidate walk and filter, rows in the order the
patch file's keys would have had, ``random.sample`` at the same point with the same ``--seed``, the same extractor and
k-Means calls (``features.py``).  ``--reader tiff`` opens JPEG-tiled TIFF / SVS slides with ``wsi.TiffSlide`` (no openslide; the
tiles are decoded on the GPU and the regions never touch the host).  Flags are those of the three CLIs; ``--mask_path`` (optional here) also writes
``<mask_path>/<slide>/mask.npy``.

    python -m sequoia_pub_amd.cli.slide_features --feat_type resnet --ref_file ref.csv --wsi_path HE \\
        --feature_path features --num_clusters 100 [--mask_path masks] [--slide_mask device]
Slides are the rows of ``--ref_file`` (``<wsi_path>/<wsi_file_name>.svs``, or ``.tiff``), in the order cli.compute_features
visits them; under torchrun the list is sharded across the GPUs like there.  A slide that fails is printed and skipped; a
slide whose reading fails part-way keeps the tiles read before, as the chain does.  Every project's slides are clustered
(cli.kmean_features looks for all of them under the first row's project).  The default reader needs openslide-python."""
import argparse
import os

import numpy as np

from .. import store
from ..data import shard_rows
from ..patchgen import embed_slide
from ..wsi import open_slide                     # the one opener of the slide CLIs: --reader openslide | tiff
from .common import init_distributed, ref_frame, seed_everything
from .compute_features import build_extractor


def build_parser():
    p = argparse.ArgumentParser(description='Slide regions to patch and cluster features without a patch store')
    p.add_argument('--ref_file', type=str, required=True, help='Path with reference csv file')
    p.add_argument('--wsi_path', default="examples/HE", metavar='WSI_PATH', type=str)
    p.add_argument('--mask_path', default=None, metavar='MASK_PATH', type=str, help='also write <mask_path>/<slide>/mask.npy')
    p.add_argument('--patch_size', default=256, type=int)
    p.add_argument('--max_patches_per_slide', default=None, type=int)
    p.add_argument('--start', type=int, default=0, help='Start slide index for parallelization')
    p.add_argument('--end', type=int, default=None, help='End slide index for parallelization')
    p.add_argument('--slide_mask', default='host', choices=['host', 'device'],
                   help="where the whole-slide tissue mask and its closing are computed (as cli.patch_gen_hdf5)")
    p.add_argument('--batch', default=256, type=int, help="candidate tiles read, uploaded and filtered at a time")
    p.add_argument('--reader', default='openslide', choices=['openslide', 'tiff'],
                   help="what opens a slide: openslide = openslide-python; tiff = wsi.TiffSlide (JPEG-tiled TIFF / Aperio SVS without "
                        "openslide, the tiles decoded on the GPU)")
    p.add_argument('--jpeg_entropy', default='serial', choices=['serial', 'split'],
                   help="JPEG tiles of --reader tiff: serial = one lane per tile (sq_jpeg_decode_tiles); split = the 64 lanes of a wave on one tile's scan (sq_jpeg_decode_tiles_split), the same bytes; JPEG 2000 levels and the openslide reader ignore it")
    p.add_argument('--feat_type', default="resnet", type=str, required=True, help='"resnet" or "uni"')
    p.add_argument('--feature_path', type=str, default="/examples/features", help='Output directory to save features')
    p.add_argument('--max_patch_number', type=int, default=4000, help='Max number of patches to use per slide')
    p.add_argument('--compute_dtype', default='fp32', choices=['fp32', 'bf16', 'f16x3', 'bf16x3'], help='as cli.compute_features')
    p.add_argument('--weights', type=str, default=None, help='as cli.compute_features')
    p.add_argument('--resize', default='float', choices=['float', 'pil'], help='as cli.compute_features')
    p.add_argument('--seed', type=int, default=99, help='Seed for random generation')
    p.add_argument("--tcga_projects", help="the tcga_projects we want to use", default=None, type=str, nargs='*')
    p.add_argument('--num_clusters', type=int, default=100)
    return p


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.batch < 1:
        p.error("--batch must be at least 1")
    seed_everything(args.seed)
    rank, world, device = init_distributed()
    model = build_extractor(args, device)
    df = ref_frame(args.ref_file, args.tcga_projects, args.start, args.end)
    lo, hi = shard_rows(df.shape[0], rank, world)
    df = df.iloc[lo:hi]
    print(f'Number of slides = {df.shape[0]} (rank {rank}/{world})')
    feat_name = f"{args.feat_type}_features"
    for _, row in df.iterrows():
        WSI = row['wsi_file_name']
        WSI_slide = WSI.split('.')[0]
        project = row['tcga_project']
        WSI = WSI.replace('.svs', '')
        slide_path = next((q for q in (os.path.join(args.wsi_path, WSI + ext) for ext in ('.svs', '.tiff')) if os.path.exists(q)), None)
        if slide_path is None:
            print('Not exist {}'.format(os.path.join(args.wsi_path, WSI + '.svs')))
            continue
        path_h5 = os.path.join(args.feature_path, project, WSI)
        os.makedirs(path_h5, exist_ok=True)
        if os.path.exists(os.path.join(path_h5, "complete_resnet.txt")):     # (sic) the name cli.compute_features checks
            print(f'{WSI}: Resnet features already obtained')
            continue
        file_h5 = os.path.join(path_h5, WSI + '.h5')
        if store.exists(file_h5):
            with store.File(file_h5, 'r') as f_done:
                done = all(k in f_done.keys() for k in (feat_name, 'coords', 'cluster_features'))
            if done:
                print(f'{WSI}: Cluster feature already available')
                continue
        try:
            r = embed_slide(open_slide(slide_path, args.reader, device, entropy=args.jpeg_entropy), model, patch_size=(args.patch_size, args.patch_size),
                            max_patches_per_slide=args.max_patches_per_slide, max_patch_number=args.max_patch_number,
                            n_clusters=args.num_clusters, random_state=0, feat_type=args.feat_type, resize=args.resize, device=device,
                            batch=args.batch, slide_mask=args.slide_mask, mask_path=args.mask_path, slide_id=WSI_slide)
            if r["features"] is None:
                raise ValueError("need at least one array to stack")          # what the chain's empty patch file ends in
            feats = r["features"].cpu().numpy()
            f_write = store.File(file_h5, "w")
            f_write.create_dataset(feat_name, data=feats)
            f_write.create_dataset("coords", data=np.ascontiguousarray(r["coords"]))
            with open(os.path.join(path_h5, "complete_tile.txt"), 'w') as f_sum:
                f_sum.write(f"Total n patch = {len(feats)}")
            if r["cluster_features"] is None:
                print(f'{WSI} less number of patches than clusters')
            else:
                f_write.create_dataset("cluster_features", data=r["cluster_features"].cpu().numpy())
            f_write.close()
        except Exception as e:                                               # skip the slide, keep going
            print(e)
            print(WSI)
            continue
    print('Done!')


if __name__ == '__main__':
    main()
