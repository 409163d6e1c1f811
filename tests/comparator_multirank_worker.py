"""Worker of tests/test_gpu_spatial_comparators.py: one of N ranks that SHARE cuda:0, process group over gloo.

    comparator_multirank_worker.py <ok_dir> <vit|he2rna> <nx> <ny> <mode> <batch_windows> <stride> <holes 0|1> <head_chunk> <small|full>
        ONE slide dealt over the ranks (spatial.sliding_window_all_genes_sharded with a ViT or an HE2RNA) against the one-rank
        call in the same process: every rank's rows must be BIT-identical, and sliding_window_method's gathered dictionary too."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sequoia_pub_amd  # noqa: E402,F401


def bits(t):
    return t.contiguous().view(torch.int32)


def main(argv):
    import pandas as pd
    from sequoia_pub_amd import spatial as sp
    ok_dir, model_type, nx, ny, mode, bw, stride, holes, head_chunk, size = (argv[0], argv[1], int(argv[2]), int(argv[3]), argv[4], int(argv[5]),
                                                                            int(argv[6]), argv[7] == "1", int(argv[8]), argv[9])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    sp.HEAD_CHUNK = head_chunk
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    x, y = xs.ravel(), ys.ravel()
    if holes:
        keep = np.random.default_rng(5).random(x.size) < 0.85
        x, y = x[keep], y[keep]
    df = pd.DataFrame({"xcoord_tf": x, "ycoord_tf": y})
    full = size == "full"
    G, D = (20820, 1024) if full else (52, 128)
    torch.manual_seed(31)                                  # the same model and the same slide on every rank
    if model_type == "vit":
        from sequoia_pub_amd.vit import ViT
        m = ViT(num_outputs=G, dim=D, depth=6 if full else 2, heads=16 if full else 2, mlp_dim=2048 if full else 256, device="cuda:0",
                compute_dtype=mode).to("cuda:0").eval()
    else:
        from sequoia_pub_amd.he2rna import HE2RNA
        m = HE2RNA(input_dim=D, output_dim=G, layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100], device="cuda:0").eval()
    g = torch.Generator().manual_seed(32)
    feats = torch.relu(torch.randn(x.size, D, generator=g))
    feats[torch.rand(x.size, generator=g) < 0.03] = 0       # masked tiles (HE2RNA: some windows' k = 1 mean is 0/0 = NaN)
    feats = feats.cuda()

    out_l, ids, votes = sp.sliding_window_all_genes_sharded(x, y, feats, m, stride, batch_windows=bw, shard=(rank, world))
    out_1, votes_1 = sp.sliding_window_all_genes(x, y, feats, m, stride, batch_windows=bw)
    assert torch.equal(votes, votes_1)
    assert out_l.shape == (ids.numel(), G) and out_1.shape == (x.size, G)
    same = torch.equal(bits(out_l), bits(out_1[ids]))      # bit patterns: NaN rows compare equal, -0.0 != 0.0
    covered = int((votes[ids] > 0).sum())
    print(f"{model_type} rank {rank}/{world}: {ids.numel()} of {x.size} tiles ({covered} covered), windows/tile max {int(votes.max())}; "
          f"rows bit-identical to the one-rank run: {same}", flush=True)
    assert same
    if model_type == "vit" and covered:
        assert bool(torch.isfinite(out_l[votes[ids] > 0]).all())
    owned = [None] * world
    dist.all_gather_object(owned, ids.cpu().tolist())
    assert sorted(sum(owned, [])) == list(range(x.size)), "the ranks' tile sets must partition the slide"
    if not full and -(-x.size // head_chunk) < world:
        assert len(owned[-1]) == 0, "this case is meant to leave the last rank without a tile chunk"

    genes = [3, 17, G - 1]
    d_s = sp.sliding_window_method(df, feats, m, genes, stride, batch_windows=bw, shard=(rank, world))
    d_1 = sp.sliding_window_method(df, feats, m, genes, stride, batch_windows=bw)
    for gi in genes:
        assert list(d_s[gi].keys()) == list(d_1[gi].keys()) and len(d_1[gi]) == int((votes > 0).sum())
        a = np.array(list(d_s[gi].values()), dtype=np.float32)
        b = np.array(list(d_1[gi].values()), dtype=np.float32)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"gene {gi}: the gathered dictionary differs from the one-rank one"
    dist.barrier()
    open(os.path.join(ok_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
