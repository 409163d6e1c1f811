"""The device-resident cohort feed on the GPU: sq_cohort_gather against torch indexing (both access widths, 64-bit offsets),
ResidentLoader's batches against DataLoader + custom_collate_fn, and the CLIs with ``--feed resident`` against ``--feed loader``
file by file.  Everything is compared for equality: the gather moves bits and the training kernels are deterministic."""
import os
import pickle

import numpy as np
import pandas as pd
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

import cohort_cases as cc  # noqa: E402
from sequoia_pub_amd import _lib  # noqa: E402
from sequoia_pub_amd.data import CohortTable, ResidentLoader, SuperTileRNADataset, cohort_gather, custom_collate_fn  # noqa: E402

DEV = "cuda:0"


def _tables(S, tokens, D, G, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(S, tokens, D, device=DEV, generator=g), torch.randn(S, G, device=DEV, generator=g))


def _index(index):
    return None if index is None else torch.tensor(index, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("S,tokens,D,G,index", cc.GATHER_CASES, ids=lambda v: None if not isinstance(v, list) else "idx" + str(len(v)))
def test_gather_equals_torch_indexing(S, tokens, D, G, index):
    _lib.require_gpu()
    xt, yt = _tables(S, tokens, D, G)
    x, y = cohort_gather(xt, _index(index), yt)
    rows = torch.arange(S, device=DEV) if index is None else torch.tensor(index, device=DEV)
    assert x.shape == (len(rows), tokens, D) and y.shape == (len(rows), G)
    assert torch.equal(x, xt[rows]) and torch.equal(y, yt[rows])
    # features only: no y table, no y output
    x_only, none = cohort_gather(xt, _index(index))
    assert none is None and torch.equal(x_only, xt[rows])


@pytest.mark.parametrize("S,tokens,D,G", cc.GUARD_SHAPES)
def test_out_of_range_rows_are_zero_and_nothing_else_is_written(S, tokens, D, G):
    _lib.require_gpu()
    xt, yt = _tables(S, tokens, D, G, seed=1)
    m, band, mark = len(cc.OUT_OF_RANGE), 64, 12345.0                               # 64 floats: the outputs keep the tables' alignment
    bufs = [torch.full((2 * band + m * t[0].numel(),), mark, device=DEV) for t in (xt, yt)]
    outs = [b[band:b.numel() - band].view((m,) + tuple(t.shape[1:])) for b, t in zip(bufs, (xt, yt))]
    x, y = cohort_gather(xt, _index(cc.OUT_OF_RANGE), yt, x_out=outs[0], y_out=outs[1])
    assert x.data_ptr() == outs[0].data_ptr() and y.data_ptr() == outs[1].data_ptr()
    for out, t, b in ((x, xt, bufs[0]), (y, yt, bufs[1])):
        assert not out[0].any() and not out[1].any() and torch.equal(out[2], t[2])
        assert bool((b[:band] == mark).all()) and bool((b[-band:] == mark).all())


def test_a_table_off_the_16_byte_grid_goes_by_the_dword():
    _lib.require_gpu()
    S, tokens, D, G, index = cc.GATHER_CASES[1]
    xt, yt = _tables(S, tokens, D, G, seed=2)
    shifted = torch.empty(xt.numel() + 1, device=DEV)[1:].view_as(xt)               # a sliced view: 4 bytes past an aligned address
    shifted.copy_(xt)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    x, y = cohort_gather(shifted, _index(index), yt)
    assert torch.equal(x, xt[index]) and torch.equal(y, yt[index])
    out = torch.empty(len(index) * tokens * D + 1, device=DEV)[1:].view(len(index), tokens, D)   # and an output off the grid
    cohort_gather(xt, _index(index), x_out=out)
    assert torch.equal(out, xt[index])


def test_offsets_beyond_two_gib():
    """S = 5300 rows of 100 x 1024 f32 (2.17 GB): row 5242 straddles 2^31 bytes, row 5299 lies beyond.  Only the rows read are
    filled; a 32-bit byte or float offset would fetch another row (or fault)."""
    _lib.require_gpu()
    xt = torch.empty(cc.BIG_S, cc.BIG_TOKENS, cc.BIG_D, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    for r in cc.BIG_ROWS:
        xt[r] = torch.randn(cc.BIG_TOKENS, cc.BIG_D, device=DEV, generator=g)
    yt = torch.arange(cc.BIG_S * 3, device=DEV, dtype=torch.float32).view(cc.BIG_S, 3)
    x, y = cohort_gather(xt, _index(cc.BIG_ROWS), yt)
    for j, r in enumerate(cc.BIG_ROWS):
        assert torch.equal(x[j], xt[r]) and torch.equal(y[j], yt[r]), r
    assert not torch.equal(x[0], x[2])


def _same_batch(mine, real):
    if isinstance(real[0], list) and not real[0]:
        assert tuple(mine) == ([], [], [], []) and tuple(real) == ([], [], [], [])
        return 0
    assert len(mine) == len(real) == 4
    for a, b in zip(mine[:2], real[:2]):
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a, b.to(DEV))
    for a, b in zip(mine[2:], real[2:]):
        assert type(a) is type(b) and a == b and all(type(u) is type(v) for u, v in zip(a, b))
    return len(real[2])


@pytest.mark.parametrize("batch,shuffle,epochs", [(2, False, 1), (4, True, 2)])
def test_batches_equal_the_loader_path(tmp_path, batch, shuffle, epochs):
    _lib.require_gpu()
    frame, feature_path = cc.write_cohort(tmp_path, extra=5)
    table = CohortTable(frame, feature_path).to(DEV)
    assert table.x_dev.is_cuda and torch.equal(table.x_dev.cpu(), torch.from_numpy(table.x)) and torch.equal(table.y_dev.cpu(), torch.from_numpy(table.y))
    rows = np.arange(len(frame))
    real_loader = DataLoader(SuperTileRNADataset(frame, feature_path), batch_size=batch, shuffle=shuffle, num_workers=0, pin_memory=True,
                             collate_fn=custom_collate_fn, generator=torch.Generator().manual_seed(5))
    mine_loader = ResidentLoader(table, rows, batch, shuffle=shuffle, generator=torch.Generator().manual_seed(5))
    assert len(mine_loader) == len(real_loader)
    for _ in range(epochs):
        real, mine = list(real_loader), list(mine_loader)
        assert len(real) == len(mine) == len(real_loader)
        sizes = [_same_batch(a, b) for a, b in zip(mine, real)]
        assert sum(sizes) == len(frame) - 2
        if not shuffle:
            assert sizes[1] == 0 and all(sizes[:1] + sizes[2:])                      # slides 2 and 3: the all-invalid batch
    # a row subset (a fold): table rows 7.., against the dataset of that slice of the frame
    part = np.arange(7, len(frame))
    real = list(DataLoader(SuperTileRNADataset(frame.iloc[part], feature_path), batch_size=batch, collate_fn=custom_collate_fn))
    mine = list(ResidentLoader(table, part, batch))
    assert len(real) == len(mine) and all(_same_batch(a, b) for a, b in zip(mine, real))


# ---------------------------------------------------------------------------------------------------------------------
# the CLIs: --feed resident writes what --feed loader writes
# ---------------------------------------------------------------------------------------------------------------------
TOKENS, WIDTH, GENES, SLIDES, FOLDS = 100, 64, 30, 12, 3       # 64: the smallest input_dim the ViS config check admits
FEEDS = ("loader", "resident")


def _same_value(a, b, where):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same_value(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, pd.DataFrame):
        assert list(a.index) == list(b.index) and list(a.columns) == list(b.columns) and np.array_equal(a.to_numpy(), b.to_numpy()), where
    elif torch.is_tensor(a):
        assert np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy()), where
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), where
    else:
        assert a == b, where


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    root = tmp_path_factory.mktemp("cohort_cli")
    frame, feature_path = cc.write_cohort(root, extra=SLIDES - 7, tokens=TOKENS, dim=WIDTH, genes=GENES, seed=6, odd=False)
    ref = os.path.join(str(root), "ref.csv")
    frame.to_csv(ref, index=False)
    return str(root), ref, feature_path


@pytest.fixture(scope="module")
def trained(cohort):
    """cli.main --train once with each feed; the outputs of both are compared in the first test below."""
    from sequoia_pub_amd.cli import main as train_main
    _lib.require_gpu()
    root, ref, feature_path = cohort
    outs = {}
    for feed in FEEDS:
        train_main.main(["--ref_file", ref, "--feature_path", feature_path, "--save_dir", os.path.join(root, "exp"), "--exp_name", feed,
                         "--train", "--model_type", "vis", "--depth", "1", "--num-heads", "2", "--batch_size", "4", "--num_epochs", "2",
                         "--k", str(FOLDS), "--compute_dtype", "fp32", "--feed", feed])
        outs[feed] = os.path.join(root, "exp", "TCGA", feed)
    return outs


def test_main_writes_the_same_files_with_either_feed(trained):
    files = {feed: sorted(os.listdir(out)) for feed, out in trained.items()}
    assert files["loader"] == files["resident"]
    names = files["loader"]
    assert "test_results.pkl" in names and "model_best.pt" in names and f"model_best_{FOLDS - 1}.pt" in names
    assert all(f"{role}_{i}.npy" in names for role in ("train", "val", "test") for i in range(FOLDS))
    for name in names:
        a, b = (os.path.join(trained[feed], name) for feed in FEEDS)
        if name.endswith(".pt"):
            _same_value(torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu"), name)
        elif name.endswith(".npy"):
            _same_value(np.load(a, allow_pickle=True), np.load(b, allow_pickle=True), name)
        else:
            res = _load(a)
            assert set(res["split_0"]) == {"real", "preds", "random", "wsi_file_name", "tcga_project"}
            assert not np.array_equal(res["split_0"]["preds"], res["split_0"]["random"])
            _same_value(res, _load(b), name)


def test_predict_independent_dataset_writes_the_same_with_either_feed(cohort, trained):
    from sequoia_pub_amd.cli import predict_independent_dataset
    from sequoia_pub_amd.vis import ViS
    root, ref, feature_path = cohort
    for fold in range(2):
        m = ViS(GENES, WIDTH, 1, 2, 64, 64, 64, device="cpu")
        m.load_state_dict(torch.load(os.path.join(trained["resident"], "model_best.pt" if fold == 0 else f"model_best_{fold}.pt")))
        m.save_pretrained(os.path.join(root, "hub", f"sequoia-brca-{fold}"))
    for feed in FEEDS:
        predict_independent_dataset.main(["--ref_file", ref, "--feature_path", feature_path, "--folds", "2", "--tcga_project", "TCGA-BRCA",
                                          "--depth", "1", "--num-heads", "2", "--batch_size", "5", "--save_dir", os.path.join(root, "pred"),
                                          "--exp_name", feed, "--model_dir", os.path.join(root, "hub"), "--feed", feed])
    a, b = (_load(os.path.join(root, "pred", feed, "test_results.pkl")) for feed in FEEDS)
    assert a["pred"].shape == (SLIDES, GENES) and set(a) == {"pred", "random"}
    _same_value(a, b, "test_results.pkl")


def test_he2rna_writes_the_same_with_either_feed(cohort):
    from sequoia_pub_amd.cli import he2rna as he2rna_cli
    _lib.require_gpu()
    root, ref, feature_path = cohort
    outs = {}
    for feed in FEEDS:
        _, outs[feed] = he2rna_cli.main(["--path_csv", ref, "--feature_path", feature_path, "--k", str(FOLDS), "--batch_size", "4",
                                         "--max_epochs", "2", "--patience", "5", "--log", "0", "--destfolder", root, "--subfolder", "he2rna",
                                         "--exp_name", feed, "--engine", "fused", "--feed", feed])
    assert sorted(os.listdir(outs["loader"])) == sorted(os.listdir(outs["resident"]))
    res = _load(os.path.join(outs["loader"], "test_results.pkl"))
    assert res["split_0"]["preds"].shape[1] == GENES and not np.array_equal(res["split_0"]["preds"], res["split_0"]["random"])
    _same_value(res, _load(os.path.join(outs["resident"], "test_results.pkl")), "test_results.pkl")
    for i in range(FOLDS):
        a, b = (torch.load(os.path.join(outs[feed], f"model_{i}.pt"), weights_only=False).state_dict() for feed in FEEDS)
        _same_value(dict(a), dict(b), f"model_{i}.pt")
