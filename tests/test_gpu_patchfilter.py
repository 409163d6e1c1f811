"""patchgen.filter_patches (sq_patch_filter, csrc/patchfilter.hip) against the host filter of patchgen.py, and
extract_patches(device=...) against the host flow: thresholds, masks, counts and every written byte equal, the contrast
ratio within 1e-12 (tests/patchfilter_cases.py holds the cases and their host results)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import patchfilter_cases as pc  # noqa: E402
from sequoia_pub_amd import _lib, patchgen, store  # noqa: E402

SHAPES = list(pc.by_shape().items())


def _run(x):
    keep, stats, raw, dil = patchgen.filter_patches(x, pc.RGB_MIN, pc.BACKGROUND, pc.FRACTION, return_stats=True, return_masks=True)
    assert keep.dtype == torch.bool and stats.dtype == torch.float64 and raw.dtype == torch.bool and dil.dtype == torch.bool
    return keep.cpu().numpy(), stats.cpu().numpy(), raw.cpu().numpy(), dil.cpu().numpy()


def _check_against_host(name, keep, row, raw, dil, golden=None):
    h = pc.host(name)
    want = pc.stats_row(h)
    print(f"{name}: thresholds {row[:4].tolist()} counts {row[4]:.0f} {row[5]:.0f} ratio {row[6]!r} (host {h['ratio']!r}, "
          f"difference {abs(row[6] - h['ratio']):.3e}) keep {bool(keep)}")
    assert np.array_equal(row[:4], want[:4]), (name, row[:4].tolist(), want[:4].tolist())
    assert np.array_equal(raw, h["mask"]), (name, int((raw != h["mask"]).sum()))
    assert np.array_equal(dil, h["dilated"]), (name, int((dil != h["dilated"]).sum()))
    assert row[4] == want[4] == raw.sum() and row[5] == want[5] == dil.sum(), (name, row[4:6].tolist(), want[4:6].tolist())
    assert abs(row[6] - h["ratio"]) <= 1e-12, (name, row[6], h["ratio"])
    assert row[7] == 0.0
    assert bool(keep) == h["keep"], (name, bool(keep), h["keep"])
    if golden is not None:                                  # the scikit-image 0.18.3 values themselves
        assert np.array_equal(row[:4], golden[name + "::thresholds"])
        assert np.array_equal(raw, golden[name + "::mask"]) and np.array_equal(dil, golden[name + "::mask_dilated"])
        assert (row[6] < pc.FRACTION) == bool(golden[name + "::low_contrast"])


@pytest.mark.parametrize("index", range(len(SHAPES)), ids=[f"{h}x{w}" for (h, w), _ in SHAPES])
def test_every_case_equals_the_host_filter(index):
    """The tiles of one shape in one call."""
    _lib.require_gpu()
    _, names = SHAPES[index]
    golden = np.load(pc.GOLDEN)
    keep, stats, raw, dil = _run(torch.from_numpy(np.stack([pc.image(n) for n in names])).cuda())
    for i, n in enumerate(names):
        _check_against_host(n, keep[i], stats[i], raw[i], dil[i], golden if n in pc.GOLDEN_CASES else None)


def test_keep_alone_equals_keep_with_stats():
    _lib.require_gpu()
    names = pc.by_shape()[(64, 64)]
    x = torch.from_numpy(np.stack([pc.image(n) for n in names])).cuda()
    keep = patchgen.filter_patches(x)
    assert torch.is_tensor(keep) and keep.dtype == torch.bool and keep.cpu().tolist() == [pc.host(n)["keep"] for n in names]
    keep2, stats = patchgen.filter_patches(x, return_stats=True)
    assert torch.equal(keep, keep2) and tuple(stats.shape) == (len(names), 8)
    # the thresholds of the call are arguments, not constants of the kernel
    h = pc.host("half_tissue_64")
    i = names.index("half_tissue_64")
    share = float(h["dilated"].sum()) / h["dilated"].size
    assert bool(patchgen.filter_patches(x, background_threshold=share - 1e-3)[i]) and not bool(patchgen.filter_patches(x, background_threshold=share)[i])
    assert not bool(patchgen.filter_patches(x, fraction_threshold=h["ratio"] + 1e-3)[i])
    strict = patchgen.filter_patches(x, rgb_min=255, return_stats=True)[1].cpu().numpy()
    assert (strict[:, 4] == 0).all() and (strict[:, 5] == 0).all()


def _filler(h, w, n, seed):
    """Noise, tissue-like, blank and flat tiles in turn."""
    rs = np.random.RandomState(seed)
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        kind = i % 4
        if kind == 0:
            out[i] = rs.randint(0, 256, (h, w, 3))
        elif kind == 1:
            out[i] = pc._tile(h, w, seed * 1000 + i, pc._columns(h, w, int(rs.randint(0, w // 2)), int(rs.randint(1, w))))
        elif kind == 2:
            out[i] = pc._tile(h, w, seed * 1000 + i)
        else:
            out[i] = pc._tile(h, w, seed * 1000 + i, np.ones((h, w), dtype=bool), spread=2.0)
    return out


@pytest.mark.parametrize("shape", [(33, 47), (64, 64)], ids=["33x47", "64x64"])
def test_batch_invariance(shape):
    """A tile gives the same row, masks and decision alone, in a batch of 7 and in a batch of 300 (more tiles than the chip
    has CUs; 33 x 47 x 3 is odd, so the tiles of a batch start at every alignment).  The planted case tiles also give the
    host's values wherever they stand."""
    _lib.require_gpu()
    h, w = shape
    names = pc.by_shape()[shape]
    x = _filler(h, w, 300, seed=h)
    planted = {}
    for j, at in enumerate((0, 5, 255, 256, 299)):
        planted[at] = names[j % len(names)]
        x[at] = pc.image(planted[at])
    x = torch.from_numpy(x).cuda()
    big = _run(x)
    for start in (0, 5):                                               # x[5:12] starts at another alignment than x[:7]
        seven = _run(x[start:start + 7])
        for got, want in zip(seven, big):
            assert np.array_equal(got, want[start:start + 7]), start
    for i in (0, 1, 5, 6, 255, 256, 298, 299):
        one = _run(x[i:i + 1])
        for got, want in zip(one, big):
            assert np.array_equal(got[0], want[i]), i
    for at, name in planted.items():
        _check_against_host(name, big[0][at], big[1][at], big[2][at], big[3][at])
    assert 0 < big[0].sum() < 300                                      # the filler is a mix of kept and rejected tiles


def test_non_contiguous_input_and_non_default_stream():
    _lib.require_gpu()
    names = pc.by_shape()[(64, 64)]
    x = torch.from_numpy(np.stack([pc.image(n) for n in names])).cuda()
    want = _run(x)
    wide = torch.zeros(len(names), 64, 100, 3, dtype=torch.uint8, device="cuda")
    wide[:, :, 7:71] = x
    for got, ref in zip(_run(wide[:, :, 7:71]), want):
        assert np.array_equal(got, ref)
    for got, ref in zip(_run(x.flip(0)), want):                      # negative stride
        assert np.array_equal(got, ref[::-1])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = patchgen.filter_patches(x, return_stats=True, return_masks=True)
    s.synchronize()
    for g, ref in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), ref)


def test_arguments_are_checked():
    _lib.require_gpu()
    x = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SequoiaHipError, match="CUDA"):
        patchgen.filter_patches(x.cpu())
    with pytest.raises(ValueError):
        patchgen.filter_patches(x.float())
    with pytest.raises(ValueError):
        patchgen.filter_patches(x[0])
    with pytest.raises(ValueError):
        patchgen.filter_patches(x[..., :2])
    with pytest.raises(_lib.SequoiaHipError, match="8..512"):
        patchgen.filter_patches(x[:, :7])
    with pytest.raises(_lib.SequoiaHipError, match="8..512"):
        patchgen.filter_patches(torch.zeros(1, 8, 513, 3, dtype=torch.uint8, device="cuda"))
    keep, stats, raw, dil = patchgen.filter_patches(x[:0], return_stats=True, return_masks=True)
    assert tuple(keep.shape) == (0,) and keep.dtype == torch.bool and tuple(stats.shape) == (0, 8) and tuple(raw.shape) == tuple(dil.shape) == (0, 16, 16)
    assert tuple(patchgen.filter_patches(x[:0]).shape) == (0,)


# ---- extract_patches(device=...) against the host flow ----------------------------------------------------------------
def _slide(seed=0, tiles=(16, 12), ps=32, cls=patchgen.ArraySlide, **kw):
    """tests/test_patchgen.py's slide: left half tissue-like, right half blank; level 1 is 8x smaller."""
    rs = np.random.RandomState(seed)
    W, H = tiles[0] * ps, tiles[1] * ps
    img = np.full((H, W, 3), 242, dtype=np.float64) + rs.randn(H, W, 3) * 2
    tissue = np.zeros((H, W), dtype=bool)
    tissue[:, : W // 2] = True
    img[tissue] = np.array([190, 110, 160]) + rs.randn(int(tissue.sum()), 3) * 25
    img = np.clip(img, 0, 255).astype(np.uint8)
    return cls([img, img[::8, ::8].copy()], **kw)


def _outputs(root, slide_id):
    with store.File(os.path.join(root, "p", slide_id, slide_id + ".hdf5"), "r") as f:
        keys = list(f.keys())
        data = {k: np.asarray(f[k][:]) for k in keys}
    done = os.path.join(root, "p", slide_id, "complete.txt")
    return keys, data, np.load(os.path.join(root, "m", slide_id, "mask.npy")), open(done).read() if os.path.exists(done) else None


def _both(tmp_path, make_slide, patch, **kw):
    """Host run and device run of extract_patches; returns their return values after asserting every output equal."""
    device_kw = {k: kw.pop(k) for k in ("batch",) if k in kw}
    n_host = patchgen.extract_patches(make_slide(), str(tmp_path / "host" / "m"), patch, str(tmp_path / "host" / "p"), "S", **kw)
    n_dev = patchgen.extract_patches(make_slide(), str(tmp_path / "dev" / "m"), patch, str(tmp_path / "dev" / "p"), "S", device="cuda:0",
                                     **kw, **device_kw)
    keys, data, mask, done = _outputs(str(tmp_path / "host"), "S")
    keys2, data2, mask2, done2 = _outputs(str(tmp_path / "dev"), "S")
    assert keys == keys2, (keys, keys2)
    for k in keys:
        assert data[k].dtype == data2[k].dtype == np.uint8 and data[k].shape == data2[k].shape and data[k].tobytes() == data2[k].tobytes(), k
    assert mask.dtype == mask2.dtype and np.array_equal(mask, mask2) and done == done2
    assert n_host == n_dev
    return n_host, keys, done


def test_flow_uncapped(tmp_path):
    _lib.require_gpu()
    n, keys, done = _both(tmp_path, _slide, (32, 32), max_patches_per_slide=None)
    assert n == len(keys) > 50 and done.endswith(f"Total n patch = {n}")


def test_flow_cap_inside_a_chunk(tmp_path):
    _lib.require_gpu()
    n, keys, done = _both(tmp_path, _slide, (32, 32), max_patches_per_slide=3, batch=4)
    assert n == len(keys) == 3 and done.endswith("Total n patch = 3")


def test_flow_batch_of_one(tmp_path):
    _lib.require_gpu()
    n, keys, _ = _both(tmp_path, lambda: _slide(seed=4, tiles=(8, 6)), (32, 32), max_patches_per_slide=None, batch=1)
    assert n == len(keys) > 10


def test_flow_40x_shrinks_on_the_device(tmp_path):
    """aperio.AppMag 40: 32 x 32 regions, filtered, then the device's bicubic resize to 16 x 16 against the host's Pillow call."""
    import PIL.Image  # noqa: F401  (the host path's resize; its absence is a failure, not a skip)
    _lib.require_gpu()
    n, keys, _ = _both(tmp_path, lambda: _slide(seed=2, tiles=(16, 10), properties={"aperio.AppMag": "40"}), (16, 16),
                       max_patches_per_slide=None, batch=16)
    assert n == len(keys) > 20


class _FailingSlide(patchgen.ArraySlide):
    """read_region raises on the k-th level-0 read."""

    def __init__(self, levels, fail_at):
        super().__init__(levels)
        self.fail_at, self.reads = fail_at, 0

    def read_region(self, location, level, size):
        if level == 0:
            self.reads += 1
            if self.reads == self.fail_at:
                raise OSError("tile decode failed")
        return super().read_region(location, level, size)


@pytest.mark.parametrize("fail_at,batch", [(11, 4), (9, 4), (1, 4), (30, 256)])
def test_read_failure_leaves_the_host_paths_datasets(tmp_path, capsys, fail_at, batch):
    """The tiles read before the failing one are filtered and written, then the error is reported as on the host: no
    complete.txt, None returned."""
    _lib.require_gpu()
    n, keys, done = _both(tmp_path, lambda: _slide(seed=3, cls=_FailingSlide, fail_at=fail_at), (32, 32), max_patches_per_slide=None, batch=batch)
    assert n is None and done is None and capsys.readouterr().out.count("error with slide id S") == 2
    assert (len(keys) == 0) == (fail_at == 1)


def test_read_failure_behind_the_cap_is_never_reached(tmp_path):
    """The host loop stops reading at the cap; a chunk may read on (up to batch - 1 regions), and a failure among those is
    not the slide's."""
    _lib.require_gpu()
    n, keys, done = _both(tmp_path, lambda: _slide(seed=3, cls=_FailingSlide, fail_at=6), (32, 32), max_patches_per_slide=2, batch=16)
    assert n == 2 and len(keys) == 2 and done.endswith("Total n patch = 2")
