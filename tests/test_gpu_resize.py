"""imgproc.resize_u8_pil (sq_resize_u8, csrc/resize.hip) against PIL.Image.resize: every byte equal, for the sizes and
filters the reference resizes with (tests/resize_cases.py; golden outputs made by Pillow, tests/golden/pil_resize.npz)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resize_cases as rc  # noqa: E402
from sequoia_pub_amd import _lib, imgproc  # noqa: E402
from sequoia_pub_amd.uni import resize_u8  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(rc.GOLDEN)


@pytest.mark.parametrize("index", range(len(rc.CASES)), ids=[c[0] for c in rc.CASES])
def test_bit_equal_to_pillow(golden, index):
    _lib.require_gpu()
    _, _, size, resample = rc.CASES[index]
    got = imgproc.resize_u8_pil(torch.from_numpy(rc.case_inputs(index)).cuda(), size, resample)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, size[0], size[1], 3) and got.is_contiguous()
    rc.assert_matches_golden(golden, index, got.cpu().numpy())


def test_int_size_and_non_square_input(golden):
    """size=224 is (224, 224) -- what Resize(224) gives a square patch; a 300 x 411 input goes through both forms."""
    _lib.require_gpu()
    index = [c[0] for c in rc.CASES].index("bilinear_300x411_224")
    x = torch.from_numpy(rc.case_inputs(index)).cuda()
    assert tuple(x.shape) == (2, 300, 411, 3)
    got = imgproc.resize_u8_pil(x, 224)
    rc.assert_matches_golden(golden, index, got.cpu().numpy())
    assert torch.equal(got, imgproc.resize_u8_pil(x, (224, 224), "bilinear"))
    # a view that is not contiguous resizes like its contiguous copy
    wide = torch.zeros(2, 300, 500, 3, dtype=torch.uint8, device="cuda")
    wide[:, :, :411] = x
    assert torch.equal(imgproc.resize_u8_pil(wide[:, :, :411], 224), got)


def _noise_batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g)


@pytest.mark.parametrize("case", ["bilinear_256_224", "bicubic_331_224"])
def test_batch_invariance(golden, case):
    """Image i gives the same bytes alone, in a batch of 7 and in a batch of 130 (331 x 331 x 3 is odd: every image of the
    batch starts at another alignment)."""
    _lib.require_gpu()
    index = [c[0] for c in rc.CASES].index(case)
    _, (h, _), size, resample = rc.CASES[index]
    x = _noise_batch(130, h, 3).cuda()
    x[5] = torch.from_numpy(rc.case_inputs(index)[0]).cuda()
    big = imgproc.resize_u8_pil(x, size, resample)
    seven = imgproc.resize_u8_pil(x[:7], size, resample)
    assert torch.equal(big[:7], seven)
    for i in (0, 5, 6, 64, 129):
        assert torch.equal(imgproc.resize_u8_pil(x[i:i + 1], size, resample)[0], big[i]), i
    assert not (rc.row_digests(big[5].cpu().numpy()) != golden[case + "/noise_rows"]).any()      # and they are Pillow's bytes


def test_thousand_patches_equal_single_calls():
    _lib.require_gpu()
    x = _noise_batch(1000, 256, 11).cuda()
    out = imgproc.resize_u8_pil(x, 224)
    assert tuple(out.shape) == (1000, 224, 224, 3)
    for i in (0, 1, 255, 256, 499, 777, 998, 999):
        assert torch.equal(imgproc.resize_u8_pil(x[i:i + 1], 224)[0], out[i]), i


def test_non_default_stream(golden):
    _lib.require_gpu()
    index = 0
    _, _, size, resample = rc.CASES[index]
    x = torch.from_numpy(rc.case_inputs(index)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = imgproc.resize_u8_pil(x, size, resample)
    s.synchronize()
    rc.assert_matches_golden(golden, index, got.cpu().numpy())


def test_arguments_are_checked():
    _lib.require_gpu()
    x = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SequoiaHipError, match="CUDA"):
        imgproc.resize_u8_pil(x.cpu(), 8)
    with pytest.raises(ValueError):
        imgproc.resize_u8_pil(x.float(), 8)
    with pytest.raises(ValueError):
        imgproc.resize_u8_pil(x[..., :2], 8)
    with pytest.raises(ValueError):
        imgproc.resize_u8_pil(x, 8, "lanczos")
    with pytest.raises(_lib.SequoiaHipError, match="extent"):
        imgproc.resize_u8_pil(x, (8, 0))
    assert tuple(imgproc.resize_u8_pil(x[:0], 8).shape) == (0, 8, 8, 3)


def test_live_against_pillow_on_odd_sizes():
    """Sizes off the golden list, where Pillow imports: small and wide images, more than 256 output columns, tap counts
    beyond the register forms of the kernel (ksize > 9)."""
    Image = pytest.importorskip("PIL.Image")
    _lib.require_gpu()
    rng = np.random.default_rng(5)
    shapes = [((5, 7), (3, 4)), ((64, 64), (7, 300)), ((37, 1030), (33, 515)), ((700, 90), (100, 45)), ((17, 19), (40, 41)),
              ((1, 1), (3, 2)), ((128, 128), (128, 128))]
    for (h_in, w_in), (h_out, w_out) in shapes:
        for resample, pil in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
            x = np.stack([rc.noise(h_in, w_in, int(rng.integers(1 << 30))) for _ in range(3)])
            want = np.stack([np.asarray(Image.fromarray(im, "RGB").resize((w_out, h_out), pil)) for im in x])
            got = imgproc.resize_u8_pil(torch.from_numpy(x).cuda(), (h_out, w_out), resample).cpu().numpy()
            assert np.array_equal(got, want), ((h_in, w_in), (h_out, w_out), resample, int((got != want).sum()))


def test_float_path_is_not_pillow_exact(golden):
    """Why resize_u8_pil exists: uni.resize_u8 (float interpolate, rounded) is not Pillow's fixed-point result.  This
    records the count on the 256 -> 224 noise case; it holds whatever the count is, a float path made exact included."""
    _lib.require_gpu()
    x = torch.from_numpy(rc.case_inputs(0)[:1]).cuda()
    want = golden["bilinear_256_224/noise"]
    flt = resize_u8(x, 224)[0].cpu().numpy()
    differ = int((flt != want).sum())
    worst = int(np.abs(flt.astype(np.int16) - want.astype(np.int16)).max())
    print(f"uni.resize_u8 vs Pillow, 256 -> 224 noise: {differ} of {want.size} bytes differ ({100.0 * differ / want.size:.1f} %), by at most {worst}")
    exact = imgproc.resize_u8_pil(x, 224)[0].cpu().numpy()
    assert np.array_equal(exact, want), f"resize_u8_pil differs from Pillow (the float path differs in {differ} bytes, by at most {worst})"
