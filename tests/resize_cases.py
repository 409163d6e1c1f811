"""Cases and seeded inputs of the Pillow-exact resize tests (tests/golden/pil_resize.npz holds only the expected outputs,
in the layout tests/golden/make_pil_resize_golden.py describes; the inputs are regenerated here).  Shared by tests/golden/make_pil_resize_golden.py, tests/test_resize_plan.py,
tests/test_gpu_resize.py and tests/test_gpu_resize_cli.py."""
import hashlib
import os

import numpy as np

# name, (h_in, w_in), (h_out, w_out), filter
CASES = [
    ("bilinear_256_224", (256, 256), (224, 224), "bilinear"),        # compute_features_hdf5.py:54 on the default 256-px patches
    ("bilinear_512_224", (512, 512), (224, 224), "bilinear"),        # visualize.py:226-230 on a 40x slide
    ("bilinear_512_256", (512, 512), (256, 256), "bilinear"),
    ("bilinear_200_224", (200, 200), (224, 224), "bilinear"),        # upsampling
    ("bilinear_300x411_224", (300, 411), (224, 224), "bilinear"),    # non-square input
    ("bilinear_256_256x265", (256, 256), (256, 265), "bilinear"),    # visualize.py:213; the vertical pass is skipped
    ("bicubic_512_256", (512, 512), (256, 256), "bicubic"),          # patch_gen_hdf5.py:117 on a 40x region
    ("bicubic_331_224", (331, 331), (224, 224), "bicubic"),
]
FILTER_IDS = {"bilinear": 0, "bicubic": 1}        # SQ_RESIZE_BILINEAR, SQ_RESIZE_BICUBIC
FULL_NOISE = ("bilinear_256_224", "bicubic_512_256")        # the noise output is stored whole (the other cases: row digests)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil_resize.npz")


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def structured(h, w, seed):
    """Gradients, a checkerboard and a modular ramp (along x in the left half, along y in the right half): full-range edges
    (bicubic overshoot clamps at both ends), smooth slopes (rounding ties) and periods that beat against the resampling grid
    of either pass."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cell = int(rng.integers(3, 9))
    img = np.empty((h, w, 3), dtype=np.uint8)
    img[..., 0] = (xx * 255) // max(w - 1, 1)
    board = (((yy // cell) + (xx // cell)) & 1) * 255
    img[..., 1] = np.where(yy < h // 2, board, (yy * 255) // max(h - 1, 1))
    a, b = int(rng.integers(5, 12)), int(rng.integers(11, 19))
    img[..., 2] = np.where(xx < w // 2, (xx * a) % 256, (yy * b) % 256)
    return img


def case_inputs(index):
    """uint8 [2, h_in, w_in, 3]: image 0 uniform noise, image 1 structured."""
    _, (h, w), _, _ = CASES[index]
    return np.stack([noise(h, w, 1000 + index), structured(h, w, 2000 + index)])


def row_digests(img):
    """uint8 [h, 32]: SHA-256 of every row of a uint8 [h, w, 3] image."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return np.stack([np.frombuffer(hashlib.sha256(row.tobytes()).digest(), dtype=np.uint8) for row in img])


def assert_matches_golden(golden, index, got, what=""):
    """got: uint8 [2, h_out, w_out, 3] for case_inputs(index); every byte must equal Pillow's."""
    name = CASES[index][0]
    got = np.asarray(got)
    want = golden[name + "/structured"].transpose(1, 2, 0)
    assert got[1].shape == want.shape, (name, got[1].shape, want.shape)
    bad = int((got[1] != want).sum())
    worst = int(np.abs(got[1].astype(np.int16) - want.astype(np.int16)).max())
    assert bad == 0, f"{what}{name} structured: {bad} of {want.size} bytes differ from Pillow (largest difference {worst})"
    rows = np.flatnonzero((row_digests(got[0]) != golden[name + "/noise_rows"]).any(axis=1))
    assert rows.size == 0, f"{what}{name} noise: {rows.size} of {got[0].shape[0]} rows differ from Pillow (first: {rows[:8].tolist()})"
    if name in FULL_NOISE:
        assert np.array_equal(got[0], golden[name + "/noise"]), name
