"""The host half of the Pillow-exact resize (sq_resize_plan_bytes / sq_resize_plan_init, csrc/resize.hip): the coefficient
tables the library computes in double precision, applied in numpy integer arithmetic exactly as the kernel applies them,
must reproduce PIL.Image.resize bit for bit (tests/golden/pil_resize.npz, made by tests/golden/make_pil_resize_golden.py).
No GPU: this pins the double-precision table code and the plan layout of include/sequoia_hip.h."""
import ctypes

import numpy as np
import pytest

import resize_cases as rc
from sequoia_pub_amd import _lib, imgproc


def split_plan(plan, h_in, w_in, h_out, w_out, flt):
    """The int32 words of include/sequoia_hip.h's plan -> ((bounds, coefs) horizontal, (bounds, coefs) vertical)."""
    head = plan[:8].tolist()
    assert head[:5] == [h_in, w_in, h_out, w_out, flt] and head[7] == 0
    ks_h, ks_v = head[5], head[6]
    p = 8
    hb = plan[p:p + 2 * w_out].reshape(w_out, 2); p += 2 * w_out
    hc = plan[p:p + w_out * ks_h].reshape(w_out, ks_h); p += w_out * ks_h
    vb = plan[p:p + 2 * h_out].reshape(h_out, 2); p += 2 * h_out
    vc = plan[p:p + h_out * ks_v].reshape(h_out, ks_v); p += h_out * ks_v
    assert p == plan.size
    return (hb, hc), (vb, vc)


def one_pass(img, bounds, coefs, n_in):
    """Resample axis 1 of uint8 [a, n_in, 3]: acc = 2^21 + sum k[i] src[xmin + i] in int32, out = clamp(acc >> 22)."""
    assert img.shape[1] == n_in
    out = np.empty((img.shape[0], bounds.shape[0], 3), dtype=np.uint8)
    for xx, (xmin, n) in enumerate(bounds.tolist()):
        assert 0 <= xmin and 1 <= n <= coefs.shape[1] and xmin + n <= n_in
        assert not coefs[xx, n:].any()                                  # zero beyond n: the kernel's register taps rely on it
        acc = (1 << 21) + np.tensordot(img[:, xmin:xmin + n, :].astype(np.int64), coefs[xx, :n].astype(np.int64), axes=([1], [0]))
        assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31             # stays inside the kernel's int32
        out[:, xx, :] = np.clip(acc >> 22, 0, 255)
    return out


def resize_with_plan(img, h_out, w_out, resample):
    """Horizontal pass, uint8 intermediate, vertical pass -- with the library's tables."""
    h_in, w_in = img.shape[:2]
    flt = rc.FILTER_IDS[resample]
    (hb, hc), (vb, vc) = split_plan(imgproc.resize_plan(h_in, w_in, h_out, w_out, resample), h_in, w_in, h_out, w_out, flt)
    mid = one_pass(img, hb, hc, w_in)
    return one_pass(mid.transpose(1, 0, 2), vb, vc, h_in).transpose(1, 0, 2)


@pytest.mark.parametrize("index", range(len(rc.CASES)), ids=[c[0] for c in rc.CASES])
def test_plan_tables_reproduce_pillow(index):
    _, _, (h_out, w_out), resample = rc.CASES[index]
    golden = np.load(rc.GOLDEN)
    got = np.stack([resize_with_plan(im, h_out, w_out, resample) for im in rc.case_inputs(index)])
    rc.assert_matches_golden(golden, index, got)


def test_identity_pass_has_one_tap():
    """A pass whose extents are equal is skipped by Pillow; the plan says the same with ksize 1, coefficient 2^22."""
    (hb, hc), (vb, vc) = split_plan(imgproc.resize_plan(256, 256, 256, 265, "bilinear"), 256, 256, 256, 265, 0)
    assert vc.shape == (256, 1) and (vc == 1 << 22).all() and np.array_equal(vb, np.stack([np.arange(256), np.ones(256, int)], 1))
    assert hc.shape == (265, 3)


def test_coefficients_fit_the_kernels_24_bit_multiply():
    for (h_in, w_in), (h_out, w_out), resample in [((331, 331), (224, 224), "bicubic"), ((200, 200), (224, 224), "bicubic"),
                                                   ((7, 9), (40, 33), "bicubic"), ((1000, 3), (7, 5), "bicubic")]:
        plan = imgproc.resize_plan(h_in, w_in, h_out, w_out, resample)
        (_, hc), (_, vc) = split_plan(plan, h_in, w_in, h_out, w_out, 1)
        assert max(np.abs(hc).max(), np.abs(vc).max()) < 1 << 23
        assert max(np.abs(hc).sum(1).max(), np.abs(vc).sum(1).max()) * 255 + (1 << 21) < 2 ** 31


def test_error_paths():
    L = _lib.lib()
    imgproc.resize_plan(8, 8, 4, 4)                                   # binds the signatures
    buf = (ctypes.c_int32 * 4096)()
    for args, word in [((0, 8, 4, 4, 0), b"extent"), ((8, 8, 4, 0, 0), b"extent"), ((8, 8, 4, 4, 2), b"filter"),
                       ((8, 8, 4, 4, -1), b"filter"), ((8, 20000, 4, 4, 1), b"extent")]:
        assert L.sq_resize_plan_bytes(*args) == 0 and word in L.sq_last_error()
        assert L.sq_resize_plan_init(*args, buf, ctypes.sizeof(buf)) != 0 and word in L.sq_last_error()
    need = L.sq_resize_plan_bytes(8, 8, 4, 4, 0)
    assert need == 4 * (8 + 4 * (2 + 5) + 4 * (2 + 5))
    assert L.sq_resize_plan_init(8, 8, 4, 4, 0, buf, need - 4) != 0 and b"bytes" in L.sq_last_error()
    assert L.sq_resize_plan_init(8, 8, 4, 4, 0, None, need) != 0 and b"null" in L.sq_last_error()
    # the launcher checks its arguments before it touches the device
    for args, word in [((None, 1, 8, 8, None, 4, 4, 0, None, None), b"null"), ((buf, 1, 8, 8, buf, 4, 4, 0, None, None), b"plan"),
                       ((buf, 1, 8, 8, buf, 4, 4, 7, buf, None), b"filter"), ((buf, 1, 8, 0, buf, 4, 4, 0, buf, None), b"extent"),
                       ((buf, 0, 8, 8, buf, 4, 4, 0, buf, None), b"images")]:
        assert L.sq_resize_u8(*args) != 0 and word in L.sq_last_error(), args
    with pytest.raises(ValueError):
        imgproc.resize_plan(8, 8, 4, 4, "lanczos")
    with pytest.raises(_lib.SequoiaHipError, match="extent"):
        imgproc.resize_plan(8, 8, 0, 4)


def test_live_against_pillow_on_random_sizes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for _ in range(6):
        h_in, w_in, h_out, w_out = (int(v) for v in rng.integers(5, 120, 4))
        for resample, pil in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
            img = rc.noise(h_in, w_in, int(rng.integers(1 << 30)))
            want = np.asarray(Image.fromarray(img, "RGB").resize((w_out, h_out), pil))
            got = resize_with_plan(img, h_out, w_out, resample)
            assert np.array_equal(got, want), (h_in, w_in, h_out, w_out, resample, int((got != want).sum()))
