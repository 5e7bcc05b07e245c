"""Host half of the device resize (`resize_for_embed_sync` of src/common.rs:31-54): the restatement of the arithmetic
(tests/resize_ref.py) against Pillow, bit for bit, and the library's host-side coefficient tables against the restatement.  No GPU."""
import numpy as np
import pytest

import resize_ref as R

GPU_TEST_SIZE = 98     # img_size of the small tower tests/test_gpu_resize.py uses


def _against_pillow(shapes, out):
    bad = []
    for w, h, pixels in shapes:
        img = R.make_image(w, h, pixels)
        got = R.resize(img, out, out)
        want = R.pil_resize(img, out, out)          # Pillow's own two passes, horizontal first (8 x 900: Image.resize would not)
        if h <= 100 * w:                             # ... and the one-call result wherever Pillow keeps that order itself
            from PIL import Image
            one = np.asarray(Image.fromarray(img, "RGB").resize((out, out), R.pil_filter(R.pick_filter(w, h, out, out))))
            assert np.array_equal(one, want), (w, h)
        n = int((got != want).sum())
        if n:
            bad.append((w, h, pixels, n))
    assert not bad, bad


def test_restatement_equals_pillow_hamming_at_384():
    assert all(R.pick_filter(w, h, 384, 384) == R.HAMMING for w, h, _ in R.HAMMING_SHAPES)
    _against_pillow(R.HAMMING_SHAPES, 384)


def test_restatement_equals_pillow_lanczos_at_384():
    assert all(R.pick_filter(w, h, 384, 384) == R.LANCZOS3 for w, h, _ in R.LANCZOS_SHAPES)
    _against_pillow(R.LANCZOS_SHAPES, 384)


def test_restatement_equals_pillow_at_the_small_tower_size(mse):
    """Every tower of the existing SigLIP tests has img_size 384 (the smallest is SO400M_384 at depth 1), which the two tests above
    cover; the device tests run a tower of img_size 98, so the restatement is compared with Pillow there as well."""
    from mse import siglip
    assert siglip.SO400M_384["img_size"] == 384
    s = GPU_TEST_SIZE
    shapes = [(1, 1, "random"), (3, 2, "stripes"), (s - 1, s - 1, "stripes"), (s + 1, s + 1, "stripes"), (s + 1, s, "random"), (s, s + 1, "random"),
              (s, s, "random"), (30, 40, "random"), (300, 50, "random"), (50, 300, "random"), (2100, 99, "random"), (99, 2100, "random"),
              (8, 900, "random"), (641, 479, "random"), (1000, 777, "stripes")]
    _against_pillow(shapes, s)


def _axes(shapes, out):
    for w, h, _ in shapes:
        f = R.pick_filter(w, h, out, out)
        if w != out:
            yield w, out, f
        if h != out:
            yield h, out, f


def test_library_coefficients_equal_the_restatement(mse):
    """mse_resize_coeffs (the host-side tables the kernels read) == the restatement: ksize, bounds and integer coefficients, for every
    (in, out, filter) the verified shapes imply; the size query; the refused arguments."""
    from mse import ffi, siglip
    import ctypes as C
    cases = sorted(set(_axes(R.HAMMING_SHAPES + R.LANCZOS_SHAPES, 384)) | set(_axes(R.HAMMING_SHAPES + R.LANCZOS_SHAPES, GPU_TEST_SIZE)) |
                   {(16384, 384, R.HAMMING), (16384, 384, R.LANCZOS3), (384, 16384, R.LANCZOS3), (16384, 1, R.HAMMING)})
    assert len(cases) > 150
    name = {R.HAMMING: "hamming", R.LANCZOS3: "lanczos3"}
    for n_in, n_out, f in cases:
        ksize, bounds, coefs = siglip.resize_coeffs(n_in, n_out, name[f])
        want_k, want_b, want_c = R.coeffs(n_in, n_out, f)
        assert ksize == want_k and np.array_equal(bounds, want_b) and np.array_equal(coefs, want_c), (n_in, n_out, f)
        assert int(np.abs(coefs.astype(np.int64)).sum(axis=1).max()) * 255 < (1 << 31) - (1 << 21)        # the int32 sum cannot overflow
    assert siglip.resize_coeffs(16384, 384, "hamming")[0] == 87
    k = C.c_int()
    L = ffi.lib()
    for bad in ((0, 384, 1), (16385, 384, 1), (385, 0, 1), (385, 16385, 2), (385, 384, 0), (385, 384, 3)):
        assert L.mse_resize_coeffs(*bad, C.byref(k), None, None) != 0 and "resize" in ffi.last_error(), bad
    assert L.mse_resize_coeffs(385, 384, 1, None, None, None) != 0
    with pytest.raises(mse.MseError):
        siglip.resize_coeffs(385, 384, "bicubic")


def test_library_auto_rule(mse):
    """The C rule itself (mse_resize_pick_filter, what the device path calls): strictly greater on BOTH sides, explicit filters kept."""
    from mse import siglip
    assert siglip.resize_pick_filter(385, 385, 384, 384) == "hamming"
    for w, h in ((385, 384), (384, 385), (384, 384), (384, 1200), (383, 1000), (1200, 383), (1, 1)):
        assert siglip.resize_pick_filter(w, h, 384, 384) == "lanczos3", (w, h)
    assert siglip.resize_pick_filter(500, 300, 400, 200) == "hamming" and siglip.resize_pick_filter(500, 300, 400, 300) == "lanczos3"
    assert siglip.resize_pick_filter(385, 385, 384, 384, "lanczos3") == "lanczos3" and siglip.resize_pick_filter(10, 10, 384, 384, "hamming") == "hamming"
    name = {R.HAMMING: "hamming", R.LANCZOS3: "lanczos3"}
    for w, h, _ in R.HAMMING_SHAPES + R.LANCZOS_SHAPES:
        assert siglip.resize_pick_filter(w, h, 384, 384) == name[R.pick_filter(w, h, 384, 384)], (w, h)
    for bad in ((0, 4, 4, 4), (4, 16385, 4, 4), (4, 4, 0, 4), (4, 4, 4, 16385)):
        with pytest.raises(mse.MseError):
            siglip.resize_pick_filter(*bad)


def test_auto_rule():
    assert R.pick_filter(385, 385, 384, 384) == R.HAMMING
    for w, h in ((385, 384), (384, 1200), (383, 1000)):
        assert R.pick_filter(w, h, 384, 384) == R.LANCZOS3
    # ... and an explicit filter is kept
    assert R.pick_filter(385, 385, 384, 384, R.LANCZOS3) == R.LANCZOS3 and R.pick_filter(10, 10, 384, 384, R.HAMMING) == R.HAMMING
    # the rule decides what is computed: the two filters give different pixels, and the restatement under AUTO is the rule's filter
    img = R.random_image(385, 385, 3)
    assert np.array_equal(R.resize(img, 384, 384), R.resize(img, 384, 384, R.HAMMING))
    assert not np.array_equal(R.resize(img, 384, 384, R.HAMMING), R.resize(img, 384, 384, R.LANCZOS3))
    img = R.random_image(385, 384, 4)
    assert np.array_equal(R.resize(img, 384, 384), R.resize(img, 384, 384, R.LANCZOS3))
