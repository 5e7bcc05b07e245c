"""Restatement of the 8-bit convolution resize the device computes (csrc/resize.hip): Pillow's `Image.resize` for
RGB8 with the Hamming and Lanczos3 filters, horizontal pass first ALWAYS, as `resize_for_embed_sync` (src/common.rs:31-54) calls it.
Filter weights in double with `math.sin` / `math.cos` (libm), integer coefficients of 22 fractional bits, int32 sums.  numpy is
used for the integer sums only, which are order-free."""
import functools
import math

import numpy as np

AUTO, HAMMING, LANCZOS3 = 0, 1, 2
PRECISION_BITS = 22
SUPPORT = {HAMMING: 1.0, LANCZOS3: 3.0}
_A = float(np.float32(0.54))        # the float32 constants of the Hamming window, widened
_B = float(np.float32(0.46))


def hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_A + _B * math.cos(x))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos3(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


FILTER = {HAMMING: hamming, LANCZOS3: lanczos3}


def pick_filter(w, h, out_w, out_h, filt=AUTO):
    """common.rs:44: Hamming when both sides shrink, Lanczos3 otherwise; one filter for both passes."""
    if filt != AUTO:
        return filt
    return HAMMING if (w > out_w and h > out_h) else LANCZOS3


@functools.lru_cache(maxsize=None)
def coeffs(n_in, n_out, filt):
    """(ksize, bounds int32 [n_out][2] = (first input, taps), coefs int32 [n_out][ksize], zero past the taps)."""
    f = FILTER[filt]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), np.int32)
    coefs = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            coefs[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    bounds.setflags(write=False)
    coefs.setflags(write=False)
    return ksize, bounds, coefs


def bounds(n_in, n_out, filt):
    """(ksize, bounds) alone, without the filter weights: what decides the kernels' tiling."""
    scale = n_in / n_out
    support = SUPPORT[filt] * max(scale, 1.0)
    center = (np.arange(n_out) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    return 2 * int(math.ceil(support)) + 1, np.stack([xmin, xmax - xmin], axis=1).astype(np.int32)


def _pass(img, n_out, filt, axis):
    """One pass along `axis` (0 = vertical, 1 = horizontal) of a [h][w][3] uint8 image."""
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    _, bounds, coefs = coeffs(a.shape[0], n_out, filt)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    for xx in range(n_out):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coefs[xx, :n].astype(np.int64), a[xmin:xmin + n], axes=(0, 0))
        assert np.abs(acc).max() < (1 << 31)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, out_w, out_h, filt=AUTO):
    """img: [h][w][3] uint8 -> [out_h][out_w][3] uint8."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    filt = pick_filter(w, h, out_w, out_h, filt)
    if w != out_w:
        img = _pass(img, out_w, filt, 1)
    if h != out_h:
        img = _pass(img, out_h, filt, 0)
    return np.ascontiguousarray(img)


def to_nchw_f16(u8_hwc):
    """The tower's input of one or more resized images: x / 127.5 - 1 in fp32, fp16 round-to-nearest-even, NCHW."""
    a = np.asarray(u8_hwc, np.uint8).astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    return np.ascontiguousarray(np.moveaxis(a, -1, -3)).astype(np.float16)


def pil_filter(filt):
    from PIL import Image
    return {HAMMING: Image.HAMMING, LANCZOS3: Image.LANCZOS}[filt]


def pil_resize(img, out_w, out_h, filt=AUTO):
    """Pillow's result with the horizontal pass first: Image.resize itself runs the vertical pass first for very tall images
    (h > 100 w with a shrinking height, e.g. 8 x 900), so the two passes are made as two calls."""
    from PIL import Image
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    f = pil_filter(pick_filter(w, h, out_w, out_h, filt))
    im = Image.fromarray(img, "RGB")
    if w != out_w:
        im = im.resize((out_w, h), f)
    if h != out_h:
        im = im.resize((out_w, out_h), f)
    return np.asarray(im, np.uint8)


def random_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def stripes(w, h):
    """Columns alternating 0 and 255, every third row inverted: drives the Lanczos lobes past both clamps."""
    col = (np.arange(w) % 2) * 255
    a = np.broadcast_to(col[None, :, None], (h, w, 3)).astype(np.uint8).copy()
    a[::3] = 255 - a[::3]
    return a


# (width, height, pixels) at which this restatement was compared with Pillow at 384 x 384; the filter is the AUTO rule's
HAMMING_SHAPES = ([(385, 385, "random"), (400, 500, "random"), (640, 480, "random"), (1000, 777, "random"), (1234, 567, "random"),
                   (777, 1999, "random"), (1920, 1080, "random"), (2049, 385, "random"), (2049, 385, "random1"), (2049, 385, "random2"),
                   (3000, 385, "random"), (385, 3000, "random"), (3001, 2001, "random"), (4000, 3000, "random"), (8191, 385, "random"),
                   (385, 385, "stripes")])
LANCZOS_SHAPES = ([(1, 1, "random"), (3, 2, "stripes"), (383, 383, "random"), (383, 383, "stripes"), (385, 384, "random"),
                   (384, 385, "random"), (384, 1200, "random"), (1200, 384, "random"), (100, 50, "random"), (100, 200, "random"),
                   (200, 100, "random"), (500, 3, "random"), (900, 5, "random"), (900, 7, "random"), (900, 300, "random"),
                   (7, 100, "random"), (7, 385, "random"), (7, 500, "random")] +
                  [(w, 900, "random") for w in range(9, 65)] + [(8, 900, "random"), (40, 3000, "random")])


def make_image(w, h, pixels, seed=0):
    if pixels == "stripes":
        return stripes(w, h)
    return random_image(w, h, seed + 1000 * w + h + (int(pixels[6:]) if len(pixels) > 6 else 0) * 7919)
