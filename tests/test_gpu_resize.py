"""Device resize in front of the image tower (csrc/resize.hip; `resize_for_embed_sync`, src/common.rs:31-54) against the
restatement of its arithmetic (tests/resize_ref.py) and against Pillow: every comparison is bit for bit.  The tower is a small one
(img_size S = 98, one block) whose size plays the role of 384."""
import ctypes as C
import functools
import io
import os
import re
import struct

import numpy as np
import pytest

import resize_ref as R
from conftest import ROOT

S = 98
CSRC = os.path.join(ROOT, "meme-search-engine_amd", "csrc")


def _const(fname, name):
    m = re.search(r"constexpr[^;]*\b" + name + r"\s*=\s*(\d+)", open(os.path.join(CSRC, fname)).read())
    assert m, (fname, name)
    return int(m.group(1))


HT_OX = _const("resize.hip", "HT_OX")                 # output pixels of a horizontal tile (32)
HT_ROWS = _const("resize.hip", "HT_ROWS")             # rows of a horizontal tile (8)
H_SEG_BYTES = _const("resize.hip", "H_SEG_BYTES")     # LDS for a horizontal tile's row segments (40960)
H_COEF_WORDS = _const("resize.hip", "H_COEF_WORDS")   # LDS for a horizontal tile's coefficients (4096 words)
VT_OY = _const("resize.hip", "VT_OY")                 # output rows of a vertical tile (8)
V_THREADS = _const("resize.hip", "V_THREADS")
V_BYTES = _const("resize.hip", "V_BYTES")
VT_XBYTES = V_THREADS * V_BYTES                       # bytes of a row of a vertical tile (256)
SUB_BATCH_IMAGES = _const("resize.h", "SUB_BATCH_IMAGES")   # images of a sub-batch (1024)


def _h_tiles(w, ow, filt, rows):
    """(row segments staged in LDS, coefficients staged in LDS) of every tile of a row band of `rows` rows, as resize_h_kernel decides."""
    k, b = R.bounds(w, ow, filt)
    out = []
    for ox0 in range(0, ow, HT_OX):
        nox = min(HT_OX, ow - ox0)
        seg = (int(b[ox0 + nox - 1].sum()) - int(b[ox0, 0])) * 3
        out.append((((seg + 30) & ~15) * rows <= H_SEG_BYTES, nox * k <= H_COEF_WORDS))
    return out


def _first_width(pred, lo, hi):
    """smallest width in (lo, hi] with pred, by bisection (pred(lo) false, pred(hi) true; test_boundaries_... checks the two sides)"""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


# first widths at which a FULL band of HT_ROWS rows of an S-wide Lanczos3 result has a tile whose segments / coefficients leave LDS
W_SEG = _first_width(lambda w: not all(p for p, _ in _h_tiles(w, S, R.LANCZOS3, HT_ROWS)), 3000, 9000)
W_COEF = _first_width(lambda w: not all(k for _, k in _h_tiles(w, S, R.LANCZOS3, HT_ROWS)), 1000, 9000)


def _cases():
    """(w, h, out_w, out_h, pixels, why)"""
    c = []
    # the stripes go where they reach both clamps (no shrink averages them away): the test asserts that they do
    c += [(3, 2, S, S, "stripes", "3 x 2"), (S - 1, S - 1, S, S, "stripes", "(s-1)^2"), (S + 1, S + 1, S, S, "stripes", "(s+1)^2: Hamming"),
          (S, S + 1, S, S, "stripes", "vertical pass only"), (S, S, S, S, "stripes", "the copy"), (30, 40, S, S, "stripes", "upscale of both sides"),
          (S + 3, 20, S, S, "stripes", "horizontal shrink by a little, vertical growth")]
    for px in ("random",):
        c += [(1, 1, S, S, px, "one pixel"), (3, 2, S, S, px, "3 x 2"), (S - 1, S - 1, S, S, px, "(s-1)^2"), (S + 1, S + 1, S, S, px, "(s+1)^2: Hamming"),
              (S + 1, S, S, S, px, "horizontal pass only"), (S, S + 1, S, S, px, "vertical pass only"), (S, S, S, S, px, "the copy"),
              (30, 40, S, S, px, "upscale of both sides"), (300, 50, S, S, px, "w shrinks, h grows"), (50, 300, S, S, px, "h shrinks, w grows"),
              (2100, 99, S, S, px, "shrink by more than 20 on one side: Hamming, 45 taps"), (99, 2100, S, S, px, "the same, vertical"),
              (8, 900, S, S, px, "h > 100 w: Pillow alone would run the vertical pass first"),
              (333, 211, S, S, px, "999-byte rows: every row starts at another 16-byte phase"), (641, 479, S, S, px, "odd sizes, Hamming")]
    # resize_h_kernel: H_SEG_BYTES and H_COEF_WORDS (a 9-row image has a full band and a one-row band, whose segments still fit)
    c += [(w, HT_ROWS + 1, S, S, "random", "H_SEG_BYTES %+d" % (w - W_SEG)) for w in (W_SEG - 1, W_SEG, W_SEG + 1)]
    c += [(w, HT_ROWS + 1, S, S, "random", "H_COEF_WORDS %+d" % (w - W_COEF)) for w in (W_COEF - 1, W_COEF, W_COEF + 1)]
    c += [(W_SEG + 1, 2 * HT_ROWS, S, S, "random", "segments and coefficients through L2, two full bands")]
    # HT_OX: output widths of one tile, one pixel more, two tiles, ...; HT_ROWS: source heights around a band
    c += [(200, 37, ow, 20, "random", "HT_OX: out_w %d" % ow) for ow in (HT_OX - 1, HT_OX, HT_OX + 1, 2 * HT_OX - 1, 2 * HT_OX, 2 * HT_OX + 1)]
    c += [(150, h, S, S, "random", "HT_ROWS: h %d" % h) for h in (HT_ROWS - 1, HT_ROWS, HT_ROWS + 1, 2 * HT_ROWS - 1, 2 * HT_ROWS, 2 * HT_ROWS + 1)]
    # VT_OY: output heights around a tile; VT_XBYTES: output rows of 255, 258, 510, 513 bytes; V_BYTES: rows of 4k + 1, 2, 3 bytes
    c += [(60, 77, 50, oh, "random", "VT_OY: out_h %d" % oh) for oh in (VT_OY - 1, VT_OY, VT_OY + 1, 2 * VT_OY - 1, 2 * VT_OY, 2 * VT_OY + 1)]
    c += [(700, 23, ow, 11, "random", "VT_XBYTES: %d-byte rows" % (3 * ow)) for ow in (VT_XBYTES // 3, VT_XBYTES // 3 + 1, 2 * VT_XBYTES // 3, 2 * VT_XBYTES // 3 + 1)]
    c += [(70, 23, ow, 11, "random", "V_BYTES: %d-byte rows" % (3 * ow)) for ow in (3, 6, 7, 8)]
    # vertical pass reading the SOURCE (horizontal skipped): rows of 300 bytes (dword loads) and of 297, 306, 303 (byte loads)
    c += [(w, 41, w, 29, "random", "source rows of %d bytes into the vertical pass" % (3 * w)) for w in (100, 99, 102, 101)]
    return c


CASES = _cases()
TOWER_CASES = [i for i, c in enumerate(CASES) if c[2:4] == (S, S)]


@functools.lru_cache(maxsize=None)
def _image(i):
    w, h, _, _, px, _ = CASES[i]
    a = R.make_image(w, h, px, seed=i)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(i):
    """the restatement's result of case i, computed once and shared"""
    a = R.resize(_image(i), CASES[i][2], CASES[i][3])
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def engine(gpu, mse):
    from mse import siglip
    cfg = dict(siglip.SO400M_384, depth=1, img_size=S)
    eng = siglip.SiglipImageEngine.from_state_dict(siglip.synthetic_state_dict(cfg), cfg, max_batch=len(TOWER_CASES))
    eng.image_size = (S, S)
    yield eng
    eng.close()


def bmp24(rgb, bottom_up=True):
    """24-bit BMP by hand (what image::codecs::bmp::BmpEncoder writes, src/common.rs:50-53; top-down: negative height): rows padded
    to 4 bytes with a NON-zero filler, so that a kernel that read the padding would show."""
    h, w, _ = rgb.shape
    stride = (3 * w + 3) & ~3
    rows = np.full((h, stride), 0xEE, np.uint8)
    rows[:, :3 * w] = (rgb[::-1] if bottom_up else rgb)[:, :, ::-1].reshape(h, 3 * w)
    pixels = rows.tobytes()
    return (b"BM" + struct.pack("<IHHI", 54 + len(pixels), 0, 0, 54)
            + struct.pack("<IiiHHIIiiII", 40, w, h if bottom_up else -h, 1, 24, 0, len(pixels), 2835, 2835, 0, 0) + pixels)


CONFIG = {"device": "cuda:0", "model": "ViT-SO400M-14-SigLIP-384", "model_name": "siglip-so400m-14-384", "max_batch_size": 4, "port": 0}


def run_with_server(server, coro_fn):
    import asyncio
    from aiohttp.test_utils import TestClient, TestServer

    async def go():
        client = TestClient(TestServer(server.make_app()))
        await client.start_server()
        try:
            return await coro_fn(client)
        finally:
            await client.close()

    server.start_threads()
    try:
        return asyncio.new_event_loop().run_until_complete(go())
    finally:
        server.stop_threads()


def test_boundaries_are_where_the_cases_put_them():
    """the staging boundaries the cases are built around, restated from the source's constants"""
    assert (HT_OX, HT_ROWS, VT_OY, VT_XBYTES) == (32, 8, 8, 256)
    for w, want in ((W_SEG - 1, True), (W_SEG, False)):
        assert all(p for p, _ in _h_tiles(w, S, R.LANCZOS3, HT_ROWS)) == want
        assert all(p for p, _ in _h_tiles(w, S, R.LANCZOS3, 1))                 # the one-row band of a 9-row image still stages
    for w, want in ((W_COEF - 1, True), (W_COEF, False)):
        assert all(k for _, k in _h_tiles(w, S, R.LANCZOS3, HT_ROWS)) == want
    assert W_SEG > W_COEF                                                    # so W_SEG + 1 has both through L2


@pytest.mark.gpu
def test_resize_equals_restatement_and_pillow(gpu, mse):
    """Items 1 and 2: every case alone through mse_resize_rgb8 == the restatement == Pillow (its own two passes, horizontal first); the
    stripe cases reach both clamps."""
    from mse import siglip
    bad = []
    for i, (w, h, ow, oh, px, why) in enumerate(CASES):
        got = siglip.resize_rgb8([_image(i)], (ow, oh))[0]
        want = _want(i)
        assert got.shape == want.shape == (oh, ow, 3)
        if px == "stripes":
            assert want.min() == 0 and want.max() == 255, (why, "the stripes do not reach both clamps")
        n_ref, n_pil = int((got != want).sum()), int((got != R.pil_resize(_image(i), ow, oh)).sum())
        print("%-70s %5d x %-5d -> %4d x %-4d %-8s differing bytes: restatement %d, Pillow %d" % (why, w, h, ow, oh, px, n_ref, n_pil))
        if n_ref or n_pil:
            bad.append((why, w, h, ow, oh, px, n_ref, n_pil))
    assert not bad, bad


@pytest.mark.gpu
def test_explicit_filters(gpu, mse):
    """The filter argument: both filters on a shrinking and a growing image, each equal to the restatement with that filter."""
    from mse import siglip
    for w, h in ((S + 30, S + 7), (S - 30, S + 7)):
        img = R.random_image(w, h, 77)
        for name, f in (("hamming", R.HAMMING), ("lanczos3", R.LANCZOS3)):
            assert np.array_equal(siglip.resize_rgb8([img], S, name)[0], R.resize(img, S, S, f)), (w, h, name)


@pytest.mark.gpu
def test_mixed_batch_equals_each_alone_and_permuted(gpu, mse):
    """Item 3: all tower-size cases in ONE call == each alone (== the restatement), and == the same batch permuted."""
    from mse import siglip
    imgs = [_image(i) for i in TOWER_CASES]
    got = siglip.resize_rgb8(imgs, S)
    for j, i in enumerate(TOWER_CASES):
        assert np.array_equal(got[j], _want(i)), CASES[i]
    perm = np.random.default_rng(3).permutation(len(imgs))
    again = siglip.resize_rgb8([imgs[j] for j in perm], S)
    assert np.array_equal(again, got[perm])


@pytest.mark.gpu
def test_sub_batches(gpu, mse):
    """SUB_BATCH_IMAGES: a call of one image more than a sub-batch holds, every image different, == each image's restatement; and two
    sub-batches by BYTES -- two images of 137 MB, above the 256 MiB of staging together -- == the image alone, twice."""
    from mse import siglip
    n = SUB_BATCH_IMAGES + 1
    rng = np.random.default_rng(9)
    imgs = [rng.integers(0, 256, size=(1 + i % 3, 1 + i % 2, 3), dtype=np.uint8) for i in range(n)]
    got = siglip.resize_rgb8(imgs, (5, 4))
    want = {}
    for j in (0, 1, 2, 3, 4, 5, SUB_BATCH_IMAGES - 1, SUB_BATCH_IMAGES):
        assert np.array_equal(got[j], R.resize(imgs[j], 5, 4)), j
    for j in range(n):                                   # every image: a 1..3 x 1..2 source has few distinct results per shape
        key = imgs[j].tobytes() + bytes(imgs[j].shape)
        if key not in want:
            want[key] = R.resize(imgs[j], 5, 4)
        assert np.array_equal(got[j], want[key]), j
    big = rng.integers(0, 256, size=(2800, 16384, 3), dtype=np.uint8)
    assert 2 * big.nbytes > (256 << 20) > big.nbytes
    alone = siglip.resize_rgb8([big], S)[0]
    both = siglip.resize_rgb8([big, big], S)
    assert np.array_equal(both[0], alone) and np.array_equal(both[1], alone)
    rows = R.resize(big[:40], S, 40)                     # the horizontal pass of its first rows against the restatement (16384 -> 98)
    assert np.array_equal(siglip.resize_rgb8([big[:40]], (S, 40))[0], rows)


@pytest.mark.gpu
def test_sub_batches_cut_by_table_bytes(gpu, mse):
    """The coefficient tables count towards the 256 MiB of a sub-batch: 700 one-row images of 700 different widths near 16384 bring 700
    horizontal Lanczos3 tables of 0.38 MB each (264 MB), so the call is cut where the pixels alone (34 MB) would not cut it.  Images on
    both sides of the cut and at the ends == the restatement; a repeated call gives the same bytes."""
    from mse import siglip
    widths = [16384 - i for i in range(700)]
    table_bytes = [4 * (2 + 2 * S + S * R.bounds(w, S, R.LANCZOS3)[0]) for w in widths]
    assert sum(table_bytes) > (256 << 20) > sum(table_bytes[:600]) and sum(3 * w for w in widths) < (64 << 20)
    cut = next(i for i in range(700) if sum(table_bytes[:i + 1]) + sum(3 * w + 16 + 3 * S + 16 + 3 * S * 2 for w in widths[:i + 1]) > (256 << 20))
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, size=(1, w, 3), dtype=np.uint8) for w in widths]
    got = siglip.resize_rgb8(imgs, (S, 2))
    for j in (0, cut - 1, cut, cut + 1, 699):
        assert np.array_equal(got[j], R.resize(imgs[j], S, 2)), (j, cut)
    assert np.array_equal(siglip.resize_rgb8(imgs, (S, 2)), got)


@pytest.mark.gpu
def test_encode_images_equals_resize_then_encode(engine, mse):
    """Item 4: encode_images == encode_rgb8(resize_rgb8(...)): the tower input is the restatement followed by x / 127.5 - 1 in fp16,
    the embeddings are equal."""
    from mse import siglip
    imgs = [_image(i) for i in TOWER_CASES]
    got = engine.encode_images(imgs)
    tower_in = engine.debug_resize_input(len(imgs))
    want_in = R.to_nchw_f16(np.stack([_want(i) for i in TOWER_CASES]))
    assert np.array_equal(tower_in.view(np.uint16), want_in.view(np.uint16))
    two_step = engine.encode_rgb8(siglip.resize_rgb8(imgs, S))
    assert np.array_equal(got, two_step) and np.isfinite(got).all()
    # ... and the fp16 output, and a smaller call (the small-batch kernels) against the same two steps
    assert np.array_equal(engine.encode_images(imgs[:3], out="f16"), engine.encode_rgb8(siglip.resize_rgb8(imgs[:3], S), out="f16"))


@pytest.mark.gpu
def test_encode_bmp_any(engine, mse):
    """Item 5: BMP files of any size, bottom-up and top-down, widths whose 3 w mod 4 is 1, 2, 3 and 0 == PIL decode + encode_images."""
    from PIL import Image
    files, decoded = [], []
    for k, w in enumerate((99, 102, 101, 100, 3, 2, 1, 4)):
        assert (3 * w) % 4 == (1, 2, 3, 0)[k % 4]
        for bottom_up in (True, False):
            rgb = R.random_image(w, 37 + 31 * k, 500 + 2 * k + bottom_up) if k % 2 else R.stripes(w, 37 + 31 * k)
            f = bmp24(rgb, bottom_up)
            dec = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"), np.uint8)
            assert np.array_equal(dec, rgb)
            files.append(f)
            decoded.append(dec)
    assert len(files) <= engine.max_batch
    got = engine.encode_bmp_any(files)
    tower_in = engine.debug_resize_input(len(files)).copy()
    assert np.array_equal(got, engine.encode_images(decoded))
    assert np.array_equal(tower_in.view(np.uint16), engine.debug_resize_input(len(files)).view(np.uint16))
    assert np.array_equal(tower_in.view(np.uint16), R.to_nchw_f16(np.stack([R.resize(d, S, S) for d in decoded])).view(np.uint16))


@pytest.mark.gpu
def test_bmp_of_the_tower_size_equals_encode_bmp(engine, mse):
    """Item 6: files already S x S (bottom-up and top-down) through encode_bmp_any == encode_bmp."""
    files = [bmp24(R.random_image(S, S, 600 + k), bool(k % 2)) for k in range(3)]
    assert np.array_equal(engine.encode_bmp_any(files), engine.encode_bmp(files))
    assert np.array_equal(engine.encode_bmp_any(files, out="f16"), engine.encode_bmp(files, out="f16"))


@pytest.mark.gpu
def test_clip_server_device_resize(engine, mse):
    """Item 7: with `device_resize` the response equals the engine call (plain BMPs of any size as "bmp_any", other files decoded
    without resizing as "rgb8_any"); without the key an off-size image takes today's host bicubic path."""
    import msgpack
    from PIL import Image
    from mse.clip_server import ClipServer, Job, decode_image
    rgbs = [R.random_image(150, 120, 700), R.random_image(S, S, 701), R.stripes(64, 200)]
    bmps = [bmp24(rgbs[0]), bmp24(rgbs[1], False), bmp24(rgbs[2])]
    png = io.BytesIO()
    Image.fromarray(rgbs[0], "RGB").save(png, format="PNG")
    mixed = [bmps[2], png.getvalue()]
    on = ClipServer(dict(CONFIG, device_resize=True), engine)
    assert on.prepare(Job(None, bmps))[0] == "bmp_any"
    kind, payload = on.prepare(Job(None, mixed))
    assert kind == "rgb8_any" and payload[0].shape == (200, 64, 3) and np.array_equal(payload[1], rgbs[0])

    async def scenario(client):
        out = []
        for images in (bmps, mixed):
            r = await client.post("/", data=msgpack.dumps({"images": images}))
            out.append((r.status, msgpack.loads(await r.read())))
        return out

    def rows_of(answer):
        status, rows = answer
        assert status == 200, rows
        return np.stack([np.frombuffer(r, "<f2") for r in rows])

    a, b = run_with_server(on, scenario)
    assert np.array_equal(rows_of(a), engine.encode_bmp_any(bmps).astype(np.float16))
    assert np.array_equal(rows_of(b), engine.encode_images([rgbs[2], rgbs[0]]).astype(np.float16))
    # the key absent (and false): the bicubic fallback, byte for byte what it was
    for cfg in (CONFIG, dict(CONFIG, device_resize=False)):
        off = ClipServer(cfg, engine)
        kind, payload = off.prepare(Job(None, bmps))
        assert kind == "rgb8" and np.array_equal(payload, np.stack([decode_image(f, (S, S)) for f in bmps]))
        assert off.prepare(Job(None, [bmps[1]]))[0] == "bmp"
    a, b = run_with_server(ClipServer(CONFIG, engine), scenario)
    bicubic = np.stack([np.asarray(Image.fromarray(r, "RGB").resize((S, S), Image.BICUBIC)) if r.shape[:2] != (S, S) else r for r in rgbs])
    assert np.array_equal(rows_of(a), engine.encode_rgb8(bicubic).astype(np.float16))
    assert not np.array_equal(rows_of(a)[0], engine.encode_bmp_any(bmps[:1]).astype(np.float16)[0])   # two filters, two answers


@pytest.mark.gpu
def test_limits_are_refused_and_leave_the_engine_usable(engine, mse):
    """Item 8: every limit answers with its error before anything is launched, and the next call works."""
    from mse import ffi, siglip
    L = ffi.lib()
    img = R.random_image(40, 30, 800)
    want = engine.encode_images([img])
    buf = np.zeros(64, np.uint8)
    out = np.zeros((2, S, S, 3), np.uint8)
    of32 = np.zeros((2, engine.embedding_size), np.float32)

    def lists(n, w, h, null_image=False):
        return ((C.c_void_p * n)(*[None if null_image else buf.ctypes.data] * n), (C.c_uint32 * n)(*[w] * n), (C.c_uint32 * n)(*[h] * n))

    def refused(rc, *words):
        assert rc != 0
        msg = ffi.last_error()
        assert all(wd in msg for wd in words), msg

    o8, o32 = out.ctypes.data_as(ffi.u8p), of32.ctypes.data_as(ffi.f32p)
    for w, h, word in ((0, 4, "width"), (4, 0, "height"), (16385, 4, "width"), (4, 16385, "height")):
        p, ws, hs = lists(1, w, h)
        refused(L.mse_resize_rgb8(p, ws, hs, 1, S, S, 0, o8), word, "16384")
        refused(L.mse_siglip_encode_rgb8_any(engine._h, p, ws, hs, 1, 0, 1, o32, None), word, "16384")
    p, ws, hs = lists(1, 4, 4)
    for ow, oh in ((0, S), (S, 0), (16385, S), (S, 16385)):
        refused(L.mse_resize_rgb8(p, ws, hs, 1, ow, oh, 0, o8), "output", "16384")
    for filt in (-1, 3):
        refused(L.mse_resize_rgb8(p, ws, hs, 1, S, S, filt, o8), "unknown filter")
        refused(L.mse_siglip_encode_rgb8_any(engine._h, p, ws, hs, 1, filt, 1, o32, None), "unknown filter")
    refused(L.mse_resize_rgb8(None, ws, hs, 1, S, S, 0, o8), "null")
    refused(L.mse_resize_rgb8(p, None, hs, 1, S, S, 0, o8), "null")
    refused(L.mse_resize_rgb8(p, ws, None, 1, S, S, 0, o8), "null")
    refused(L.mse_resize_rgb8(p, ws, hs, 1, S, S, 0, None), "null")
    refused(L.mse_resize_rgb8(p, ws, hs, 0, S, S, 0, o8), "batch")
    pn, wn, hn = lists(1, 4, 4, null_image=True)
    refused(L.mse_resize_rgb8(pn, wn, hn, 1, S, S, 0, o8), "null")
    refused(L.mse_siglip_encode_rgb8_any(engine._h, pn, wn, hn, 1, 0, 1, o32, None), "null")
    refused(L.mse_siglip_encode_rgb8_any(None, p, ws, hs, 1, 0, 1, o32, None), "null")
    refused(L.mse_siglip_encode_rgb8_any(engine._h, None, ws, hs, 1, 0, 1, o32, None), "null")
    refused(L.mse_siglip_encode_bmp_any(engine._h, None, None, 1, 0, 1, o32, None), "null")
    nb = engine.max_batch + 1
    pb, wb, hb = lists(nb, 4, 4)
    refused(L.mse_siglip_encode_rgb8_any(engine._h, pb, wb, hb, nb, 0, 1, o32, None), "max_batch")
    with pytest.raises(mse.MseError, match="max batch"):
        engine.encode_images([img] * nb)
    with pytest.raises(mse.MseError, match="max batch"):
        engine.encode_bmp_any([bmp24(img)] * nb)
    with pytest.raises(mse.MseError, match="filter"):
        engine.encode_images([img], filter="bicubic")
    with pytest.raises(mse.MseError):
        engine.encode_bmp_any([bmp24(img)[:200]])            # the pixel array exceeds the file
    with pytest.raises(mse.MseError):
        engine.encode_bmp_any([b"\x89PNG" + bytes(100)])
    assert np.array_equal(engine.encode_images([img]), want)
    assert np.array_equal(siglip.resize_rgb8([img], S)[0], R.resize(img, S, S))
    t = siglip.resize_timing()
    assert set(t) == {"upload", "horizontal", "vertical", "total"} and t["total"] > 0
