"""SigLIP towers: batch invariance at every boundary where the host code switches kernels by row count.

include/mse.h promises for the image tower: (A) rows of calls of >= 5 images are bit-equal whatever the batch (and whatever the
number of streams the call is split over), (B) MSE_SIGLIP_NOSMALL=1 makes that hold for every call size, and calls of 1-4 images
otherwise stay within 1e-4 cosine of the batch kernels and 1e-3 of the fp32 model.  The text tower promises the 1e-3 only.
The call sizes below are DERIVED from the constants of the sources and from a restatement of the two split formulas, one case on
either side of each switch; every comparison is made on the fp32 outputs."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

torch.set_grad_enabled(False)

CSRC = os.path.join(ROOT, "meme-search-engine_amd", "csrc")


def _const(fname, name):
    """`name = <integer>` as the source states it (constexpr or static constexpr, possibly one of several on a line)."""
    src = open(os.path.join(CSRC, fname)).read()
    m = re.search(r"constexpr[^;]*\b" + name + r"\s*=\s*(\d+)", src)
    assert m, (fname, name)
    return int(m.group(1))


SMALL_BATCH = _const("siglip_api.hip", "SMALL_BATCH")              # images per call that take the small-batch kernels (4)
MAX_SIDE = _const("siglip_api.hip", "MAX_SIDE")                    # side streams of an image call (3)
LN_WG_MAX_ROWS = _const("siglip.h", "LN_WG_MAX_ROWS")    # rows up to which a small call's LayerNorm is layernorm_wg_kernel
SMALL_SKINNY_ROWS = _const("siglip_kernels.hip", "SMALL_SKINNY_ROWS")   # <= 64 rows: K-split skinny GEMM, short-K projection split
SMALL_MID_ROWS = _const("siglip_kernels.hip", "SMALL_MID_ROWS")    # <= 3072 rows: 64 x 64 tiles
SMALL_T128_ROWS = _const("siglip_kernels.hip", "SMALL_T128_ROWS")  # > 2048 rows and K > 2048: 128 x 128 tiles
SPLIT_MAX_ROWS = _const("siglip_kernels.hip", "SPLIT_MAX_ROWS")    # <= 768 rows: fc2 split along K
FUSED_MIN_ROWS = _const("siglip_text_api.hip", "FUSED_MIN_ROWS")   # text: parts of more rows run the LayerNorm-fused GEMMs
TEXT_MAX_PARTS = _const("siglip_text_api.hip", "MAX_PARTS")
T = 64                                                             # context length of the text tower (rows per text)
IMG_ROWS = 736                                                     # token rows of an image: 27 * 27 = 729 rounded up to 32


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / np.linalg.norm(a, axis=-1) / np.linalg.norm(b, axis=-1)


def round_up(v, m):
    return (v + m - 1) // m * m


def image_sub_batches(batch, streams):
    """Sizes of the sub-batches an image call runs as, the main stream's first: siglip_api.hip, mse_siglip_create
    (`n_side = min(max(MSE_SIGLIP_STREAMS - 1, 0), MAX_SIDE)`) and mse_siglip_encode_image (`parts = min(n_side + 1, batch / 16)`,
    `per = round_up(ceil(batch / parts), 8)`, side ranges from `per` in steps of `per`, the last is whatever remains)."""
    n_side = min(max(streams - 1, 0), MAX_SIDE)
    parts = min(n_side + 1, batch // 16)
    if parts <= 1:
        return [batch]
    per = round_up((batch + parts - 1) // parts, 8)
    return [min(per, batch - b0) for b0 in range(0, batch, per)]


def text_parts(batch, n_parts):
    """Sizes of the parts a text call runs as: siglip_text_api.hip text_forward (`parts = batch >= 32 ? min(n_parts, batch / 16) : 1`,
    `per = max(4, (batch / parts) / 4 * 4)`, the last part is whatever remains; fused when `per * T > FUSED_MIN_ROWS`)."""
    parts = min(n_parts, batch // 16) if batch >= 32 else 1
    if parts <= 1:
        return [batch]
    per = max(4, (batch // parts) // 4 * 4)
    return [per] * (parts - 1) + [batch - (parts - 1) * per]


def _slug(why):
    return re.sub(r"[^A-Za-z0-9]+", "_", why).strip("_")


def seams(sizes):
    """Row positions worth planting a kept row at: the start, both sides of every seam between sub-batches, the end."""
    pos, b0 = {0, sum(sizes) - 1}, 0
    for s in sizes[:-1]:
        b0 += s
        pos.update((b0 - 1, b0))
    return sorted(pos)


# ---------------------------------------------------------------------------------------------------------
# the image tower's cases
# ---------------------------------------------------------------------------------------------------------
IMG_MAX = 80          # the largest derived batch (four sub-batches of 24 with a trailing 8)


def _image_cases():
    """(streams, batch, the boundary it sits on).  For every stream count the smallest batch that runs on ALL its streams and
    whose last sub-batch is 1 image (736 rows <= LN_WG_MAX_ROWS: a launch-sized LayerNorm choice would differ there), 2 images,
    8 images and a full `per` -- where the split formula can produce it -- and the batch with the smallest trailing sub-batch
    otherwise; then the fixed sizes on either side of SMALL_BATCH, of the 16-image and 32-image steps of `parts` and of 48."""
    cases = []
    for streams in (1, 2, 3, 4):
        for b, why in ((SMALL_BATCH + 1, "first batch-kernel size"), (16, "below a 16-image step"), (17, "above a 16-image step"),
                       (31, "last unsplit size at two streams"), (32, "first split size"), (47, "last two-part size at three streams"),
                       (48, "first three-part size"), (49, "one past a 16-image step")):
            cases.append((streams, b, why))
        if streams == 1:
            continue
        full = [b for b in range(16 * streams, IMG_MAX + 1) if len(image_sub_batches(b, streams)) == streams]
        for last, why in ((1, "trailing sub-batch of 1 image"), (2, "trailing sub-batch of 2 images"), (8, "trailing sub-batch of 8 images")):
            hit = [b for b in full if image_sub_batches(b, streams)[-1] == last]
            if hit:
                cases.append((streams, hit[0], why))
        smallest = min(full, key=lambda b: image_sub_batches(b, streams)[-1])
        cases.append((streams, smallest, "smallest trailing sub-batch this stream count can produce"))
        even = [b for b in full if len(set(image_sub_batches(b, streams))) == 1 and image_sub_batches(b, streams)[0] > 16]
        if even:
            cases.append((streams, even[0], "every sub-batch a full `per`"))
    seen, out = set(), []
    for s, b, why in cases:
        if (s, b) not in seen:
            seen.add((s, b))
            out.append(pytest.param(s, b, id=f"streams{s}-batch{b}-{'+'.join(map(str, image_sub_batches(b, s)))}-{_slug(why)}"))
    return out


IMAGE_CASES = _image_cases()


@pytest.mark.gpu
def test_the_restated_image_split_produces_the_cases_the_contract_names():
    """The restatement against the splits DESIGN 3.3 and tests/test_siglip.py state (41 -> 24 + 17, 256 -> 128 + 128, 32 -> 16 + 16),
    and the hole of the issue: 49 images on three streams end in ONE image."""
    assert image_sub_batches(41, 2) == [24, 17] and image_sub_batches(256, 2) == [128, 128] and image_sub_batches(32, 2) == [16, 16]
    assert image_sub_batches(31, 4) == [31] and image_sub_batches(49, 1) == [49]
    assert image_sub_batches(49, 3) == [24, 24, 1] and image_sub_batches(50, 3) == [24, 24, 2] and image_sub_batches(56, 3) == [24, 24, 8]
    assert image_sub_batches(73, 4) == [24, 24, 24, 1] and image_sub_batches(80, 4) == [24, 24, 24, 8]
    assert IMG_ROWS <= LN_WG_MAX_ROWS < 2 * IMG_ROWS          # exactly ONE image is "few rows" to a launch-sized LayerNorm choice
    ids = {p.id.split("-")[0] + "-" + p.id.split("-")[1] for p in IMAGE_CASES}
    assert {"streams3-batch49", "streams3-batch50", "streams3-batch56", "streams4-batch73", "streams2-batch33", "streams2-batch32"} <= ids
    assert text_parts(31, 4) == [31] and text_parts(32, 2) == [16, 16] and text_parts(49, 3) == [16, 16, 17] and text_parts(104, 2) == [52, 52]


_ENGINES = {}


def _engine(cls, key, env, *args, **kw):
    """One engine per (tower, environment): the hooks are read when an engine is created, so set, create, delete."""
    if key not in _ENGINES:
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, str(v))
            _ENGINES[key] = cls.from_state_dict(*args, **kw)
            for k in env:
                mp.delenv(k)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


@pytest.fixture(scope="module")
def ref():
    from oracle import siglip_ref
    return siglip_ref


def _plant_layernorms(sd, names, seed):
    g = torch.Generator().manual_seed(seed)
    for nm in names:
        sd[nm + "weight"] = 0.5 + torch.rand(1152, generator=g)
        sd[nm + "bias"] = 0.2 * torch.randn(1152, generator=g)


class Images:
    DEPTH = 2

    def __init__(self, ref):
        self.cfg = dict(ref.CONFIG, depth=self.DEPTH)
        self.sd = ref.synthetic_weights(self.cfg)
        _plant_layernorms(self.sd, [f"trunk.blocks.{i}.{nm}." for i in range(self.DEPTH) for nm in ("norm1", "norm2")] +
                          ["trunk.norm.", "trunk.attn_pool.norm."], 9)
        self.named = {"visual." + k: v for k, v in self.sd.items()}
        self.x = ref.synthetic_images(IMG_MAX, self.cfg).numpy().astype(np.float16)
        # other data for the neighbours of a kept image: another seed, with pixels far outside [-1, 1] planted in every image
        self.other = ref.synthetic_images(IMG_MAX, self.cfg, seed=0x5EED0A04).numpy().astype(np.float16)
        self.other[:, :, ::7, ::5] = np.float16(200.0)
        self.other[:, 1, 3::11, 2::13] = np.float16(-1500.0)

    def engine(self, streams=None, nosmall=False, max_batch=IMG_MAX):
        from mse import siglip
        env = {}
        if streams is not None:
            env["MSE_SIGLIP_STREAMS"] = streams
        if nosmall:
            env["MSE_SIGLIP_NOSMALL"] = 1
        return _engine(siglip.SiglipImageEngine, ("image", streams, nosmall, max_batch), env, self.named,
                       dict(siglip.SO400M_384, depth=self.DEPTH), max_batch=max_batch)


@pytest.fixture(scope="module")
def images(gpu, mse, ref):
    return Images(ref)


@pytest.fixture(scope="module")
def five_rows(images):
    """Every image encoded in a call of FIVE (the smallest call of the batch kernels, one stream): what contract A measures against."""
    eng = images.engine(streams=1)
    rows = np.empty((IMG_MAX, 1152), np.float32)
    for lo in list(range(0, IMG_MAX - 5, 5)) + [IMG_MAX - 5]:
        rows[lo:lo + 5] = eng.encode_image(images.x[lo:lo + 5])
    assert np.isfinite(rows).all() and np.all(np.abs(np.linalg.norm(rows, axis=1) - 1) < 1e-3)
    return rows


def _differing(got, want):
    d = np.flatnonzero((got != want).any(axis=1))
    return "rows that differ: %s; largest |difference| %.3g" % (d.tolist(), float(np.abs(got - want).max())) if d.size else ""


@pytest.mark.gpu
@pytest.mark.parametrize("streams,batch", IMAGE_CASES)
def test_rows_of_batch_calls_equal_five_image_calls(images, five_rows, streams, batch):
    """Contract A: a call of >= 5 images, whatever its size and however many streams it is split over, returns for every image the
    bits a five-image call returns for it."""
    got = images.engine(streams=streams).encode_image(images.x[:batch])
    print("image call", batch, "on", streams, "streams:", image_sub_batches(batch, streams), _differing(got, five_rows[:batch]) or "bit-equal")
    assert np.array_equal(got, five_rows[:batch]), _differing(got, five_rows[:batch])


@pytest.mark.gpu
def test_default_engine_equals_the_one_stream_reference(images, five_rows):
    """The engine as shipped (no hook set; two streams): a window of five anywhere, and the whole set at once."""
    eng = images.engine()
    assert np.array_equal(eng.encode_image(images.x), five_rows)
    for lo in (0, 37, IMG_MAX - 5):
        assert np.array_equal(eng.encode_image(images.x[lo:lo + 5]), five_rows[lo:lo + 5]), lo


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2, 3, 4])
def test_nosmall_calls_equal_rows_of_a_six_image_call(images, five_rows, batch):
    """Contract B: with MSE_SIGLIP_NOSMALL=1 calls of 1..4 images are bit-equal to the same rows of a six-image call -- an image
    encoded alone at the first and at the LAST position too."""
    eng = images.engine(nosmall=True, max_batch=8)
    six = eng.encode_image(images.x[:6])
    assert np.array_equal(six, five_rows[:6]), _differing(six, five_rows[:6])
    got = eng.encode_image(images.x[:batch])
    print("NOSMALL call of", batch, _differing(got, six[:batch]) or "bit-equal")
    assert np.array_equal(got, six[:batch]), _differing(got, six[:batch])
    tail = eng.encode_image(images.x[6 - batch:6])
    assert np.array_equal(tail, six[6 - batch:]), _differing(tail, six[6 - batch:])
    if batch == 1:
        for i in range(6):
            assert np.array_equal(eng.encode_image(images.x[i:i + 1]), six[i:i + 1]), i


@pytest.mark.gpu
def test_small_calls_stay_within_the_documented_distance(images, five_rows, ref):
    """Calls of 1..SMALL_BATCH images (the small-batch kernels): cosine within 1e-4 of the batch kernels' rows and within 1e-3 of the
    fp32 model (both from mse.h), at the first and at the last images of the set."""
    eng = images.engine()
    for lo in (0, IMG_MAX - SMALL_BATCH):
        want = ref.encode_image(torch.from_numpy(images.x[lo:lo + SMALL_BATCH].astype(np.float32)), images.sd, images.cfg).numpy()
        assert np.all(cosine(five_rows[lo:lo + SMALL_BATCH], want) > 1 - 1e-3)
        for b in range(1, SMALL_BATCH + 1):
            got = eng.encode_image(images.x[lo:lo + b])
            c_big, c_ref = cosine(got, five_rows[lo:lo + b]), cosine(got, want[:b])
            print("small call of", b, "at", lo, "1 - cosine vs batch kernels", (1 - c_big).max(), "vs fp32 model", (1 - c_ref).max())
            assert np.all(c_big > 1 - 1e-4), (b, c_big)
            assert np.all(c_ref > 1 - 1e-3), (b, c_ref)
            assert np.array_equal(eng.encode_image(images.x[lo:lo + b]), got)


NEIGHBOUR_CASES = [pytest.param(None, b, id=f"default-batch{b}") for b in (2, 3, 4)] + IMAGE_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("streams,batch", NEIGHBOUR_CASES)
def test_an_image_row_does_not_depend_on_its_neighbours(images, streams, batch):
    """Keep image i, replace every other image of the call with other data (pixels of magnitude 200 and 1500 among them): row i
    comes back bit-equal.  i at the start, on both sides of every sub-batch seam and at the end."""
    eng = images.engine(streams=streams)
    base = eng.encode_image(images.x[:batch])
    for i in seams(image_sub_batches(batch, 2 if streams is None else streams)):
        x = images.other[:batch].copy()
        x[i] = images.x[i]
        got = eng.encode_image(x)
        assert np.array_equal(got[i], base[i]), (i, float(np.abs(got[i] - base[i]).max()))
        assert batch == 1 or not np.array_equal(got[(i + 1) % batch], base[(i + 1) % batch])     # the neighbours really changed
    assert np.array_equal(eng.encode_image(images.x[:batch]), base)


@pytest.mark.gpu
@pytest.mark.parametrize("streams,a,b", [(None, 1, 5), (None, 4, 5), (None, 5, 4), (3, 49, 5), (3, 5, 49), (4, 73, 1), (None, 33, 2)])
def test_an_image_call_leaves_nothing_behind(images, streams, a, b):
    """A call of size A, then of size B (other images, across a boundary), then A again: A's bits."""
    eng = images.engine(streams=streams)
    first = eng.encode_image(images.x[:a])
    eng.encode_image(images.other[IMG_MAX - b:])
    again = eng.encode_image(images.x[:a])
    assert np.array_equal(again, first), _differing(again, first)


# ---------------------------------------------------------------------------------------------------------
# the text tower
# ---------------------------------------------------------------------------------------------------------
def _first_fused(n_parts):
    """The smallest batch whose parts (all but the last are `per` texts) exceed FUSED_MIN_ROWS rows."""
    return next(b for b in range(1, 4096) if text_parts(b, n_parts)[0] * T > FUSED_MIN_ROWS)


TEXT_MAX = _first_fused(TEXT_MAX_PARTS)          # 208: the first batch whose parts are fused at four parts


def _text_pairs(n_parts):
    """(batch below, batch above, the switch between them) for an engine of n_parts parts."""
    f = _first_fused(n_parts)
    pairs = [(f - 1, f, f"per * {T} rows crosses FUSED_MIN_ROWS {FUSED_MIN_ROWS} at {n_parts} parts"),
             (SMALL_MID_ROWS // T, SMALL_MID_ROWS // T + 1, f"{SMALL_MID_ROWS} rows in the call")]
    if n_parts > 1:
        pairs += [(31, 32, "parts start at 32 texts"), (32, 33, "the last part outgrows the others")]
        pairs += [(16 * p - 1, 16 * p, f"{p} parts from {16 * p} texts") for p in range(3, n_parts + 1)]
    return pairs


SMALL_TEXT_PAIRS = [
    (SMALL_SKINNY_ROWS // T, SMALL_SKINNY_ROWS // T + 1, f"{SMALL_SKINNY_ROWS} rows: K-split skinny GEMMs and the three-way projection split end"),
    (SPLIT_MAX_ROWS // T, SPLIT_MAX_ROWS // T + 1, f"{SPLIT_MAX_ROWS} rows: fc2's split along K ends"),
    (LN_WG_MAX_ROWS // T, LN_WG_MAX_ROWS // T + 1, f"{LN_WG_MAX_ROWS} rows: the workgroup LayerNorm ends"),
]
ONE_PART_PAIRS = [
    (SMALL_T128_ROWS // T, SMALL_T128_ROWS // T + 1, f"{SMALL_T128_ROWS} rows: fc2 moves to 128 x 128 tiles"),
    (SMALL_MID_ROWS // T, SMALL_MID_ROWS // T + 1, f"{SMALL_MID_ROWS} rows: the small-batch tiles end"),
]


def _text_cases():
    pairs = [(2, lo, hi, why) for lo, hi, why in SMALL_TEXT_PAIRS]          # below 32 texts no part count matters: the default engine
    pairs += [(1, lo, hi, why) for lo, hi, why in ONE_PART_PAIRS]
    for n in range(1, TEXT_MAX_PARTS + 1):
        pairs += [(n, lo, hi, why) for lo, hi, why in _text_pairs(n)]
    seen, out = set(), []
    for n, lo, hi, why in pairs:
        if (n, lo, hi) not in seen:
            seen.add((n, lo, hi))
            out.append(pytest.param(n, lo, hi, id=f"parts{n}-{lo}_{hi}-{_slug(why)}"))
    return out


TEXT_CASES = _text_cases()


class Texts:
    LAYERS = 2

    def __init__(self, ref):
        self.cfg = dict(ref.TEXT_CONFIG, layers=self.LAYERS)
        self.sd = ref.synthetic_text_weights(self.cfg)
        _plant_layernorms(self.sd, [f"text.transformer.resblocks.{i}.{nm}." for i in range(self.LAYERS) for nm in ("ln_1", "ln_2")] +
                          ["text.ln_final."], 11)
        self.tok = ref.synthetic_tokens(TEXT_MAX, self.cfg).numpy()
        self.other = ref.synthetic_tokens(TEXT_MAX, self.cfg, seed=0x5EED0A07).numpy()
        self.want = ref.encode_text(torch.from_numpy(self.tok), self.sd, self.cfg, normalize=True).numpy()

    def engine(self, n_parts, max_batch=TEXT_MAX):
        from mse import siglip
        return _engine(siglip.SiglipTextEngine, ("text", n_parts, max_batch), {"MSE_SIGLIP_TEXT_PARTS": n_parts}, self.sd,
                       dict(siglip.SO400M_TEXT, layers=self.LAYERS), max_batch=max_batch)


@pytest.fixture(scope="module")
def texts(gpu, mse, ref):
    return Texts(ref)


@pytest.mark.gpu
def test_the_derived_text_sizes_are_the_ones_the_issue_names():
    got = {(p.values[0], p.values[1], p.values[2]) for p in TEXT_CASES}
    assert {(2, 1, 2), (2, 12, 13), (2, 16, 17), (2, 31, 32), (2, 32, 33), (2, 48, 49), (1, 48, 49), (1, 32, 33), (2, 103, 104), (3, 47, 48),
            (4, 63, 64), (3, 155, 156), (4, 207, 208)} <= got, sorted(got)
    assert TEXT_MAX == 208


@pytest.mark.gpu
@pytest.mark.parametrize("n_parts,lo,hi", TEXT_CASES)
def test_text_calls_on_both_sides_of_a_switch(texts, n_parts, lo, hi):
    """Both sizes: every row within 1e-3 cosine of the fp32 model (the tower's contract), the call deterministic, a row independent of
    its neighbours (kept at the start, on both sides of every part seam, at the end), and size A -> size B -> size A returns A's bits.
    mse.h promises no bit-equality of a text across call sizes and no tolerance for it has been measured: the cosine between the two
    sizes' common rows is printed, not asserted."""
    eng = texts.engine(n_parts)
    out = {}
    for b in (lo, hi):
        got = eng.encode_text(texts.tok[:b])
        c = cosine(got, texts.want[:b])
        assert np.all(c > 1 - 1e-3), (b, c.min())
        assert np.all(np.abs(np.linalg.norm(got, axis=1) - 1) < 1e-3)
        assert np.array_equal(eng.encode_text(texts.tok[:b]), got), b
        for i in seams(text_parts(b, n_parts)):
            t = texts.other[:b].copy()
            t[i] = texts.tok[i]
            alt = eng.encode_text(t)
            assert np.array_equal(alt[i], got[i]), (b, i, float(np.abs(alt[i] - got[i]).max()))
            assert b == 1 or not np.array_equal(alt[(i + 1) % b], got[(i + 1) % b])
        out[b] = got
    for a, b in ((lo, hi), (hi, lo)):
        eng.encode_text(texts.other[TEXT_MAX - b:])
        assert np.array_equal(eng.encode_text(texts.tok[:a]), out[a]), (a, b)
    c = cosine(out[lo], out[hi][:lo])
    print("text calls of %d and %d at %d parts (%s | %s): 1 - cosine of the common rows max %.3g, bit-equal rows %d of %d" %
          (lo, hi, n_parts, text_parts(lo, n_parts), text_parts(hi, n_parts), float((1 - c).max()),
           int((out[lo] == out[hi][:lo]).all(axis=1).sum()), lo))


@pytest.mark.gpu
def test_text_final_layernorm_past_1024_texts(texts):
    """The final LayerNorm of the text tower runs over `batch` rows: LN_WG_MAX_ROWS and one more text take the same kernel now.  Both
    sizes against the fp32 model (first and last rows), deterministic, the last row independent of the others; the two sizes' common
    rows are compared and the figure printed (no promise across text call sizes)."""
    n = LN_WG_MAX_ROWS + 1
    eng = texts.engine(2, max_batch=n)
    tok = np.concatenate([texts.tok] * (n // TEXT_MAX + 1))[:n]
    want = np.concatenate([texts.want] * (n // TEXT_MAX + 1))[:n]
    out = {}
    for b in (n - 1, n):
        got = eng.encode_text(tok[:b])
        c = cosine(got, want[:b])
        assert np.all(c > 1 - 1e-3), (b, c.min())
        assert np.array_equal(eng.encode_text(tok[:b]), got)
        t = np.concatenate([texts.other] * (n // TEXT_MAX + 1))[:b].copy()
        t[b - 1] = tok[b - 1]
        assert np.array_equal(eng.encode_text(t)[b - 1], got[b - 1])
        out[b] = got
    print("text calls of %d and %d: bit-equal common rows %d of %d" % (n - 1, n, int((out[n - 1] == out[n][:n - 1]).all(axis=1).sum()), n - 1))
