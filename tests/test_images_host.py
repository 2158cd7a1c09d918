"""Problems given as pictures, host side (dot-socp_amd/images.py): the PNG / BMP decoder against an independent one and against
hand-made files, the tap table of imresize against the library's own (dotsocp_imresize_table needs no GPU) bit for bit, the
numpy twin's properties, the reference's image-based examples and the two labyrinth barriers."""
import functools
import os
import struct
import zlib

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import images as I
from dotsocp_amd import render as R
from dotsocp_amd.examples import _truncated_bumps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "tests", "golden", "images")
SHAPES = [os.path.join("DOTmark", "Shapes", "%d.png" % i) for i in range(1, 9)]
# fixture -> the array imread returns: the Shapes are RGBA files with an opaque alpha, the rest 8-bit gray
FIXTURES = [(p, (512, 512, 3)) for p in SHAPES] + [("maze.png", (1024, 1024)), ("maze-14.png", (1024, 1024)),
                                                    ("centaur.bmp", (540, 530)), ("man.bmp", (540, 530))]
ULP = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def fixture(name):
    a = I.imread(os.path.join(RES, name))
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("name,shape", FIXTURES, ids=[f[0].replace(os.sep, "/") for f in FIXTURES])
def test_fixture_decodes(name, shape):
    a = fixture(name)
    assert a.dtype == np.uint8 and a.shape == shape
    Image = pytest.importorskip("PIL.Image")
    ref = np.asarray(Image.open(os.path.join(RES, name)))
    if ref.ndim == 3 and ref.shape[2] == 4:
        assert np.all(ref[..., 3] == 255)
        ref = ref[..., :3]
    assert np.array_equal(a, ref)


@pytest.mark.parametrize("w", [1, 7, 64])
@pytest.mark.parametrize("rgb", [False, True], ids=["gray", "rgb"])
def test_write_png_round_trip(tmp_path, w, rgb):
    rng = np.random.default_rng(w + 100 * rgb)
    im = rng.integers(0, 256, (5, w, 3) if rgb else (5, w), dtype=np.uint8)
    assert np.array_equal(I.imread(R.write_png(str(tmp_path / "a.png"), im)), im)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def _png(w, h, ctype, rows, depth=8, interlace=0, extra=b""):
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)) + extra
            + _chunk(b"IDAT", zlib.compress(rows)) + _chunk(b"IEND", b""))


def _filter_rows(px, bpp, ftypes):
    """PNG-filter the rows of px (h, stride) with the given filter type per row (the encoder's side of the five filters)"""
    px = px.astype(np.int64)
    out = bytearray()
    prev = np.zeros(px.shape[1], dtype=np.int64)
    for row, ft in zip(px, ftypes):
        left = np.concatenate([np.zeros(bpp, np.int64), row[:-bpp]])
        ul = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]])
        if ft == 0:
            pred = np.zeros_like(row)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (left + prev) // 2
        else:
            p = left + prev - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        out += bytes([ft]) + ((row - pred) % 256).astype(np.uint8).tobytes()
        prev = row
    return bytes(out)


@pytest.mark.parametrize("ctype,ch", [(0, 1), (2, 3), (4, 2), (6, 4)], ids=["gray", "rgb", "gray+alpha", "rgba"])
def test_handmade_png_every_filter(tmp_path, ctype, ch):
    rng = np.random.default_rng(ctype)
    h, w = 11, 9
    px = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    if ctype in (4, 6):
        px[..., -1] = 255
    ftypes = [0, 1, 2, 3, 4, 4, 3, 2, 1, 4, 3]             # every filter, also after every other one
    path = tmp_path / "f.png"
    path.write_bytes(_png(w, h, ctype, _filter_rows(px.reshape(h, w * ch), ch, ftypes)))
    want = px[..., 0] if ch <= 2 else px[..., :3]
    assert np.array_equal(I.imread(str(path)), want)


def test_handmade_png_palette(tmp_path):
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 4, (6, 5), dtype=np.uint8)
    plte = _chunk(b"PLTE", bytes([9, 9, 9, 200, 0, 0, 0, 200, 0, 0, 0, 200]))
    path = tmp_path / "p.png"
    path.write_bytes(_png(5, 6, 3, _filter_rows(idx, 1, [0, 1, 2, 3, 4, 0]), extra=plte))
    assert np.array_equal(I.imread(str(path)), idx)


def _bmp(w, h, bits, body, comp=0, palette=b""):
    off = 54 + len(palette)
    return (b"BM" + struct.pack("<IHHI", off + len(body), 0, 0, off)
            + struct.pack("<IiiHHIIiiII", 40, w, h, 1, bits, comp, len(body), 2835, 2835, len(palette) // 4, 0) + palette + body)


GREY = b"".join(bytes([i, i, i, 0]) for i in range(256))


def test_handmade_bmp(tmp_path):
    rng = np.random.default_rng(5)
    g = rng.integers(0, 256, (4, 5), dtype=np.uint8)                     # rows of 5 bytes are padded to 8
    body = b"".join(row.tobytes() + b"\0\0\0" for row in g[::-1])
    (tmp_path / "g.bmp").write_bytes(_bmp(5, 4, 8, body, palette=GREY))
    assert np.array_equal(I.imread(str(tmp_path / "g.bmp")), g)
    (tmp_path / "t.bmp").write_bytes(_bmp(5, -4, 8, b"".join(row.tobytes() + b"\0\0\0" for row in g), palette=GREY))
    assert np.array_equal(I.imread(str(tmp_path / "t.bmp")), g)          # negative height: top-down rows
    c = rng.integers(0, 256, (3, 3, 3), dtype=np.uint8)                  # rows of 9 bytes are padded to 12
    body = b"".join(row[:, ::-1].tobytes() + b"\0\0\0" for row in c[::-1])
    (tmp_path / "c.bmp").write_bytes(_bmp(3, 3, 24, body))
    assert np.array_equal(I.imread(str(tmp_path / "c.bmp")), c)


def test_decoder_refusals(tmp_path):
    def refused(name, data, word):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(ValueError, match=word):
            I.imread(str(p))
    rows = b"\0" + bytes(8)
    refused("i.png", _png(8, 1, 0, rows, interlace=1), "interlaced")
    refused("d.png", _png(4, 1, 0, rows, depth=16), "16-bit")
    refused("a.png", _png(2, 1, 6, b"\0" + bytes([1, 2, 3, 255, 4, 5, 6, 254])), "alpha")
    refused("r.bmp", _bmp(4, 1, 8, bytes(4), comp=1, palette=GREY), "compressed")
    refused("p.bmp", _bmp(4, 1, 8, bytes(4), palette=GREY[4:] + GREY[:4]), "palette")
    refused("b.bmp", _bmp(4, 1, 16, bytes(8)), "16-bit")
    refused("x.gif", b"GIF89a" + bytes(60), "neither")


# ------------------------------------------------------------------------------------------ table
TABLES = [(5, 9), (9, 5), (1, 3), (3, 1), (37, 9), (29, 16), (512, 128), (512, 1024), (256, 257), (540, 256), (7, 7)]


@pytest.mark.parametrize("n_in,n_out", TABLES)
def test_table_matches_library_bit_for_bit(n_in, n_out):
    w, idx = I.imresize_table(n_in, n_out)
    wc, ic = I.imresize_table_c(n_in, n_out)
    assert w.shape == wc.shape and idx.dtype == ic.dtype == np.int32
    assert np.array_equal(w.view(np.int64), wc.view(np.int64))
    assert np.array_equal(idx, ic)
    assert idx.min() >= 0 and idx.max() < n_in
    assert D.capi.lib().dotsocp_imresize_taps(n_in, n_out) == I.imresize_max_taps(n_in, n_out) >= w.shape[1]


def test_tap_counts():
    for n_in, n_out in [(5, 9), (1, 3), (512, 1024), (256, 257), (2, 64), (100, 101)]:
        assert I.imresize_table(n_in, n_out)[0].shape[1] == 4           # any upscale, once the zero columns are dropped
    assert I.imresize_table(37, 9)[0].shape[1] == 17
    assert I.imresize_table(7, 7)[0].shape[1] == 1                      # the identity


def test_table_refuses_bad_lengths():
    L = D.capi.lib()
    assert L.dotsocp_imresize_taps(0, 4) == -1 and L.dotsocp_imresize_taps(4, 65537) == -1
    with pytest.raises(ValueError):
        I.imresize_table(0, 4)


@pytest.mark.skipif(D.capi.lib().dotsocp_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    a = np.arange(30, dtype=np.uint8).reshape(6, 5)
    with pytest.raises(D.capi.DotsocpError) as e:
        I.imresize_device(a, (4, 3))
    assert e.value.code == -2                                   # DOTSOCP_ENODEVICE
    with pytest.raises(D.capi.DotsocpError) as e:
        I.image_density([a], 5, 5, "single", device=0)
    assert e.value.code == -2
    with pytest.raises(D.capi.DotsocpError) as e:               # the arguments are judged first
        I.imresize_device(a.reshape(6, 5, 1).repeat(5, axis=2), (4, 3))
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------ twin alone
def test_same_size_is_identity():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (13, 7), dtype=np.uint8)
    assert np.array_equal(I.imresize(a, a.shape), a)
    d = rng.standard_normal((13, 7))
    assert np.array_equal(I.imresize(d, d.shape), d)


@pytest.mark.parametrize("c", [1.0, 0.7310585786300049, 255.0])
@pytest.mark.parametrize("size", [(64, 29), (37, 100), (74, 29), (37, 30)])
def test_constant_double_image_stays_constant(size, c):
    """To 2 ulp (2 * 2^-52 c = 4 u c, u the unit roundoff).  What the arithmetic guarantees: a pass of an upscale has four
    taps with sum |w| <= 1.25 and partial sums <= 1.1 c, so its four products round by at most 0.63 u c together, its three
    additions by 1.65 u c, and the row sums to 1 within 1 u (Neumaier): 3.3 u c < 4 u c.  So the cases are ONE four-tap pass
    (the other axis keeps its length: the identity table, exact).  Two passes, or the 17 taps of a shrinking pass, are not
    bound by 2 ulp by this arithmetic: measured, 37 x 29 -> 9 x 16 gives 1.4 to 2.01 ulp and -> 64 x 50 1.0 to 2.05 ulp for
    the three constants here, -> 3 x 100 gives 3 ulp (the first two printed by `python -m pytest -s`)."""
    out = I.imresize(np.full((37, 29), c), size)
    dev = lambda s: np.max(np.abs(I.imresize(np.full((37, 29), c), s) - c)) / (ULP * c)      # noqa: E731
    print("constant %.17g -> %s: %.2f ulp; two passes: (9, 16) %.2f ulp, (64, 50) %.2f ulp" % (c, size, dev(size), dev((9, 16)), dev((64, 50))))
    assert np.max(np.abs(out - c)) <= 2 * ULP * c


def test_pass_order_matters_and_is_the_references():
    rng = np.random.default_rng(0)
    a = (rng.integers(0, 2, (37, 29)) * 255).astype(np.uint8)
    assert I.pass_order(37, 29, 9, 16) == (0, 1) and I.pass_order(29, 37, 16, 9) == (1, 0)
    assert I.pass_order(10, 10, 5, 5) == (0, 1)                          # a tie: the rows first
    x, y = I.imresize(a, (9, 16)), I.imresize(a, (9, 16), order=(1, 0))
    differ = int(np.count_nonzero(x != y))
    print("bytes that differ between the two pass orders: %d of %d" % (differ, x.size))
    assert differ > x.size // 2                                          # 103 of 144: a wrong order cannot hide
    assert np.array_equal(I.imresize(a, (9, 16), order=(0, 1)), x)


@pytest.mark.parametrize("n", [128, 1024])
def test_binary_picture_saturates_at_both_ends(n):
    g = I.rgb2gray(fixture(SHAPES[2]))
    first = I.round_u8(I._resize_pass(g.astype(np.float64).reshape(512, 512, 1), 0, n))
    acc = I._resize_pass(first.astype(np.float64), 1, n)
    print("Shapes/3 512 -> %d: accumulators %.1f .. %.1f before the clip" % (n, acc.min(), acc.max()))
    assert acc.min() < -1.0 and acc.max() > 256.0                         # the cubic overshoots (-11 .. 266, -24 .. 273)
    out = I.imresize(g, (n, n))
    assert np.array_equal(out, I.round_u8(acc)[..., 0])
    assert out.min() == 0 and out.max() == 255
    assert np.all(out[acc[..., 0] < 0.0] == 0) and np.all(out[acc[..., 0] > 255.0] == 255)       # nothing wraps


def test_rgb2gray_of_equal_channels():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(I.rgb2gray(np.stack([v, v, v], axis=2)), v)


# ------------------------------------------------------------------------------------------ examples
def _mean_is_one(rho):
    return abs(float(np.mean(rho)) - 1.0) <= 4 * ULP


@pytest.mark.parametrize("n", [17, 33])
def test_example_densities(n):
    r5 = D.get_example_2d("example5", n, n, resources=RES)
    plain = I.get_example_from_images(os.path.join(RES, "centaur.bmp"), os.path.join(RES, "man.bmp"), n, n)
    rev = I.get_example_from_images(os.path.join(RES, "centaur.bmp"), os.path.join(RES, "man.bmp"), n, n, ReverseColor=True)
    for rho in r5 + plain + rev:
        assert rho.shape == (n, n) and _mean_is_one(rho), float(np.mean(rho)) - 1.0
        assert np.all(rho[-1, :] == 0.0) and np.all(rho[:, -1] == 0.0) and rho.min() >= 0.0
    for a, b in zip(r5, rev):
        assert np.array_equal(a, b)                          # lower_bound 0: the bits of get_example_from_images' normalisation
    raw = I.gene_example5(n, n, RES)
    assert all(np.allclose(a / a.mean(), b, rtol=1e-14) for a, b in zip(raw, r5))
    st = D.get_example_2d("DOTmark_4stitch", n, n, resources=RES, DOTmark_type="Shapes")
    for rho in st:
        assert rho.shape == (n, n) and _mean_is_one(rho), float(np.mean(rho)) - 1.0
    assert st[0].min() < 0.0                                 # the double resize overshoots on binary pictures: restated
    lb = D.get_example_2d("example5", n, n, 0.1, resources=RES)
    assert all(_mean_is_one(r) and abs(r.min() - 0.1 / 1.1) < 1e-15 for r in lb)


def test_example_argument_errors():
    with pytest.raises(ValueError, match="Novalid input"):
        D.get_example_2d("example5", 17, 17)
    with pytest.raises(ValueError, match="Novalid input"):
        D.get_example_2d("DOTmark_4stitch", 17, 17)
    with pytest.raises(ValueError, match="Novalid input"):
        D.get_example_2d("example8", 17, 17, resources=RES)
    with pytest.raises(ValueError, match=r"type \(pos 3\) must be 'ClassicImages' or 'Shapes'"):
        I.gene_example_DOTmark_4stitch(17, 17, "Faces", resources=RES)
    with pytest.raises(ValueError, match=r"stitch1_indices \(pos 4\) must be a vector of length 4"):
        I.gene_example_DOTmark_4stitch(17, 17, "Shapes", [1, 2, 3], resources=RES)
    with pytest.raises(ValueError, match=r"stitch2_indices \(pos 5\) must be a vector of length 4"):
        I.gene_example_DOTmark_4stitch(17, 17, "Shapes", [1, 2, 3, 4], [5], resources=RES)
    a, b = I.gene_example_DOTmark_4stitch(17, 17, "shapes", [4, 3, 2, 1], [8, 7, 6, 5], resources=RES)
    assert a.shape == b.shape == (17, 17)


# ------------------------------------------------------------------------------------------ mazes
MAZES = [("example6", I.gene_barrier_of_example6, ((0.925, 0.075), (0.075, 0.925), 0.09, 0.09 / 3)),
         ("maze14", I.gene_barrier_of_maze14, ((0.075, 0.075), (0.925, 0.925), 0.075, 0.075 / 2))]


@pytest.mark.parametrize("n", [33, 65, 129])
@pytest.mark.parametrize("name,make,bumps", MAZES, ids=[m[0] for m in MAZES])
def test_maze_barriers(name, make, bumps, n):
    barrier = make(RES)
    rho0, rho1 = _truncated_bumps(n, n, *bumps)
    m0, m1 = rho0.sum(), rho1.sum()
    k0, k1, mask = D.ensure_barrier_validity(rho0, rho1, barrier)
    kept0, kept1 = rho0[~mask].sum() / m0, rho1[~mask].sum() / m1
    sw = D.get_space_weight_by_barrier(n, n, barrier)
    edges = float(np.mean(sw.weightX > 1.0))
    print("%s at %d: %.1f %% of the nodes masked, %.1f %% / %.1f %% of the mass kept, %.1f %% of the x edges marked"
          % (name, n, 100 * mask.mean(), 100 * kept0, 100 * kept1, 100 * edges))
    assert 0.17 <= mask.mean() <= 0.25
    assert kept0 > 0.95 and kept1 > 0.95
    assert 0.16 <= edges <= 0.20
    assert abs(k0.mean() - 1.0) < 1e-12 and abs(k1.mean() - 1.0) < 1e-12


def test_nearest_sample_sends_midpoints_up():
    pic = np.arange(1024, dtype=np.float64)[:, None] * np.ones((1, 1024))
    b = I.ImageBarrier(pic)
    assert b(0.5, 0.0) == 512.0                                         # x = 0.5: 511.5 + 0.5 -> row 512, not 511
    assert b(0.0, 0.5) == 0.0 and b(1.0, 1.0) == 1023.0 and b(-0.2, 0.3) == 0.0 and b(1.2, 0.3) == 1023.0
    x = np.array([[0.25, 0.5], [0.75, 1.0]])
    assert np.array_equal(b(x, np.zeros_like(x)), np.floor(x * 1023.0 + 0.5))
    sat = I.barrier_of_image(np.array([[0, 100], [200, 128]], dtype=np.uint8))
    assert np.array_equal(sat.picture, [[200.0, 100.0], [0.0, 72.0]])     # 255 / 200 rounds to 1 in uint8 arithmetic
    sat = I.barrier_of_image(np.array([[0, 100], [50, 90]], dtype=np.uint8))
    assert np.array_equal(sat.picture, [[255.0, 0.0], [150.0, 30.0]])     # 255 / 100 rounds to 3; 100 * 3 saturates
