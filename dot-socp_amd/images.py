"""Problems given as pictures: the reference's image-based examples (Example 5.5 centaur -> man, the DOTmark stitch,
get_example_from_images) and the two labyrinth barriers of wdot2d, without a MATLAB toolbox.

Four documented MATLAB functions are restated: imread (PNG and BMP, with zlib and struct), imresize (antialiased bicubic,
separable, uint8 rounded after each pass), rgb2gray and griddedInterpolant(..., "nearest").  imresize_table / imresize /
rgb2gray / image_density(device=None) are the numpy twins of dotsocp_imresize_table / dotsocp_imresize /
dotsocp_image_density (include/dotsocp.h; csrc/image_table.h, csrc/image.hip), operation for operation: products and sums
separately rounded, taps added in ascending order, the sum of the density in advect._tree_sum's order -- uint8 results
are equal byte for byte, doubles bit for bit.  Parity with MATLAB itself is not pinned.

Pictures are numpy arrays (h, w) or (h, w, 3), as imread returns them.  Product code never reads the test fixtures:
`resources` is the directory the caller names, laid out as the reference's examples/*/resources.
"""
import ctypes
import math
import os
import struct
import zlib

import numpy as np

from . import capi
from .advect import _tree_sum

IMG_U8, IMG_F64 = 0, 1                      # DOTSOCP_IMG_U8 / DOTSOCP_IMG_F64
LAYOUT_SINGLE, LAYOUT_STITCH4 = 0, 1        # DOTSOCP_IMG_SINGLE / DOTSOCP_IMG_STITCH4
LAYOUTS = {"single": LAYOUT_SINGLE, "stitch4": LAYOUT_STITCH4}
MAX_LEN = 65536                             # DOTSOCP_IMG_MAX_LEN
GRAY_WEIGHTS = (0.298936021293775, 0.587043074451121, 0.114020904255103)     # rgb2gray


# ------------------------------------------------------------------------------------------ imread
def _png_unfilter(raw, h, stride, bpp):
    out = np.empty((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    pos = 0
    for y in range(h):
        ft = raw[pos]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=pos + 1)
        pos += 1 + stride
        if ft == 0:
            cur = line.copy()
        elif ft == 1:           # Sub: running sum of every channel, modulo 256
            pad = (-stride) % bpp
            cur = np.cumsum(np.concatenate([line, np.zeros(pad, np.uint8)]).reshape(-1, bpp), axis=0, dtype=np.uint8).ravel()[:stride]
        elif ft == 2:           # Up
            cur = line + prev
        elif ft in (3, 4):      # Average, Paeth: each byte needs the one bpp to its left
            c = bytearray(stride)
            ln, pv = line.tobytes(), prev.tobytes()
            for i in range(stride):
                a = c[i - bpp] if i >= bpp else 0
                b = pv[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    cc = pv[i - bpp] if i >= bpp else 0
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                c[i] = (ln[i] + pred) & 255
            cur = np.frombuffer(bytes(c), dtype=np.uint8)
        else:
            raise ValueError("imread: PNG row filter %d does not exist" % ft)
        out[y] = cur
        prev = out[y]
    return out


def _drop_alpha(px, what):
    if not np.all(px[..., -1] == 255):
        raise ValueError("imread: %s with an alpha channel that is not opaque everywhere" % what)
    px = px[..., :-1]
    return px[..., 0] if px.shape[-1] == 1 else px


def _read_png(data):
    pos, ihdr, idat, trns = 8, None, [], None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"tRNS":
            trns = body
        elif kind == b"IEND":
            break
    if ihdr is None or not idat:
        raise ValueError("imread: PNG without IHDR or IDAT")
    w, h, depth, ctype, _, _, interlace = ihdr
    if interlace:
        raise ValueError("imread: interlaced PNG is not supported")
    if depth != 8:
        raise ValueError("imread: %d-bit PNG is not supported (8-bit only)" % depth)
    if ctype not in (0, 2, 3, 4, 6):
        raise ValueError("imread: PNG colour type %d does not exist" % ctype)
    if trns is not None and any(b != 255 for b in trns):
        raise ValueError("imread: PNG with a tRNS chunk that is not opaque")
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    raw = zlib.decompress(b"".join(idat))
    stride = w * ch
    if len(raw) < h * (stride + 1):
        raise ValueError("imread: PNG data is shorter than its header says")
    px = _png_unfilter(raw, h, stride, ch).reshape(h, w, ch)
    if ctype in (4, 6):
        return np.ascontiguousarray(_drop_alpha(px, "PNG"))
    return np.ascontiguousarray(px[..., 0] if ch == 1 else px)      # palette: the indices, as imread's single output


def _read_bmp(data):
    off, = struct.unpack("<I", data[10:14])
    hdr, = struct.unpack("<I", data[14:18])
    if hdr < 40:
        raise ValueError("imread: BMP with a %d-byte header (OS/2) is not supported" % hdr)
    w, h, _, bits, comp = struct.unpack("<iiHHI", data[18:34])
    used, = struct.unpack("<I", data[46:50])
    if comp != 0:
        raise ValueError("imread: compressed BMP (method %d) is not supported" % comp)
    if bits not in (8, 24):
        raise ValueError("imread: %d-bit BMP is not supported (8 and 24 only)" % bits)
    if w < 1 or h == 0:
        raise ValueError("imread: BMP of size %d x %d" % (w, h))
    rows, stride = abs(h), (w * bits // 8 + 3) // 4 * 4
    if len(data) < off + rows * stride:
        raise ValueError("imread: BMP data is shorter than its header says")
    px = np.frombuffer(data, dtype=np.uint8, count=rows * stride, offset=off).reshape(rows, stride)
    if h > 0:
        px = px[::-1]
    if bits == 8:
        n = used or 256
        pal = np.frombuffer(data, dtype=np.uint8, count=4 * n, offset=14 + hdr).reshape(n, 4)[:, :3]
        if not np.array_equal(pal, np.repeat(np.arange(n, dtype=np.uint8)[:, None], 3, axis=1)):
            raise ValueError("imread: 8-bit BMP whose palette is not the identity grey ramp (the indices would not be grey values)")
        return np.ascontiguousarray(px[:, :w])
    return np.ascontiguousarray(px[:, :3 * w].reshape(rows, w, 3)[..., ::-1])


def imread(path):
    """uint8 array (h, w) or (h, w, 3) of a PNG (non-interlaced, 8-bit; gray, gray + alpha, RGB, RGBA, palette: the indices) or
    a BMP (uncompressed; 8-bit with the identity grey palette: the indices; 24-bit).  An alpha channel is dropped when it is
    255 everywhere; everything else raises ValueError naming what it met."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] == b"\x89PNG\r\n\x1a\n":
        return _read_png(data)
    if data[:2] == b"BM" and len(data) >= 54:
        return _read_bmp(data)
    raise ValueError("imread: %s is neither a PNG nor a BMP file" % os.path.basename(str(path)))


# ------------------------------------------------------------------------------------------ imresize
def _cubic(x):
    ax = np.abs(x)
    ax2 = ax * ax
    ax3 = ax2 * ax
    inner = ((1.5 * ax3) - (2.5 * ax2)) + 1.0
    outer = (((-0.5 * ax3) + (2.5 * ax2)) - (4.0 * ax)) + 2.0
    return np.where(ax <= 1.0, inner, np.where(ax <= 2.0, outer, 0.0))


def _check_lengths(n_in, n_out):
    if not (1 <= n_in <= MAX_LEN and 1 <= n_out <= MAX_LEN):
        raise ValueError("imresize: lengths must lie in 1 .. %d" % MAX_LEN)


def imresize_max_taps(n_in, n_out):
    """ceil(kernel width) + 2: the columns of the table before the all-zero ones are dropped (dotsocp_imresize_taps)"""
    n_in, n_out = int(n_in), int(n_out)
    _check_lengths(n_in, n_out)
    s = float(n_out) / float(n_in)
    return int(math.ceil(4.0 / s if s < 1.0 else 4.0)) + 2


def imresize_table(n_in, n_out):
    """Twin of dotsocp_imresize_table (csrc/image_table.h): (weights (n_out, taps) float64, indices (n_out, taps) int32,
    0-based) of one pass from n_in to n_out samples -- MATLAB's `contributions` for the cubic kernel, widened by 1 / scale
    when shrinking, rows normalised, positions mirrored at the borders, all-zero columns dropped."""
    n_in, n_out = int(n_in), int(n_out)
    P = imresize_max_taps(n_in, n_out)
    s = float(n_out) / float(n_in)
    shrink = s < 1.0
    width = 4.0 / s if shrink else 4.0
    half = width / 2.0
    shift = 0.5 * (1.0 - 1.0 / s)
    u = np.arange(1, n_out + 1, dtype=np.float64) / s + shift
    left = np.floor(u - half)
    pos = left[:, None] + np.arange(P, dtype=np.float64)[None, :]
    arg = u[:, None] - pos
    w = s * _cubic(s * arg) if shrink else _cubic(arg)
    total, comp = np.zeros(n_out), np.zeros(n_out)          # Neumaier's compensated sum of every row, k ascending
    for k in range(P):
        t = total + w[:, k]
        comp = comp + np.where(np.abs(total) >= np.abs(w[:, k]), (total - t) + w[:, k], (w[:, k] - t) + total)
        total = t
    total = total + comp
    w = w / total[:, None]
    m = np.mod(pos.astype(np.int64) - 1, 2 * n_in)          # a true modulo: `left` is negative at the border
    idx = np.where(m < n_in, m, 2 * n_in - 1 - m)
    keep = np.any(w != 0.0, axis=0)
    return np.ascontiguousarray(w[:, keep]), np.ascontiguousarray(idx[:, keep].astype(np.int32))


def round_u8(acc):
    """floor(acc), one more where the fraction is >= 0.5, clamped to 0 .. 255: the store of every uint8 step"""
    r = np.floor(acc)
    r = r + ((acc - r) >= 0.5)
    return np.clip(r, 0.0, 255.0).astype(np.uint8)


def _resize_pass(a, axis, n_out):
    """float64 (h, w, planes) array -> the accumulators of one pass along `axis`: acc = acc + w_k * v[idx_k], k ascending"""
    w, idx = imresize_table(a.shape[axis], n_out)
    a = np.moveaxis(a, axis, 0)
    acc = np.zeros((n_out,) + a.shape[1:])
    for k in range(w.shape[1]):
        acc = acc + w[:, k].reshape(-1, 1, 1) * a[idx[:, k]]
    return np.moveaxis(acc, 0, axis)


def pass_order(h_in, w_in, h_out, w_out):
    """The axes in the order the passes take them: the smaller scale first, on a tie the rows (sort(scale))"""
    return (1, 0) if float(w_out) / float(w_in) < float(h_out) / float(h_in) else (0, 1)


def imresize(a, size, order=None):
    """Twin of dotsocp_imresize: a uint8 or float64 array (h, w) or (h, w, planes) to size = (h_out, w_out).  uint8 pictures are
    rounded (round_u8) after EACH pass, float64 ones never.  order: the axes in another order than pass_order()'s (tests)."""
    a = np.asarray(a)
    if a.dtype not in (np.uint8, np.float64) or a.ndim not in (2, 3):
        raise ValueError("imresize: a uint8 or float64 array (h, w) or (h, w, planes)")
    h_out, w_out = int(size[0]), int(size[1])
    _check_lengths(a.shape[0], h_out)
    _check_lengths(a.shape[1], w_out)
    u8 = a.dtype == np.uint8
    v = a.reshape(a.shape[0], a.shape[1], -1)
    for axis in (pass_order(a.shape[0], a.shape[1], h_out, w_out) if order is None else order):
        acc = _resize_pass(v.astype(np.float64), axis, (h_out, w_out)[axis])
        v = round_u8(acc) if u8 else acc
    return v.reshape((h_out, w_out) + a.shape[2:])


def rgb2gray(a):
    """uint8 (h, w, 3) -> uint8 (h, w): 0.298936021293775 R + 0.587043074451121 G + 0.114020904255103 B, added in that order,
    round_u8"""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("rgb2gray: a uint8 array (h, w, 3)")
    v = a.astype(np.float64)
    acc = GRAY_WEIGHTS[0] * v[..., 0]
    acc = acc + GRAY_WEIGHTS[1] * v[..., 1]
    acc = acc + GRAY_WEIGHTS[2] * v[..., 2]
    return round_u8(acc)


# ------------------------------------------------------------------------------------------ densities
def _check_images(imgs, layout):
    if layout not in (LAYOUT_SINGLE, LAYOUT_STITCH4):
        raise ValueError("image_density: layout is 'single' or 'stitch4'")
    imgs = [np.asarray(i) for i in imgs]
    if len(imgs) != (1 if layout == LAYOUT_SINGLE else 4):
        raise ValueError("image_density: 'single' takes one picture, 'stitch4' four")
    for i in imgs:
        if i.dtype != np.uint8 or i.ndim not in (2, 3) or (i.ndim == 3 and i.shape[2] not in (1, 3)) or i.size == 0:
            raise ValueError("image_density: pictures are uint8 arrays (h, w) or (h, w, 3)")
    return [i[..., 0] if i.ndim == 3 and i.shape[2] == 1 else i for i in imgs]


def _raw_density(imgs, ny, nx, layout, reverse):
    """The (ny, nx) picture of doubles before the normalisation: what gene_example5.m / gene_example_DOTmark_4stitch.m return"""
    if layout == LAYOUT_SINGLE:
        v = imresize(imgs[0], (ny - 1, nx - 1))
        if v.ndim == 3:
            v = rgb2gray(v)
        d = (255.0 - v.astype(np.float64)) / 255.0 if reverse else v.astype(np.float64)
        rho = np.zeros((ny, nx))
        rho[:ny - 1, :nx - 1] = d
    else:
        sub_h, sub_w = nx // 2, ny // 2         # the reference passes nx as the height (gene_big_image(paths, nx, ny))
        t = [imresize(rgb2gray(i) if i.ndim == 3 else i, (sub_h, sub_w)).astype(np.float64) for i in imgs]
        rho = np.block([[t[0], t[1]], [t[2], t[3]]])
        if rho.shape != (ny, nx):
            rho = imresize(rho, (ny, nx))
    return rho


def _density_twin(imgs, ny, nx, layout, reverse, lower_bound):
    rho = _raw_density(imgs, ny, nx, layout, reverse)
    total = _tree_sum(rho.ravel(order="F"))
    with np.errstate(divide="ignore", invalid="ignore"):
        factor = float(nx * ny) / np.float64(total)
        return np.asfortranarray((factor * rho + lower_bound) / (1.0 + lower_bound))


class _Image(ctypes.Structure):
    """dotsocp_image"""
    _fields_ = [("pix", ctypes.c_void_p), ("h", capi.i64), ("w", capi.i64), ("planes", capi.i64)]


def image_density(imgs, ny, nx, layout="single", reverse=False, lower_bound=0.0, device=None):
    """The (ny, nx) density of one picture ("single": resized to (ny - 1, nx - 1), gray, optionally (255 - v) / 255, one zero
    row and column appended) or of four ("stitch4": gray, each resized to (nx // 2, ny // 2), placed [1 2; 3 4], resized as
    doubles to (ny, nx) where the sizes differ), then ((nx ny / sum) rho + lower_bound) / (1 + lower_bound).
    device None: the numpy twin; a device ordinal: dotsocp_image_density, the same bits."""
    code = LAYOUTS[layout] if isinstance(layout, str) else int(layout)
    if isinstance(imgs, np.ndarray):
        imgs = [imgs]
    imgs = _check_images(imgs, code)
    ny, nx = int(ny), int(nx)
    if not (2 <= ny <= MAX_LEN and 2 <= nx <= MAX_LEN):
        raise ValueError("image_density: ny and nx must lie in 2 .. %d" % MAX_LEN)
    if reverse and code != LAYOUT_SINGLE:
        raise ValueError("image_density: reverse belongs to the 'single' layout")
    if device is None:
        return _density_twin(imgs, ny, nx, code, bool(reverse), float(lower_bound))
    keep = [np.asfortranarray(i) for i in imgs]
    arr = (_Image * len(keep))(*[_Image(k.ctypes.data, k.shape[0], k.shape[1], 1 if k.ndim == 2 else 3) for k in keep])
    opts = capi.ImageOpts(ny, nx, code, int(bool(reverse)), float(lower_bound))
    rho = np.empty((ny, nx), order="F")
    capi.check(capi.lib().dotsocp_image_density(ctypes.byref(opts), arr, len(keep), capi.fptr(rho), int(device)))
    return rho


def imresize_device(a, size, device=0):
    """dotsocp_imresize on device `device`: the same arrays as imresize() takes and returns"""
    a = np.asarray(a)
    if a.dtype not in (np.uint8, np.float64) or a.ndim not in (2, 3):
        raise ValueError("imresize: a uint8 or float64 array (h, w) or (h, w, planes)")
    src = np.asfortranarray(a.reshape(a.shape[0], a.shape[1], -1))
    out = np.empty((int(size[0]), int(size[1]), src.shape[2]), dtype=a.dtype, order="F")
    capi.check(capi.lib().dotsocp_imresize(out.ctypes.data, src.ctypes.data, IMG_U8 if a.dtype == np.uint8 else IMG_F64,
                                           src.shape[0], src.shape[1], src.shape[2], out.shape[0], out.shape[1], int(device)))
    return out.reshape(out.shape[:2] + a.shape[2:])


def imresize_table_c(n_in, n_out):
    """dotsocp_imresize_table (host arithmetic of the library, no device): (weights, indices) as imresize_table returns them"""
    L = capi.lib()
    P = L.dotsocp_imresize_taps(int(n_in), int(n_out))
    if P < 0:
        raise capi.DotsocpError(P, L.dotsocp_last_error().decode())
    w = np.empty(int(n_out) * P)
    idx = np.empty(int(n_out) * P, dtype=np.int32)
    taps = ctypes.c_int()
    capi.check(L.dotsocp_imresize_table(int(n_in), int(n_out), capi.fptr(w), idx.ctypes.data, ctypes.byref(taps)))
    t = taps.value
    return w[:int(n_out) * t].reshape(int(n_out), t).copy(), idx[:int(n_out) * t].reshape(int(n_out), t).copy()


# ------------------------------------------------------------------------------------------ the reference's examples
def get_example_from_images(path_to_img1, path_to_img2, nx, ny, ReverseColor=False, device=None):
    """examples/dot2d/get_example_from_images.m: two pictures -> (rho0, rho1) of shape (ny, nx), each of mean 1"""
    return tuple(image_density([imread(p)], ny, nx, "single", ReverseColor, 0.0, device) for p in (path_to_img1, path_to_img2))


def _example5_images(resources):
    return [imread(os.path.join(str(resources), name)) for name in ("centaur.bmp", "man.bmp")]


def gene_example5(nx, ny, resources):
    """examples/dot2d/gene_example5.m (Example 5.5, centaur -> man): resized, inverted, padded; NOT normalised, as in the file"""
    return tuple(_raw_density([img], int(ny), int(nx), LAYOUT_SINGLE, True) for img in _example5_images(resources))


def _stitch_images(type, stitch1, stitch2, resources):
    kind = "classicimages" if type is None else str(type).lower()
    if kind not in ("classicimages", "shapes"):
        raise ValueError("type (pos 3) must be 'ClassicImages' or 'Shapes'")
    stitch1 = [1, 2, 3, 4] if stitch1 is None else list(stitch1)
    stitch2 = [5, 6, 7, 8] if stitch2 is None else list(stitch2)
    if len(stitch1) != 4:
        raise ValueError("stitch1_indices (pos 4) must be a vector of length 4")
    if len(stitch2) != 4:
        raise ValueError("stitch2_indices (pos 5) must be a vector of length 4")
    folder = os.path.join(str(resources), "DOTmark", "ClassicImages" if kind == "classicimages" else "Shapes")
    return [[imread(os.path.join(folder, "%d.png" % int(i))) for i in s] for s in (stitch1, stitch2)]


def gene_example_DOTmark_4stitch(nx, ny, type=None, stitch1=None, stitch2=None, resources=None):
    """examples/dot2d/gene_example_DOTmark_4stitch.m (Example 5.6): four DOTmark pictures per density, [1 2; 3 4]; NOT
    normalised, as in the file.  The double resize overshoots on binary pictures (negative entries): the reference's
    behaviour, restated."""
    if resources is None:
        raise ValueError("gene_example_DOTmark_4stitch needs resources=: the directory that holds DOTmark/")
    return tuple(_raw_density(imgs, int(ny), int(nx), LAYOUT_STITCH4, False) for imgs in _stitch_images(type, stitch1, stitch2, resources))


def get_example_2d_images(problem, nx, ny, lowerBound=0.0, resources=None, DOTmark_type=None, stitch1_indices=None,
                          stitch2_indices=None, device=None):
    """The two image-based rows of examples/dot2d/get_example.m:32-46 ("example5", "DOTmark_4stitch"), normalised with
    lowerBound as there; examples.get_example_2d forwards to it."""
    if resources is None:
        raise ValueError("Novalid input: 'Problem' (%s reads image files: pass resources=, the directory that holds them)" % problem)
    if problem == "example5":
        return tuple(image_density([i], ny, nx, "single", True, lowerBound, device) for i in _example5_images(resources))
    if problem == "DOTmark_4stitch":
        return tuple(image_density(s, ny, nx, "stitch4", False, lowerBound, device)
                     for s in _stitch_images(DOTmark_type, stitch1_indices, stitch2_indices, resources))
    raise ValueError("Novalid input: 'Problem'")


# ------------------------------------------------------------------------------------------ the labyrinths
class ImageBarrier:
    """barrier(x, y) = the nearest sample of a picture whose ROWS run along x (ndgrid(linspace(0, 1, n0), linspace(0, 1, n1))
    with griddedInterpolant(..., "nearest")): index floor(x (n0 - 1) + 0.5), exact midpoints go up, clamped to the picture."""

    def __init__(self, picture):
        self.picture = np.asarray(picture, dtype=np.float64)
        if self.picture.ndim != 2:
            raise ValueError("a barrier picture is a gray image")

    def __call__(self, x, y):
        n0, n1 = self.picture.shape
        i = np.clip(np.floor(np.asarray(x, dtype=np.float64) * float(n0 - 1) + 0.5), 0, n0 - 1).astype(np.int64)
        j = np.clip(np.floor(np.asarray(y, dtype=np.float64) * float(n1 - 1) + 0.5), 0, n1 - 1).astype(np.int64)
        return self.picture[i, j]


def barrier_of_image(img):
    """(max - img) * (255 / max) in MATLAB's saturating uint8 arithmetic (255 / max is rounded to an integer there), as an
    ImageBarrier"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("a barrier picture is a gray uint8 image")
    top = int(img.max())
    if top == 0:
        raise ValueError("a barrier picture that is black everywhere")
    factor = min(255, int(math.floor(255.0 / top + 0.5)))
    return ImageBarrier(np.minimum((top - img.astype(np.int64)) * factor, 255))


def gene_barrier_of_example6(resources):
    """examples/wdot2d/gene_barrier_of_example6.m: the labyrinth of Example 5.6 from resources/maze.png"""
    return barrier_of_image(imread(os.path.join(str(resources), "maze.png")))


def gene_barrier_of_maze14(resources):
    """examples/wdot2d/gene_barrier_of_maze14.m: the labyrinth of Papadakis, Peyre, Oudet (2014) from resources/maze-14.png"""
    return barrier_of_image(imread(os.path.join(str(resources), "maze-14.png")))
