"""Looking at a solution: frames of the density evolution, filled levels, the arrows of the flux -- as arrays of bytes.

Host twins (numpy, no plotting library) of what the reference's demos draw from the outputs of a solve --
utils/show_evolution_2d.m ("imshow", "contourf"), utils/export_evolution_2d.m (the inverted gray frames, the frame nodes),
utils/show_movement_2d.m (the arrows) -- and of the device call that forms the same bytes from the device-resident state
(include/dotsocp.h: dotsocp_render_evolution; InPALMContext.render(), the drivers' render=dict(...)).  The definitions are
those of the header, restated operation by operation: uint8 pictures are equal, doubles are equal as bytes.

    vmax       max of rho over all finite nodes that are not set in `barrier` (the reference paints barrier nodes Inf before
               it takes the maximum, show_evolution_2d.m:36,52, and so loses its own scale; not followed)
    "imshow"   i = 0 for rho <= 0 or NaN, else min(255, floor((rho / vmax) * 256.0))      imshow(rho, [0, vmax])
    "inverted" 255 - that                                                                 imshow(vmax - rho, [0, vmax])
    "levels"   i = number of levels <= rho * (255.0 / vmax), levels = log_levels(n)       contourf without its lines
    barrier nodes get barrier_index in every mode

Pictures are C-ordered uint8 arrays (nf, ny, nx[, 3]) -- x fastest, one image row per y, as imshow(rho(:,:,t)) shows it; 1-D
problems give (nf, nx[, 3]), with all nodes requested the space-time diagram.  A colour table is any (256, 3) uint8 array:
gray_lut(), ramp_lut(anchors), or one of the caller's (the reference's custom_turbo table is not shipped).  write_png() writes
8-bit gray or RGB files with zlib and struct alone.
"""
import struct
import zlib

import numpy as np

MODES = {"imshow": 0, "inverted": 1, "levels": 2}       # DOTSOCP_RENDER_LINEAR / _INVERTED / _LEVELS
MASK_FRAC = 0.01                                        # show_movement_2d.m:31: arrows vanish where rho < max(rho) / 1e2


def barrier_mask(barrier, shape):
    """The boolean mask of `shape` = (ny, nx) (1-D: (nx,)) from an array of that shape (non-zero = masked) or from a
    barrier function of the examples (gene_barrier_of_*: f(x, y) on the node grid, as ensure_barrier_validity evaluates
    it); None stays None."""
    if barrier is None:
        return None
    if callable(barrier):
        ny, nx = shape
        xx, yy = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny))
        barrier = np.asarray(barrier(xx, yy)) > 0
    b = np.asarray(barrier) != 0
    if b.shape != tuple(shape):
        raise ValueError("the barrier mask must have the shape of a node layer, %r" % (tuple(shape),))
    return b


def rho_range(output, barrier=None):
    """dict(vmax, rho_min, nonfinite, masked) over all nt layers of output["rho"]: extrema over the finite nodes that are not
    masked (a -0.0 counts as +0.0; -Inf / +Inf if there is no such node), the unmasked nodes that are NaN or +-Inf, the masked
    nodes."""
    rho = np.asarray(output["rho"], dtype=np.float64)
    b = barrier_mask(barrier, rho.shape[:-1])
    keep = np.isfinite(rho)
    off = np.zeros(rho.shape, dtype=bool) if b is None else np.broadcast_to(b[..., None], rho.shape)
    vals = rho[keep & ~off] + 0.0
    return dict(vmax=float(vals.max()) if vals.size else float("-inf"), rho_min=float(vals.min()) if vals.size else float("inf"),
                nonfinite=int(np.count_nonzero(~keep & ~off)), masked=int(np.count_nonzero(off)))


def frame_nodes(nt, num_frame):
    """round(linspace(1, nt, num_frame)) - 1 (export_evolution_2d.m:129) with MATLAB's linspace (d1 + (0:n-1) * (d2 - d1) /
    (n - 1), the last point d2 itself; one point: d2) and MATLAB's round, half away from zero"""
    nt, n = int(nt), int(num_frame)
    if n < 1 or nt < 1:
        raise ValueError("frame_nodes() needs nt >= 1 and num_frame >= 1")
    if n == 1:
        v = np.array([float(nt)])
    else:
        v = 1.0 + (np.arange(n, dtype=np.float64) * float(nt - 1)) / float(n - 1)
        v[-1] = float(nt)
    r = np.floor(v)
    r = r + (v - r >= 0.5)                      # the values are positive: half away from zero is half up
    return r.astype(np.int64) - 1


def log_levels(n=128):
    """exp(linspace(0, log(255), n)) (show_evolution_2d.m:63,72): n strictly ascending doubles from 1 to 255, 1 <= n <= 254;
    the table the device compares against is this one"""
    n = int(n)
    if not 1 <= n <= 254:
        raise ValueError("log_levels() makes 1 to 254 levels")
    top = np.log(255.0)
    return np.exp(np.array([top]) if n == 1 else np.linspace(0.0, top, n))


def indices(rho, vmax, mode="imshow", levels=None, barrier=None, barrier_index=255):
    """uint8 array of the shape of rho: the index of every node (module docstring).  barrier: a mask of rho's shape or of
    its leading axes (a node layer)."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % sorted(MODES))
    rho = np.asarray(rho, dtype=np.float64)
    vmax = float(vmax)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mode == "levels":
            lv = np.asarray(log_levels(128) if levels is None else levels, dtype=np.float64)
            s = rho * (255.0 / vmax)
            i = np.where(np.isnan(s), 0, np.searchsorted(lv, s, side="right"))
        else:
            v = (rho / vmax) * 256.0
            i = np.where(rho > 0.0, np.minimum(v, 255.0), 0.0).astype(np.int64)     # (non-negative: the cast is floor)
            if mode == "inverted":
                i = 255 - i
    if barrier is not None:
        b = np.asarray(barrier) != 0
        if b.ndim < rho.ndim:
            b = b.reshape(b.shape + (1,) * (rho.ndim - b.ndim))
        i = np.where(b, int(barrier_index), i)
    return i.astype(np.uint8)


def _scale(rng, vmax):
    scale = float(vmax) if vmax is not None and vmax > 0 else rng["vmax"]
    if not (scale > 0 and np.isfinite(scale)):
        raise ValueError("the scale (the largest finite density, or vmax) is not a positive finite number")
    return scale


def render(output, frames=None, num_frame=6, mode="imshow", nlevels=128, levels=None, lut=None, barrier=None, vmax=None,
           barrier_index=255):
    """numpy twin of dotsocp_render_evolution without the arrows, from the `output` dict of the drivers /
    InPALMContext.outputs(): dict(image, nodes, vmax, rho_min, nonfinite, masked).  frames: node indices in any order, repeats
    allowed (None: frame_nodes(nt, num_frame)); lut: a (256, 3) uint8 table for RGB pictures; vmax > 0 fixes the scale."""
    rho = np.asarray(output["rho"], dtype=np.float64)
    nt = rho.shape[-1]
    b = barrier_mask(barrier, rho.shape[:-1])
    rng = rho_range(output, b)
    scale = _scale(rng, vmax)
    nodes = frame_nodes(nt, num_frame) if frames is None else np.array(frames, dtype=np.int64).ravel()
    if nodes.size < 1 or nodes.min() < 0 or nodes.max() >= nt:
        raise ValueError("frame nodes must lie in [0, nt)")
    if mode == "levels" and levels is None:
        levels = log_levels(nlevels)
    idx = indices(rho[..., nodes], scale, mode, levels, b, barrier_index)
    image = np.ascontiguousarray(np.moveaxis(idx, -1, 0))
    if lut is not None:
        image = check_lut(lut)[image]
    return dict(image=image, nodes=nodes, vmax=scale, rho_min=rng["rho_min"], nonfinite=rng["nonfinite"], masked=rng["masked"])


def movement_skips(ny, nx):
    """(skip_y, skip_x) as show_movement_2d.m:18-28 picks them: 1 up to 40 nodes, else floor(nx / 30) -- for BOTH axes the
    reference divides nx (:21,27)"""
    ny, nx = int(ny), int(nx)
    return (1 if ny <= 40 else nx // 30), (1 if nx <= 40 else nx // 30)


def movement(output, nodes, vmax, skip_y=1, skip_x=1, mask_frac=MASK_FRAC):
    """The arrows of show_movement_2d.m:31-33,45-46,56 at the frame nodes: dict(Ex, Ey) of Fortran-ordered arrays
    (my, mx, nf) -- output["Ex"] / ["Ey"] at y = 0, skip_y, .., x = 0, skip_x, .., bit for bit, except +0.0 where
    rho < vmax * mask_frac (strict).  1-D outputs: dict(Ex) of shape (mx, nf), skip_x along the axis."""
    rho = np.asarray(output["rho"], dtype=np.float64)
    nodes = np.array(nodes, dtype=np.int64).ravel()
    with np.errstate(invalid="ignore"):
        small = rho[..., nodes] < float(vmax) * float(mask_frac)
    cut = (slice(None, None, int(skip_x)),) if rho.ndim == 2 else (slice(None, None, int(skip_y)), slice(None, None, int(skip_x)))
    out = {}
    for k in ("Ex",) if rho.ndim == 2 else ("Ex", "Ey"):
        E = np.where(small, 0.0, np.asarray(output[k], dtype=np.float64)[..., nodes])
        out[k] = np.asfortranarray(E[cut])
    return out


def check_lut(lut):
    t = np.ascontiguousarray(lut)
    if t.dtype != np.uint8 or t.shape != (256, 3):
        raise ValueError("a colour table is a (256, 3) uint8 array")
    return t


def gray_lut():
    """index i -> (i, i, i)"""
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def ramp_lut(anchors):
    """Piecewise-linear table between RGB anchors (values 0 .. 255) spread evenly over the indices 0 .. 255: channels
    interpolated linearly and rounded to nearest."""
    a = np.asarray(anchors, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 2 or a.min() < 0 or a.max() > 255:
        raise ValueError("ramp_lut() needs at least two (r, g, b) anchors with values in 0 .. 255")
    pos = np.linspace(0.0, 255.0, a.shape[0])
    i = np.arange(256, dtype=np.float64)
    return np.stack([np.rint(np.interp(i, pos, a[:, c])) for c in range(3)], axis=1).astype(np.uint8)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, image):
    """8-bit PNG of a uint8 array (h, w): gray, or (h, w, 3): RGB.  Standard library only: one IDAT chunk, filter 0 on
    every row, no interlace."""
    im = np.ascontiguousarray(image)
    if im.dtype != np.uint8 or im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] != 3) or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError("write_png() takes a uint8 array (h, w) or (h, w, 3)")
    h, w = im.shape[:2]
    rows = np.empty((h, 1 + w * (3 if im.ndim == 3 else 1)), dtype=np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = im.reshape(h, -1)
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if im.ndim == 3 else 0, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(data)
    return path
