"""Host side of the pictures (dot-socp_amd/render.py, include/dotsocp.h: dotsocp_render_evolution): the frame nodes, the
index of a density in the three modes at its exact boundaries, the arrow mask at its threshold, the barrier, the colour
tables, the PNG writer decoded by hand, and render() of a small oracle solve against the formulas written out here.  No GPU.
Every comparison is exact."""
import struct
import zlib

import numpy as np
import pytest

import dotsocp_amd as D
from dotsocp_amd import render as R
from oracle import driver as OD
from oracle.examples import get_example_2d


def test_frame_nodes():
    assert R.frame_nodes(33, 6).tolist() == [0, 6, 13, 19, 26, 32]
    assert R.frame_nodes(4, 3).tolist() == [0, 2, 3]              # 2.5 rounds away from zero; numpy's round gives 2 -> node 1
    assert int(np.round(2.5)) - 1 == 1
    assert R.frame_nodes(9, 1).tolist() == [8]                    # linspace(1, nt, 1) is nt
    assert R.frame_nodes(9, 9).tolist() == list(range(9))
    assert R.frame_nodes(33, 6).dtype == np.int64


def test_linear_index_at_its_boundaries():
    vmax = 2.0
    j = np.arange(257)
    rho = vmax * j / 256
    want = np.minimum(j, 255)
    assert np.array_equal(R.indices(rho, vmax), want.astype(np.uint8))
    assert np.array_equal(R.indices(rho, vmax, "inverted"), (255 - want).astype(np.uint8))
    below = np.nextafter(rho[1:], 0)                              # one ulp under a boundary: the index before it
    assert np.array_equal(R.indices(below, vmax), (want[1:] - (j[1:] <= 255)).astype(np.uint8))
    odd = np.array([-1.0, -0.0, 0.0, np.nan, np.inf, -np.inf, 5 * vmax])
    assert R.indices(odd, vmax).tolist() == [0, 0, 0, 0, 255, 0, 255]
    assert R.indices(odd, vmax, "inverted").tolist() == [255, 255, 255, 255, 0, 255, 0]
    assert R.indices(rho, vmax).dtype == np.uint8


@pytest.mark.parametrize("n", [1, 2, 128, 254])
def test_levels(n):
    lv = R.log_levels(n)
    assert lv.shape == (n,) and np.all(np.diff(lv) > 0) and abs(lv[-1] - 255) < 1e-10 and (n == 1 or lv[0] == 1.0)
    vmax = 510.0                                                  # k = 255 / 510 = 0.5: rho = 2 * level gives s = level exactly
    k = 255.0 / vmax
    assert k == 0.5
    got = R.indices(lv / k, vmax, "levels", levels=lv)
    assert np.array_equal(got, np.arange(1, n + 1).astype(np.uint8))          # s exactly on a level counts that level
    assert np.array_equal(R.indices(np.nextafter(lv, 0) / k, vmax, "levels", levels=lv), np.arange(n).astype(np.uint8))
    assert R.indices(np.array([0.0, -3.0, np.nan, np.inf, -np.inf]), vmax, "levels", levels=lv).tolist() == [0, 0, 0, n, 0]
    vmax = 3.7                                                    # a scale whose k is not exact: the count is taken from s itself
    rho = np.concatenate([lv / (255.0 / vmax), np.linspace(0, vmax, 50)])
    want = np.array([np.count_nonzero(lv <= v * (255.0 / vmax)) for v in rho])
    assert np.array_equal(R.indices(rho, vmax, "levels", levels=lv), want.astype(np.uint8))
    with pytest.raises(ValueError):
        R.log_levels(0)
    with pytest.raises(ValueError):
        R.log_levels(255)


def _hand_output():
    ny, nx, nt = 4, 5, 3
    rng = np.random.default_rng(3)
    rho = np.asfortranarray(rng.uniform(0.0, 1.0, (ny, nx, nt)))
    rho[1, 2, 1] = 8.0                                            # the maximum, a power of two
    Ex = np.asfortranarray(rng.normal(size=(ny, nx, nt)))
    Ey = np.asfortranarray(rng.normal(size=(ny, nx, nt)))
    return dict(rho=rho, Ex=Ex, Ey=Ey)


def test_arrow_mask_is_strict():
    out = _hand_output()
    vmax, frac = 8.0, 0.01
    thr = vmax * frac
    out["rho"][0, 0, 0] = thr                                     # keeps its arrow
    out["rho"][1, 0, 0] = np.nextafter(thr, 0)                    # loses it
    out["rho"][2, 0, 0] = np.nan                                  # a NaN is not smaller than anything
    out["Ex"][1, 0, 0] = -3.0
    mv = R.movement(out, [0, 2, 0], vmax, skip_y=1, skip_x=2, mask_frac=frac)
    assert mv["Ex"].shape == (4, 3, 3) and mv["Ex"].flags.f_contiguous and set(mv) == {"Ex", "Ey"}
    for k in ("Ex", "Ey"):
        assert mv[k][0, 0, 0] == out[k][0, 0, 0] and mv[k][2, 0, 0] == out[k][2, 0, 0]
        assert mv[k][1, 0, 0] == 0.0 and not np.signbit(mv[k][1, 0, 0])
        keep = out["rho"][:, ::2, [0, 2, 0]] >= thr
        assert np.array_equal(mv[k][keep], out[k][:, ::2, [0, 2, 0]][keep])
        assert np.all(mv[k][out["rho"][:, ::2, [0, 2, 0]] < thr] == 0.0)
    big = R.movement(out, [1], vmax, skip_y=7, skip_x=9)
    assert big["Ey"].shape == (1, 1, 1)
    one_d = dict(rho=out["rho"][:, 0, :], Ex=out["Ey"][:, 0, :])
    assert set(R.movement(one_d, [0, 1], vmax, skip_x=3)) == {"Ex"} and R.movement(one_d, [0, 1], vmax, skip_x=3)["Ex"].shape == (2, 2)
    assert R.movement_skips(129, 129) == (4, 4) and R.movement_skips(40, 41) == (1, 1) and R.movement_skips(41, 90) == (3, 3)
    assert R.movement_skips(90, 40) == (1, 1)                     # the reference divides nx for both axes


def test_barrier_stays_out_of_the_range_and_gets_its_index():
    out = _hand_output()
    b = np.zeros((4, 5), dtype=bool)
    b[1, 2] = b[3, 4] = True                                      # the node of the maximum is masked
    out["rho"][0, 1, 2] = np.inf
    out["rho"][3, 4, 0] = np.nan                                  # masked: not counted as non-finite
    free = R.rho_range(out)
    rng = R.rho_range(out, b)
    rest = out["rho"][np.isfinite(out["rho"]) & ~b[:, :, None]]
    assert free["vmax"] == 8.0 and free["nonfinite"] == 2 and free["masked"] == 0
    assert rng == dict(vmax=rest.max(), rho_min=rest.min(), nonfinite=1, masked=6)
    r = R.render(out, frames=[1, 0], barrier=b, barrier_index=77)
    assert r["image"].shape == (2, 4, 5) and r["image"].flags.c_contiguous and r["vmax"] == rest.max()
    assert np.all(r["image"][:, b] == 77)
    want = R.indices(out["rho"][:, :, 1], rest.max())
    assert np.array_equal(r["image"][0][~b], want[~b])
    lev = R.render(out, frames=[1], mode="levels", nlevels=5, barrier=lambda x, y: (x > 0.4) & (x < 0.6) & (y > 0.3) & (y < 0.4))
    assert lev["masked"] == 3 and lev["image"][0, 1, 2] == 255 and lev["image"].max() == 255 and np.all(np.delete(lev["image"].ravel(), 7) <= 5)
    with pytest.raises(ValueError):
        R.render(dict(rho=-np.ones((2, 2, 2))))                   # no positive scale
    with pytest.raises(ValueError):
        R.render(out, frames=[3])


def test_colour_tables():
    g = R.gray_lut()
    assert g.shape == (256, 3) and g.dtype == np.uint8 and np.array_equal(g[:, 1], np.arange(256))
    t = R.ramp_lut([(0, 0, 0), (255, 0, 10), (255, 255, 20)])
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert t[0].tolist() == [0, 0, 0] and t[255].tolist() == [255, 255, 20] and t[51].tolist() == [102, 0, 4]
    assert np.all(np.diff(t[:, 0].astype(int)) >= 0)
    out = _hand_output()
    rgb = R.render(out, frames=[2], lut=t)["image"]
    assert rgb.shape == (1, 4, 5, 3) and np.array_equal(rgb, t[R.render(out, frames=[2])["image"]])
    with pytest.raises(ValueError):
        R.ramp_lut([(0, 0, 0)])
    with pytest.raises(ValueError):
        R.render(out, lut=np.zeros((256, 4), dtype=np.uint8))


def _decode_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xffffffff
        chunks.append((kind, data))
        pos += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT")), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert np.all(rows[:, 0] == 0)                                # filter type 0 on every row
    return rows[:, 1:].reshape((h, w, 3) if ch == 3 else (h, w))


@pytest.mark.parametrize("shape", [(7, 5), (7, 5, 3), (9, 1), (1, 6, 3)])
def test_write_png(tmp_path, shape):
    im = np.random.default_rng(len(shape) + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    assert R.write_png(path, im) == path
    assert np.array_equal(_decode_png(path), im)
    R.write_png(path, np.asfortranarray(im))                      # any memory order
    assert np.array_equal(_decode_png(path), im)
    with pytest.raises(ValueError):
        R.write_png(path, im.astype(np.int32))
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(path)), im)


def test_render_of_an_oracle_solve_equals_the_formulas():
    rho0, rho1 = get_example_2d("example1", 17, 17)
    nt = 5
    var, model, hist, sigma = OD.solve_single_level(rho0, rho1, nt, dict(tol=1e-3, maxit=60))
    rho, Ex, Ey = OD.recover_RhoE(var, model)
    out = dict(rho=rho, Ex=Ex, Ey=Ey)
    vmax = rho.max()
    assert np.isfinite(rho).all() and vmax > 0
    r = R.render(out, num_frame=3)
    assert r["nodes"].tolist() == [0, 2, 4] and r["vmax"] == vmax and r["rho_min"] == rho.min() + 0.0
    assert r["nonfinite"] == 0 and r["masked"] == 0 and r["image"].shape == (3, 17, 17) and r["image"].dtype == np.uint8
    lv = np.exp(np.linspace(0, np.log(255.0), 16))
    rl = R.render(out, num_frame=3, mode="levels", nlevels=16)
    ri = R.render(out, num_frame=3, mode="inverted", vmax=2 * vmax)
    assert ri["vmax"] == 2 * vmax
    for f, t in enumerate([0, 2, 4]):
        for y in range(17):
            for x in range(17):
                v = rho[y, x, t]
                lin = 0 if not v > 0 else min(255, int(np.floor((v / vmax) * 256.0)))
                assert r["image"][f, y, x] == lin
                assert rl["image"][f, y, x] == sum(1 for e in lv if e <= v * (255.0 / vmax))
                assert ri["image"][f, y, x] == 255 - (0 if not v > 0 else min(255, int(np.floor((v / (2 * vmax)) * 256.0))))
    assert np.array_equal(r["image"][0], R.indices(np.asarray(rho0, dtype=np.float64), vmax))     # frame 0 is rho0 itself
    assert r["image"].max() == 255 and len(np.unique(rl["image"])) > 4
    mv = R.movement(out, r["nodes"], vmax, 2, 3)
    small = rho[::2, ::3, ::2] < vmax * 0.01
    assert small.any() and not small.all()
    assert np.array_equal(mv["Ex"], np.where(small, 0.0, Ex[::2, ::3, ::2])) and mv["Ey"].shape == (9, 6, 3)


@pytest.mark.parametrize("driver", ["solver_dotsocp2d", "solver_dotsocp1d", "solver_wdotsocp2d"])
def test_render_needs_the_device_transfer(driver):
    one_d = driver.endswith("1d")
    rho = np.ones(9) if one_d else np.ones((9, 9))
    with pytest.raises(ValueError, match="render= needs transfer='device'"):
        getattr(D, driver)(rho, rho, 5, 1, dict(tol=1e-3, weight=None), transfer="host", render=dict(num_frame=2))
