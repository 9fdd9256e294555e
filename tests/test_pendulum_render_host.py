"""Pendulum-v1 frames without a device: the NumPy twin against the reference's recorded draw lists, the PNG decoder, the blit's window
means, and every argument refusal of the arrow_image= surfaces (they come before any device work)."""
import ctypes
import importlib.util
import io
import os
import zlib

import numpy as np
import pytest

import pendulum_render_host as prh
import pixels_host as ph
import render_host as rh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "render_pendulum.npz"))


def test_twin_records_equal_the_reference_draw_lists(golden):
    g = golden
    assert tuple(g["dims"]) == (prh.H, prh.W) and int(g["fps"]) == prh.FPS
    assert g["flip"].all()
    for i in range(len(g["states"])):
        ours = prh.scene(g["states"][i], g["last_u"][i])
        theirs = prh.golden_records(g, i)
        assert np.array_equal(ours, theirs), (i, g["states"][i], g["last_u"][i], ours, theirs)


def test_golden_covers_the_cases_the_rule_depends_on(golden):
    g = golden
    u = g["last_u"]
    has = g["blit"][:, 0] == 1
    assert (np.isnan(u) == ~has)[~g["raised"]].all()
    assert np.isnan(g["states"][:, 0]).any() and np.isinf(g["states"][:, 0]).any() and g["raised"].any()
    assert (np.abs(g["states"][:, 0][np.isfinite(g["states"][:, 0])]) >= 1e3).sum() >= 5
    sizes = g["blit"][has, 3]
    assert (sizes == 0).any() and (sizes == 1).any()
    assert ((u == 0) & np.signbit(u)).any() and ((u == 0) & ~np.signbit(u)).any()
    # sizes where float32 (the reference under NumPy 2) and float64 evaluation truncate to different integers
    div = [i for i in np.flatnonzero(has) if int(prh.SCALE * abs(float(u[i])) / 2) != g["blit"][i, 3]]
    assert len(div) >= 5
    assert all(g["blit"][i, 3] == prh.blit_size(u[i]) for i in np.flatnonzero(has))
    # clipped through the reference's own step(): last_u is the float32 clip of the raw action
    stepped = ~np.isnan(g["pre_state"][:, 0])
    assert stepped.sum() >= 20 and set(g["max_torque"][stepped]) == {2.0, 0.7}
    for i in np.flatnonzero(stepped):
        assert np.float32(u[i]).tobytes() == prh.clip(g["action"][i], g["max_torque"][i]).tobytes()
    assert (np.abs(g["action"][stepped]) > g["max_torque"][stepped]).sum() >= 10


def test_fixture_is_the_reference_asset():
    p = os.path.join(GOLDEN, "clockwise.png")
    assert os.path.getsize(p) == 6992
    img = prh.arrow()
    assert img.shape == (312, 329, 4) and img.dtype == np.uint8
    assert img[..., 3].min() == 0 and img[..., 3].max() == 255


def test_png_decoder_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    from gym_amd.arrow import decode_png

    ours = prh.arrow()
    theirs = np.asarray(Image.open(os.path.join(GOLDEN, "clockwise.png")).convert("RGBA"))
    assert np.array_equal(ours, theirs)
    # every filter type and the RGB colour type, through Pillow's encoder
    rng = np.random.default_rng(3)
    for mode, ch in (("RGB", 3), ("RGBA", 4)):
        arr = (rng.integers(0, 256, (17, 23, ch)) // 7 * 7).astype(np.uint8)
        arr[5:9] = arr[4]                       # rows the Up / Paeth filters like
        buf = io.BytesIO()
        Image.fromarray(arr, mode).save(buf, format="PNG", optimize=True)
        out = decode_png(buf.getvalue())
        want = arr if ch == 4 else np.concatenate([arr, np.full(arr.shape[:2] + (1,), 255, np.uint8)], axis=2)
        assert np.array_equal(out, want)


def _png(width, height, depth, ctype, interlace, raw):
    def chunk(kind, body):
        return len(body).to_bytes(4, "big") + kind + body + (zlib.crc32(kind + body) & 0xFFFFFFFF).to_bytes(4, "big")

    ihdr = width.to_bytes(4, "big") + height.to_bytes(4, "big") + bytes([depth, ctype, 0, 0, interlace])
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


def test_png_decoder_filters_and_refusals():
    from gym_amd.arrow import decode_png

    # one RGBA row per filter type 0..4 over known bytes, decoded by hand
    w = 2
    rows = [bytes([0, 10, 20, 30, 40, 50, 60, 70, 80]),          # None
            bytes([1, 1, 1, 1, 1, 1, 1, 1, 1]),                   # Sub: left + 1
            bytes([2, 1, 2, 3, 4, 5, 6, 7, 8]),                   # Up
            bytes([3, 0, 0, 0, 0, 0, 0, 0, 0]),                   # Average
            bytes([4, 0, 0, 0, 0, 0, 0, 0, 0])]                   # Paeth
    img = decode_png(_png(w, 5, 8, 6, 0, b"".join(rows)))
    r0 = np.array([[10, 20, 30, 40], [50, 60, 70, 80]])
    r1 = np.array([[1, 1, 1, 1], [2, 2, 2, 2]])
    r2 = r1 + np.array([[1, 2, 3, 4], [5, 6, 7, 8]])
    r3 = np.array([r2[0] // 2, (r2[0] // 2 + r2[1]) // 2])
    assert np.array_equal(img[0], r0) and np.array_equal(img[1], r1) and np.array_equal(img[2], r2) and np.array_equal(img[3], r3)
    assert np.array_equal(img[4], r3)            # Paeth over zeros: up wins for the first pixel, then left/up ties
    for args in ((2, 1, 16, 6, 0), (2, 1, 8, 0, 0), (2, 1, 8, 3, 0), (2, 1, 8, 6, 1)):
        with pytest.raises(ValueError, match="pass arrow_image"):
            decode_png(_png(*args, bytes(1 + 2 * 8)))
    with pytest.raises(ValueError, match="pass arrow_image"):
        decode_png(b"GIF89a")
    with pytest.raises(ValueError, match="filter"):
        decode_png(_png(1, 1, 8, 6, 0, bytes([7, 1, 2, 3, 4])))


def test_window_means_from_the_table_equal_direct_means():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (13, 9, 4)).astype(np.uint8)
    for h, w in ((1, 1), (13, 9), (5, 4), (26, 18), (31, 7), (2, 40)):
        got = prh.window_means(img, h, w)
        rows, cols = np.array(ph.windows(13, h)), np.array(ph.windows(9, w))
        for i in range(h):
            for j in range(w):
                blk = img[rows[i, 0]:rows[i, 1], cols[j, 0]:cols[j, 1]].astype(np.int64).reshape(-1, 4)
                n = len(blk)
                assert np.array_equal(got[i, j], (blk.sum(0) + n // 2) // n), (h, w, i, j)


def test_blit_is_drawn_in_place_and_size_zero_draws_nothing():
    img = prh.arrow()
    plain = prh.render([0.3, 0.0], np.nan, img)
    assert np.array_equal(prh.render([0.3, 0.0], np.float32(0.0), img), plain)
    assert np.array_equal(prh.render([0.3, 0.0], np.float32(0.01), img), plain)
    pos, neg = prh.render([0.3, 0.0], np.float32(1.5), img), prh.render([0.3, 0.0], np.float32(-1.5), img)
    assert not np.array_equal(pos, plain) and not np.array_equal(pos, neg)
    # the arrow flips horizontally with the sign: the blits of +u and -u alone are mirror images inside their common box
    rec, rneg = prh.scene([0.3, 0.0], np.float32(1.5))[6], prh.scene([0.3, 0.0], np.float32(-1.5))[6]
    assert rec[0] == prh.OP_BLIT and rec[6] == rec[7] == 85 and rec[8] == 1 and rec[9] == 1
    assert rneg[0] == prh.OP_BLIT and rneg[8] == 0 and np.array_equal(rec[4:8], rneg[4:8])
    x0, w = int(rec[4]), int(rec[6])
    a, b = prh.rasterize([rec], img), prh.rasterize([rneg], img)
    assert np.array_equal(a[:, x0:x0 + w], b[:, x0:x0 + w][:, ::-1])
    assert not np.array_equal(a, b) and (a[:, :x0] == 255).all() and (a[:, x0 + w:] == 255).all()


def test_argument_refusals_come_before_device_work():
    import gym_amd
    from gym_amd import _native, _render
    from gym_amd.vector_env import HipVectorEnv

    img = prh.arrow()
    with pytest.raises(TypeError, match="arrow_image"):
        HipVectorEnv("CartPole-v1", 2, arrow_image=img)
    with pytest.raises(TypeError, match="arrow_image"):
        gym_amd.make("Acrobot-v1", 2, render_mode="rgb_array", arrow_image=img)
    with pytest.raises(TypeError, match="arrow_image"):
        gym_amd.DeviceRollout("MountainCar-v0", 4, arrow_image=img)
    with pytest.raises(TypeError, match="arrow_image"):
        gym_amd.PixelRollout("CartPole-v1", 4, arrow_image=img)
    from gym_amd.single_env import HipEnv

    with pytest.raises(TypeError, match="arrow_image"):
        HipEnv("CartPole-v1", render_mode="rgb_array", arrow_image=img)
    bad = [(img[..., :3], ValueError), (img.astype(np.int16), ValueError), (np.zeros((0, 4, 4), np.uint8), ValueError),
           (np.zeros((1025, 4, 4), np.uint8), ValueError), (np.zeros((4, 1025, 4), np.uint8), ValueError), (img[0], ValueError),
           ([[[0, 0, 0, 0]]], TypeError), (os.path.join(GOLDEN, "no_such.png"), FileNotFoundError)]
    for value, exc in bad:
        with pytest.raises(exc):
            HipVectorEnv("Pendulum-v1", 2, render_mode="rgb_array", arrow_image=value)
        with pytest.raises(exc):
            HipEnv("Pendulum-v1", render_mode="rgb_array", arrow_image=value)
        with pytest.raises(exc):
            gym_amd.DeviceRollout("Pendulum-v1", 4, arrow_image=value)
        with pytest.raises(exc):
            gym_amd.PixelRollout("Pendulum-v1", 4, arrow_image=value)
    # without arrow_image every refusal stays what it was
    with pytest.raises(NotImplementedError, match="clockwise.png"):
        HipVectorEnv("Pendulum-v1", 1, render_mode="rgb_array")
    with pytest.raises(NotImplementedError, match="clockwise.png"):
        gym_amd.PixelRollout("Pendulum-v1", 4)
    with pytest.raises(NotImplementedError, match="clockwise.png"):
        _render.dims(_native.PENDULUM)
    # the C ABI's argument checks need no device either
    lib = _native.lib
    h, w = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mxv_render_frame_dims(None, ctypes.byref(h), ctypes.byref(w)) == _native.ERR_INVALID_ARG
    assert lib.mxv_render_attach_image(None, img.ctypes.data, 312, 329) == _native.ERR_INVALID_ARG
    buf = np.zeros(4, np.float32)
    assert lib.mxv_render_get_torques_host(None, buf.ctypes.data) == _native.ERR_INVALID_ARG
    assert lib.mxv_render_set_torques_host(None, buf.ctypes.data) == _native.ERR_INVALID_ARG
    assert lib.mxv_render_dims(_native.PENDULUM, ctypes.byref(h), ctypes.byref(w)) == _native.ERR_UNSUPPORTED
    assert _render.PENDULUM_RENDER_FPS == 30


def test_pendulum_arrow_image_finds_an_installed_gym():
    from gym_amd import pendulum_arrow_image

    spec = importlib.util.find_spec("gym")
    roots = list(spec.submodule_search_locations or []) if spec is not None else []
    if not any(os.path.isfile(os.path.join(r, "envs", "classic_control", "assets", "clockwise.png")) for r in roots):
        with pytest.raises(FileNotFoundError, match="arrow_image"):
            pendulum_arrow_image()
        pytest.skip("no installed gym carries the asset here")
    assert np.array_equal(pendulum_arrow_image(), prh.arrow())
