"""Pixel observations without a device: the host rule of tests/pixels_host.py against torch's adaptive_avg_pool2d on
random, binary and rendered frames, its anchors (identity, box mean, white), the C ABI's exports and argument checks, the refusals of
PixelRollout, and the resource budget of the pixel kernel (cross-compiled for gfx950)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pixels_host as ph  # noqa: E402
import render_host as rh  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "render_scenes.npz")
SIZES = {(400, 600): [(84, 84), (64, 96), (100, 150), (399, 599)], (500, 500): [(84, 84), (7, 13)]}


def _torch_rule(img: np.ndarray, h: int, w: int) -> np.ndarray:
    """floor(adaptive_avg_pool2d(float64) + 0.5): an independent statement of the area rule."""
    import torch

    t = torch.from_numpy(img.astype(np.float64))
    t = t[None, None] if img.ndim == 2 else t.permute(2, 0, 1)[None]
    r = torch.floor(torch.nn.functional.adaptive_avg_pool2d(t, (h, w)) + 0.5)[0]
    r = r[0] if img.ndim == 2 else r.permute(1, 2, 0)
    return r.numpy().astype(np.uint8)


@pytest.mark.parametrize("HW", list(SIZES))
def test_rule_equals_adaptive_avg_pool_on_random_and_binary_frames(HW):
    rng = np.random.default_rng(7)
    H, W = HW
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8), (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)]
    for f in frames:
        for h, w in SIZES[HW] + [(1, 1), (H, W)]:
            assert np.array_equal(ph.reduce(f, h, w, False), _torch_rule(f, h, w)), (HW, h, w)
            assert np.array_equal(ph.reduce(f, h, w, True), _torch_rule(ph.gray(f), h, w)), (HW, h, w)


def test_rule_equals_adaptive_avg_pool_on_rendered_frames():
    g = np.load(GOLDEN)
    for name in rh.DIMS:
        states, params = g[f"{name}_states"], g[f"{name}_params"]
        H, W = rh.DIMS[name]
        for i in range(0, len(states), max(1, len(states) // 6)):
            f = rh.render(name, states[i], params[i])
            for h, w in SIZES[(H, W)]:
                assert np.array_equal(ph.reduce(f, h, w, True), _torch_rule(ph.gray(f), h, w)), (name, i, h, w)
                assert np.array_equal(ph.reduce(f, h, w, False), _torch_rule(f, h, w)), (name, i, h, w)


def test_identity_box_mean_and_white():
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, (400, 600, 3), dtype=np.uint8)
    assert np.array_equal(ph.reduce(f, 400, 600, False), f)
    assert np.array_equal(ph.reduce(f, 400, 600, True), ph.gray(f))
    for h, w in ((200, 300), (100, 100), (40, 60), (8, 12)):       # integer ratios: a plain box mean with integer rounding
        ry, rx = 400 // h, 600 // w
        blocks = f.astype(np.int64).reshape(h, ry, w, rx, 3).sum(axis=(1, 3))
        n = ry * rx
        assert np.array_equal(ph.reduce(f, h, w, False), ((blocks + n // 2) // n).astype(np.uint8)), (h, w)
    assert sum(ph.GRAY_WEIGHTS) == 1 << 14
    white = np.full((400, 600, 3), 255, np.uint8)
    assert (ph.gray(white) == 255).all() and (ph.reduce(white, 84, 84) == 255).all()
    assert (ph.gray(np.zeros((1, 1, 3), np.uint8)) == 0).all()
    with pytest.raises(ValueError):
        ph.area_resize(f, 401, 600)
    with pytest.raises(ValueError):
        ph.area_resize(f, 84, 0)


def test_pixel_exports_match_the_header():
    from gym_amd import _native, _render

    text = open(os.path.join(ROOT, "include", "mxv_render.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mxv_[a-z_0-9]+)\s*\(", text)))
    assert {"mxv_pixels", "mxv_pixels_strided", "mxv_pixels_host"} <= set(declared)
    assert sorted(_render.RENDER_EXPORTS) == declared
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    assert not set(declared) & set(_native.EXPORTS)


def test_pixel_argument_checks_without_a_device():
    from gym_amd import _native, _render

    lib = _native.lib
    buf = np.zeros(64, np.uint8)
    assert lib.mxv_pixels(None, None, 1, 84, 84, 1, buf.ctypes.data) == _native.ERR_INVALID_ARG
    assert lib.mxv_pixels_host(None, None, 1, 84, 84, 1, buf.ctypes.data) == _native.ERR_INVALID_ARG
    assert lib.mxv_pixels_strided(None, None, 84, 84, 1, 1, buf.ctypes.data, 7056, 7056) == _native.ERR_INVALID_ARG
    assert _render.pixel_shape(_native.CARTPOLE, 84, 84, True) == (84, 84)
    assert _render.pixel_shape(_native.ACROBOT, 500, 500, False) == (500, 500, 3)
    for h, w in ((0, 84), (84, 0), (401, 84), (84, 601), (84.0, 84)):
        with pytest.raises(ValueError, match="height"):
            _render.pixel_shape(_native.CARTPOLE, h, w, True)
    with pytest.raises(ValueError):
        _render.pixel_shape(_native.ACROBOT, 84, 501, True)
    with pytest.raises(NotImplementedError, match="clockwise.png"):
        _render.pixel_shape(_native.PENDULUM, 84, 84, True)


def test_pixel_rollout_refusals_come_before_device_work():
    import gym_amd

    with pytest.raises(NotImplementedError, match="clockwise.png"):
        gym_amd.PixelRollout("Pendulum-v1", 4)
    for tid in ("FrozenLake-v1", "Taxi-v3", "CliffWalking-v0", "Blackjack-v1"):
        with pytest.raises(NotImplementedError, match="toy_text"):
            gym_amd.PixelRollout(tid, 4)
    with pytest.raises(ValueError, match="height"):
        gym_amd.PixelRollout("CartPole-v1", 4, height=0)
    with pytest.raises(ValueError, match="width"):
        gym_amd.PixelRollout("Acrobot-v1", 4, width=501)
    with pytest.raises(ValueError, match="stack"):
        gym_amd.PixelRollout("MountainCar-v0", 4, stack=0)


HIPCC = "/opt/rocm/bin/hipcc"


def _resources(remarks):
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: .*?(Function Name|VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k.split(" [")[0]] = int(v)
    return out


def test_pixel_kernel_resources():
    """pixels_kernel<H, W, C>: no VGPR spills, scratch no larger than render_kernel's, LDS within 64 KiB, and no scalar store."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "gym_amd", "csrc", "mxv_render.hip")
    d = tempfile.mkdtemp(prefix="mxv_pix_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", src,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage", "-save-temps"], cwd=d,
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        asm = open(os.path.join(d, [f for f in os.listdir(d) if f.endswith("gfx950.s")][0])).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res = _resources(p.stderr)
    render = [r for name, r in res.items() if "render_kernel" in name]
    pixels = {name: r for name, r in res.items() if "pixels_kernel" in name}
    assert len(render) == 2 and len(pixels) == 4, sorted(res)
    scratch_bound = max(r["ScratchSize"] for r in render)
    assert scratch_bound <= 48
    for name, r in pixels.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize"] <= scratch_bound, (name, r)
        assert r["LDS Size"] <= 64 * 1024, (name, r)
    assert not re.search(r"^\s*s_(buffer_|scratch_)?(store|atomic)", asm, flags=re.M | re.I)
    assert not re.search(r"^\s*s_dcache_(wb|discard)", asm, flags=re.M | re.I)
