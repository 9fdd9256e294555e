"""ctypes binding of include/mxv_render.h: rgb_array frames of the classic-control envs, drawn on the device, and the
pixel observations reduced from them.

The header is optional (mxv.h does not include it), so its symbols are bound here, over the same library as gym_amd._native, and are
not part of _native.EXPORTS.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

RENDER_EXPORTS = ("mxv_render_dims", "mxv_render", "mxv_render_host", "mxv_render_scene_host", "mxv_pixels", "mxv_pixels_strided",
                  "mxv_pixels_host", "mxv_render_frame_dims", "mxv_render_attach_image", "mxv_render_get_torques_host",
                  "mxv_render_set_torques_host")
RECORD_INTS = 12
MAX_RECORDS = 112
# frames per second of the reference's metadata (cartpole.py:89, acrobot.py:96, mountain_car.py:100, continuous_mountain_car.py:105)
RENDER_FPS = {_native.CARTPOLE: 50, _native.ACROBOT: 15, _native.MOUNTAINCAR: 30, _native.MOUNTAINCAR_CONT: 30}
PENDULUM_RENDER_FPS = 30   # pendulum.py:90-93 (its frames need the caller's arrow image: arrow_image=)
PENDULUM_REASON = ("Pendulum-v1 has no rgb_array frames on the device engine: its frame blits the reference's image asset "
                   "(assets/clockwise.png, pendulum.py:228-244), which the engine does not carry")

lib = _native.lib
lib.mxv_render_dims.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
lib.mxv_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.mxv_render_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.mxv_render_scene_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.mxv_pixels.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
lib.mxv_pixels_strided.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64]
lib.mxv_pixels_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
lib.mxv_render_frame_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
lib.mxv_render_attach_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
lib.mxv_render_get_torques_host.argtypes = [C.c_void_p, C.c_void_p]
lib.mxv_render_set_torques_host.argtypes = [C.c_void_p, C.c_void_p]
for _name in RENDER_EXPORTS:
    getattr(lib, _name).restype = C.c_int


def dims(env_id: int):
    """(H, W) of an env kind's frame; NotImplementedError for Pendulum."""
    h, w = C.c_int32(), C.c_int32()
    rc = lib.mxv_render_dims(int(env_id), C.byref(h), C.byref(w))
    if rc == _native.ERR_UNSUPPORTED:
        raise NotImplementedError(PENDULUM_REASON)
    if rc != _native.OK:
        raise _native.MxvError(rc, f"unknown env_id {env_id}")
    return h.value, w.value


def frame_dims(handle):
    """(H, W) of a handle's frames: dims() of its kind; 500 x 500 for a Pendulum handle with an arrow image attached (NotImplementedError
    without one)."""
    if handle.env_id != _native.PENDULUM:
        return dims(handle.env_id)
    if getattr(handle, "_arrow_image", None) is None:
        raise NotImplementedError(PENDULUM_REASON)
    h, w = C.c_int32(), C.c_int32()
    handle._check(lib.mxv_render_frame_dims(handle._h, C.byref(h), C.byref(w)))
    return h.value, w.value


def arrow_kwarg(env_id: int, id: str, arrow_image):
    """The `arrow_image=` argument of a constructor, checked before any device work: None stays None; for Pendulum-v1 a uint8 (H, W, 4)
    array (gym_amd.arrow.as_arrow_image); for any other id a TypeError, like every unexpected keyword argument."""
    if arrow_image is None:
        return None
    if env_id != _native.PENDULUM:
        raise TypeError(f"{id} got an unexpected keyword argument 'arrow_image' (only Pendulum-v1 frames blit an image)")
    from .arrow import as_arrow_image

    return as_arrow_image(arrow_image)


def attach_image(handle, image: np.ndarray):
    """Attach Pendulum's arrow image (a checked uint8 (H, W, 4) array) to `handle`: frames and pixels become available and last_u is
    tracked from here on, every env at None.  Synchronises."""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    handle._check(lib.mxv_render_attach_image(handle._h, img.ctypes.data, img.shape[0], img.shape[1]))
    handle._arrow_image = img


def get_torques(handle) -> np.ndarray:
    """float32 (N,): every env's last_u (NaN = None).  Synchronises."""
    out = np.empty(handle.num_envs, np.float32)
    handle._check(lib.mxv_render_get_torques_host(handle._h, out.ctypes.data))
    return out


def set_torques(handle, last_u):
    u = np.ascontiguousarray(last_u, dtype=np.float32).reshape(handle.num_envs)
    handle._check(lib.mxv_render_set_torques_host(handle._h, u.ctypes.data))


def _indices_host(handle, indices):
    if indices is None:
        return None, handle.num_envs
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    if idx.size and (idx.min() < -(2 ** 31) or idx.max() >= 2 ** 31):
        raise IndexError("env index out of range")
    return idx.astype(np.int32), idx.size


def render_host(handle, indices=None) -> np.ndarray:
    """uint8 (k, H, W, 3) frames of envs `indices` (all when None) in host memory.  Synchronises."""
    H, W = frame_dims(handle)
    idx, k = _indices_host(handle, indices)
    out = np.empty((k, H, W, 3), np.uint8)
    if k == 0:
        return out
    handle._check(lib.mxv_render_host(handle._h, None if idx is None else idx.ctypes.data, k, out.ctypes.data))
    return out


def scene_host(handle, indices=None) -> np.ndarray:
    """int32 (k, MAX_RECORDS, RECORD_INTS): the integer draw lists the device computes for those frames.  Synchronises."""
    frame_dims(handle)
    idx, k = _indices_host(handle, indices)
    out = np.zeros((k, MAX_RECORDS, RECORD_INTS), np.int32)
    handle._check(lib.mxv_render_scene_host(handle._h, None if idx is None else idx.ctypes.data, k, out.ctypes.data))
    return out


def render_device(handle, frames, indices=None, count=None):
    """Frames into the device tensor `frames` (uint8 [count, H, W, 3]); `indices` an int32 device tensor or None.  Stream-ordered on the
    handle's stream, no synchronisation."""
    k = int(count if count is not None else (indices.numel() if indices is not None else handle.num_envs))
    handle._check(lib.mxv_render(handle._h, None if indices is None else indices.data_ptr(), k, frames.data_ptr()))


def pixel_shape(env_id: int, height: int, width: int, grayscale: bool, frame=None):
    """Shape of one pixel observation: (height, width) or (height, width, 3).  NotImplementedError for Pendulum (unless `frame`, the
    handle's (H, W) from frame_dims(), is given), ValueError for a size outside [1, H] x [1, W] of the frame."""
    H, W = dims(env_id) if frame is None else frame
    if not (isinstance(height, int) and isinstance(width, int) and 1 <= height <= H and 1 <= width <= W):
        raise ValueError(f"pixel observations are reduced from the {H} x {W} frame: height must lie in [1, {H}] and width in [1, {W}], "
                         f"got {height!r} x {width!r}")
    return (height, width) if grayscale else (height, width, 3)


def pixels_host(handle, height: int, width: int, grayscale: bool = True, indices=None) -> np.ndarray:
    """uint8 (k, h, w) or (k, h, w, 3) pixel observations of envs `indices` (all when None) in host memory.  Synchronises."""
    shape = pixel_shape(handle.env_id, height, width, grayscale, frame_dims(handle))
    idx, k = _indices_host(handle, indices)
    out = np.empty((k,) + shape, np.uint8)
    if k == 0:
        return out
    handle._check(lib.mxv_pixels_host(handle._h, None if idx is None else idx.ctypes.data, k, height, width, 1 if grayscale else 3,
                                      out.ctypes.data))
    return out


def pixels_device(handle, out, height: int, width: int, grayscale: bool = True, indices=None, count=None):
    """Pixel observations into the device tensor `out` (uint8 [count, h, w(, 3)]); `indices` an int32 device tensor or None.
    Stream-ordered on the handle's stream, no synchronisation."""
    k = int(count if count is not None else (indices.numel() if indices is not None else handle.num_envs))
    handle._check(lib.mxv_pixels(handle._h, None if indices is None else indices.data_ptr(), k, height, width, 1 if grayscale else 3,
                                 out.data_ptr()))


def pixels_strided(handle, out_ptr: int, height: int, width: int, grayscale: bool, copies: int, env_stride: int, copy_stride: int,
                   mask=None):
    """Every env i whose mask byte is set (all when `mask` is None; a uint8 device tensor [N]): its observation `copies` times at
    out_ptr + i * env_stride + c * copy_stride (bytes).  Stream-ordered on the handle's stream, no synchronisation."""
    handle._check(lib.mxv_pixels_strided(handle._h, None if mask is None else mask.data_ptr(), height, width, 1 if grayscale else 3,
                                         int(copies), out_ptr, int(env_stride), int(copy_stride)))
