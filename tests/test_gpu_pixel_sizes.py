"""mxv_pixels / mxv_pixels_strided at every output height and at every alignment class of the output row (-m gpu).

tests/test_gpu_pixels.py holds the reduction to tests/pixels_host.py at six sizes; the launch shape of pixels_kernel (rows per band,
chunks per band, 16-byte or byte stores, the partial last band) changes with (h, w, channels) far more often than that.  Here every
height 1..H is run at widths that reach every gcd class of w * channels with 16, both sides of the LDS stage cap and the extremes, for
CartPole (400 x 600), Acrobot (500 x 500) and Pendulum with its arrow (500 x 500, the blit path), gray and RGB.

The reference is exact integer arithmetic on the device's own full frames: one int64 summed-area table per frame and channel (after
the integer gray weights), four lookups per output pixel at the corners of the windows [floor(i H / h), ceil((i + 1) H / h)) x
[floor(j W / w), ceil((j + 1) W / w)), rounded (sum + n // 2) // n.  It is itself held to tests/pixels_host.py at three sizes per case
before it judges anything.  It knows nothing of bands, tiles or chunks.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pendulum_render_host as prh  # noqa: E402
import pixels_host as ph  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
SENTINEL = 0xA7
GUARD = 64
DIMS = {"CartPole": (400, 600), "Acrobot": (500, 500), "Pendulum": (500, 500)}
CASES = [(kind, ch) for kind in DIMS for ch in (1, 3)]
SAT_CHECK_SIZES = [(84, 84), (7, 13)]          # and (H - 1, W - 1)


def widths(W):
    """w * C reaches every gcd class with 16 for C = 1 and 3 (1, 2, 4, 8, 16); 301 / 449 / 451 / W - 1 / W lie on both sides of the
    7 200-byte stage at four rows, three rows (RGB) and one row per band; 84 and 150 are the sizes learners use."""
    return sorted({1, 2, 3, 4, 8, 13, 16, 84, 150, 301, 449, 451, W - 1, W})


def _states(kind):
    """3-4 envs per kind: a reset state, extreme poses, and (CartPole) a cart off the screen, whose frame is the track line alone."""
    if kind == "Pendulum":
        g = np.load(os.path.join(GOLDEN, "render_pendulum.npz"))
        u = g["last_u"]
        pick = [int(np.flatnonzero(np.isnan(u))[0]),                 # no arrow
                int(np.nanargmax(u)), int(np.nanargmin(u)),          # the largest arrows, both flips
                int(np.nanargmin(np.where(np.abs(u) > 0.05, np.abs(u), np.nan)))]   # a small one
        return g["states"][pick], None, u[pick]
    g = np.load(os.path.join(GOLDEN, "render_scenes.npz"))
    st, pr = g[f"{kind}_states"], g[f"{kind}_params"]
    same = np.flatnonzero((pr == pr[0]).all(1))                      # the default attributes (one common parameter vector)
    st = st[same]
    if kind == "CartPole":
        far = np.array([[40.0, 0.0, 0.1, 0.0]])                      # cartx = 5 300 px: cart, pole and axle are clipped away
        return np.concatenate([st[[0, int(np.argmax(np.abs(st[:, 2]))), int(np.argmax(np.abs(st[:, 0])))]], far]), pr[0], None
    up = int(np.argmin(np.abs(np.abs(st[:, 0]) - np.pi)))            # first link up: the rows above the pivot are crowded
    return st[[0, up, int(np.argmax(np.abs(st[:, 1]))), int(np.argmax(np.abs(st[:, 0])))]], pr[0], None


class SatReference:
    """uint8 frames [k, H, W, 3] -> the pixel observation of any size, uint8 [k, h, w, C] on `device`, from one int64 summed-area table
    per frame and channel: four lookups per output pixel, (sum + n // 2) // n."""

    def __init__(self, frames, channels, device):
        import torch

        self.dev = device
        k, self.H, self.W, _ = frames.shape
        f = torch.from_numpy(frames).to(device).to(torch.int64)
        if channels == 1:
            r, g, b = ph.GRAY_WEIGHTS
            f = ((r * f[..., 0] + g * f[..., 1] + b * f[..., 2] + 8192) >> 14)[:, None]
        else:
            f = f.permute(0, 3, 1, 2)
        self.sat = torch.zeros((k, channels, self.H + 1, self.W + 1), dtype=torch.int64, device=device)
        self.sat[:, :, 1:, 1:] = f.cumsum(2).cumsum(3)
        self._rows, self._cols = {}, {}

    def _window(self, src, dst):
        import torch

        i = torch.arange(dst, dtype=torch.int64, device=self.dev)
        return torch.div(i * src, dst, rounding_mode="floor"), torch.div((i + 1) * src + dst - 1, dst, rounding_mode="floor")

    def __call__(self, h, w):
        import torch

        if w not in self._cols:                                      # column differences of the table, once per width
            c0, c1 = self._window(self.W, w)
            self._cols[w] = (self.sat[..., c1] - self.sat[..., c0], c1 - c0)
        if h not in self._rows:
            self._rows[h] = self._window(self.H, h)
        cols, cw = self._cols[w]
        r0, r1 = self._rows[h]
        s = cols[:, :, r1] - cols[:, :, r0]
        n = (r1 - r0)[:, None] * cw[None, :]
        return torch.div(s + torch.div(n, 2, rounding_mode="floor"), n, rounding_mode="floor").to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class Case:
    """One handle of a kind on its own torch stream, its full frames, and the summed-area-table reference for one channel count."""

    def __init__(self, kind, channels):
        import torch

        from gym_amd import _native, _render
        from gym_amd.registration import spec

        self.kind, self.C = kind, channels
        self.H, self.W = DIMS[kind]
        states, params, last_u = _states(kind)
        self.k = k = len(states)
        self.dev = torch.device("cuda", 0)
        if kind == "Pendulum":
            self.handle = h = _native.Handle(_native.PENDULUM, k, 200, device=0, seed=11, action_seed=12)
            _render.attach_image(h, prh.arrow())
        else:
            self.handle = h = _native.Handle(spec(f"{kind}-v1").kind, k, 500, device=0, seed=1, action_seed=2)
        h.reset_host()
        h.set_state(np.ascontiguousarray(np.asarray(states, np.float64).T), np.zeros(k, np.int32))
        if params is not None:
            h.set_params(np.asarray(params, np.float64))
        if last_u is not None:
            _render.set_torques(h, np.asarray(last_u, np.float32))
        self.frames = _render.render_host(h)                         # uint8 [k, H, W, 3], once
        assert self.frames.shape == (k, self.H, self.W, 3)
        self.stream = torch.cuda.Stream(device=self.dev)             # the launches and the reference share one stream: no host waits
        h.set_stream(self.stream.cuda_stream)
        with torch.cuda.stream(self.stream):
            self.table = SatReference(self.frames, channels, self.dev)
            for hh, ww in SAT_CHECK_SIZES + [(self.H - 1, self.W - 1)]:     # the table is not a second unverified rule
                want = ph.reduce(self.frames, hh, ww, channels == 1)
                assert np.array_equal(self.table(hh, ww).cpu().numpy().reshape(want.shape), want), (kind, channels, hh, ww)

    def reference(self, h, w):
        return self.table(h, w)

    def close(self):
        self.handle.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(kind, channels):
        if (kind, channels) not in made:
            made[kind, channels] = Case(kind, channels)
        return made[kind, channels]

    yield get
    for c in made.values():
        c.close()


def _first_difference(got, want, shape):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    bad = np.flatnonzero(g != w)
    at = [tuple(int(v) for v in np.unravel_index(b, shape)) for b in bad[:4]]
    return {"differing bytes": int(bad.size), "first (env, row, col, channel)": at, "got": g[bad[:4]].tolist(), "want": w[bad[:4]].tolist()}


@pytest.mark.parametrize("kind,channels", CASES)
def test_every_height_at_the_width_classes(cases, kind, channels):
    """One mxv_pixels launch per (h, w), h = 1..H, w in widths(W), into a sentinel-filled buffer: the observation equals the
    summed-area-table reference byte for byte and the 64 bytes on either side of it keep the sentinel."""
    import torch

    from gym_amd import _render

    c = cases(kind, channels)
    H, W, k = c.H, c.W, c.k
    guard = torch.full((GUARD,), SENTINEL, dtype=torch.uint8, device=c.dev)
    launches = 0
    with torch.cuda.stream(c.stream):
        buf = torch.empty(GUARD + k * H * W * channels + GUARD, dtype=torch.uint8, device=c.dev)
        assert buf.data_ptr() % 16 == 0
        for w in widths(W):
            for h in range(1, H + 1):
                nb = k * h * w * channels
                span = buf[:GUARD + nb + GUARD]
                span.fill_(SENTINEL)
                _render.pixels_device(c.handle, span[GUARD:], h, w, channels == 1, None, k)
                want = c.reference(h, w)
                launches += 1
                if torch.equal(span, torch.cat([guard, want.reshape(-1), guard])):
                    continue
                assert torch.equal(span[:GUARD], guard) and torch.equal(span[GUARD + nb:], guard), (kind, channels, h, w, "guard bytes written")
                pytest.fail(f"{kind} C={channels} h={h} w={w}: {_first_difference(span[GUARD:GUARD + nb], want.reshape(-1), (k, h, w, channels))}")
            c.handle.sync()                                          # no latched error
    assert launches == H * len(widths(W))


def _strided_sizes(H, W, count=40):
    """About 40 (h, w) of the sweep, fixed seed: one width per gcd class of w * C with 16 (w = 1, 2, 4, 8, 16 for C = 1 and 3 alike),
    heights below H / 48 and H / 16 (several source tiles per output row for gray and for RGB), the whole frame, then random draws."""
    rng = np.random.default_rng(20)
    forced = [(1, 1), (3, 2), (7, 4), (5, 8), (2, 16), (6, 13), (H, W), (H - 1, W - 1), (20, 84), (84, 84)]
    ws = widths(W)
    seen = list(dict.fromkeys(forced))
    while len(seen) < count:
        hw = (int(rng.integers(1, H + 1)), int(ws[rng.integers(len(ws))]))
        if hw not in seen:
            seen.append(hw)
    return seen


@pytest.mark.parametrize("channels", [1, 3])
def test_strided_masked_copies_at_the_alignment_classes(cases, channels):
    """mxv_pixels_strided as PixelRollout calls it, at 40 sizes: copies 1 and 3, a mask, a base pointer at an odd address, an env_stride
    that is no multiple of 16 (env 3 alone starts 16-byte aligned, so both store paths run), a copy_stride larger than the frame.
    Every copy of every masked env holds the reference; every other byte of the buffer keeps the sentinel."""
    import torch

    from gym_amd import _render

    c = cases("CartPole", channels)
    H, W, k = c.H, c.W, c.k
    rng = np.random.default_rng(21)
    with torch.cuda.stream(c.stream):
        for h, w in _strided_sizes(H, W):
            F = h * w * channels
            want = c.reference(h, w).reshape(k, 1, F)
            for copies in (1, 3):
                m = rng.random(k) < 0.5
                m[3], m[0] = True, False
                mask = torch.tensor(m.astype(np.uint8), device=c.dev)
                copy_stride = F + 5
                env_stride = copies * copy_stride + 7
                env_stride += (5 - env_stride) % 16                  # = 5 mod 16: base offset 1 + 3 * env_stride = 0 mod 16
                assert env_stride % 16 == 5 and env_stride >= copies * copy_stride
                total = 1 + k * env_stride + GUARD
                buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=c.dev)
                exp = torch.full((total,), SENTINEL, dtype=torch.uint8, device=c.dev)
                assert buf.data_ptr() % 16 == 0
                view = torch.as_strided(exp, (k, copies, F), (env_stride, copy_stride, 1), 1)
                view[mask.bool()] = want[mask.bool()].expand(-1, copies, -1)
                _render.pixels_strided(c.handle, buf.data_ptr() + 1, h, w, channels == 1, copies, env_stride, copy_stride, mask)
                if not torch.equal(buf, exp):
                    bad = np.flatnonzero(buf.cpu().numpy() != exp.cpu().numpy())
                    off = bad[:4] - 1
                    pytest.fail(f"C={channels} h={h} w={w} copies={copies} mask={m.astype(int).tolist()}: {bad.size} bytes differ, first at "
                                f"(env, byte in env) {[(int(o // env_stride), int(o % env_stride)) for o in off]}")
        c.handle.sync()
