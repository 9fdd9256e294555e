"""PixelRollout — device-resident pixel observations with frame stacks.

The reference's pixel pipeline on one env is PixelObservationWrapper -> GrayScaleObservation -> ResizeObservation -> FrameStack
(pixel_observation.py:165-190, gray_scale_observation.py:50-64, resize_observation.py:48-70, frame_stack.py:164-189), under a
SyncVectorEnv that autoresets (sync_vector_env.py:150-156).  Here every step is a handful of launches on one stream, with no host
synchronisation: the dynamics of a DeviceRollout(autoreset=False); the frame of every stepped state reduced on the device
(mxv_pixels_strided) into the newest slot of its env's stack; the stacks of finished envs copied into `final_pixels` (their newest
slot is the TERMINAL frame, which the autoreset engine would already have overwritten); a masked reset of the finished envs, whose
reset stream is keyed by each env's reset ordinal (include/mxv.h RNG contract), so states, rewards and flags are those of the
autoreset engine; and the stacks of those envs refilled with their reset frame.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _native, _render
from .registration import spec as _spec
from .rollout import DeviceRollout
from .spaces import Box, batch_space

TOY_TEXT_REASON = ("{id} has no pixel observations on the device engine: the toy_text engines keep tabular states only, and their "
                   "frames (pygame sprite sheets) are not drawn by it")


class PixelRollout:
    """`num_envs` envs of a classic-control `id` whose observations are stacks of `stack` reduced frames, oldest first:
    uint8 [N, stack, height, width] (gray) or [N, stack, height, width, 3].  `reset()` / `step()` return device tensors ordered on
    `self.stream` (see DeviceRollout: `ready()`, `synchronize()`).  The engine's own tensors stay reachable: `obs`, `final_obs`,
    `reward`, `terminated`, `truncated`, and `actions` (the actions of the last sampled step)."""

    def __init__(self, id: str, num_envs: int, *, height: int = 84, width: int = 84, grayscale: bool = True, stack: int = 4,
                 seed: int = 0, action_seed: int = 0, max_episode_steps: Optional[int] = None, device: int = 0,
                 stream: Optional["torch.cuda.Stream"] = None, arrow_image=None):
        from .toy_text import TOY_TEXT_REGISTRY

        if id in TOY_TEXT_REGISTRY or id.startswith("Blackjack"):
            raise NotImplementedError(TOY_TEXT_REASON.format(id=id))
        kind = _spec(id).kind
        # Pendulum-v1: frames only with the caller's arrow image (pendulum.py:228-244); any other id refuses the keyword
        arrow_image = _render.arrow_kwarg(kind, id, arrow_image)
        if kind == _native.PENDULUM and arrow_image is None:
            raise NotImplementedError(_render.PENDULUM_REASON)
        self.frame_shape = _render.pixel_shape(kind, height, width, grayscale, (500, 500) if kind == _native.PENDULUM else None)
        if not isinstance(stack, int) or stack < 1:
            raise ValueError(f"stack must be a positive int, got {stack!r}")
        self.height, self.width, self.grayscale, self.stack = height, width, bool(grayscale), stack
        self.engine = DeviceRollout(id, num_envs, device=device, seed=seed, action_seed=action_seed,
                                    max_episode_steps=max_episode_steps, autoreset=False, stream=stream, arrow_image=arrow_image)
        self.spec, self.num_envs, self.device, self.stream = self.engine.spec, self.engine.num_envs, self.engine.device, self.engine.stream
        self.single_observation_space = Box(0, 255, shape=(stack,) + self.frame_shape, dtype=np.uint8)
        self.observation_space = batch_space(self.single_observation_space, self.num_envs)
        n = self.num_envs
        self._frame_bytes = math.prod(self.frame_shape)
        self._env_stride = stack * self._frame_bytes
        with torch.cuda.stream(self.stream):
            # two stacks, used in turn: a step shifts the current one into the other (one copy, no overlapping source and target)
            self._stacks = [torch.zeros((n, stack) + self.frame_shape, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.final_pixels = torch.zeros((n, stack) + self.frame_shape, dtype=torch.uint8, device=self.device)
            self._done = torch.zeros(n, dtype=torch.bool, device=self.device)
        self._cur = 0
        self.stream.synchronize()

    # -- the engine's tensors ----------------------------------------------------------------------------------------------------------
    @property
    def obs(self):
        return self.engine.obs

    @property
    def final_obs(self):
        return self.engine.final_obs

    @property
    def reward(self):
        return self.engine.reward

    @property
    def terminated(self):
        return self.engine.terminated

    @property
    def truncated(self):
        return self.engine.truncated

    @property
    def actions(self):
        return self.engine.actions

    @property
    def pixels(self) -> torch.Tensor:
        """The current stacks (what the last reset() / step() returned)."""
        return self._stacks[self._cur]

    def _push(self, stacks: torch.Tensor, copies: int, mask: Optional[torch.Tensor]):
        """Reduced frames of the current states into `copies` slots of each (masked) env's stack, from the last slot - copies + 1 on."""
        ptr = stacks.data_ptr() + (self.stack - copies) * self._frame_bytes
        _render.pixels_strided(self.engine.handle, ptr, self.height, self.width, self.grayscale, copies, self._env_stride,
                               self._frame_bytes, mask)

    def reset(self, seed: Optional[int] = None) -> torch.Tensor:
        """Resets every env (reseeding first when `seed` is given) and fills every slot of its stack with the reset frame."""
        self.engine.reset(seed)
        self._push(self.pixels, self.stack, None)
        self.ready()
        return self.pixels

    def step(self, actions: Optional[torch.Tensor] = None):
        """One vector step: (pixels, reward, terminated, truncated).  `actions`: a device tensor of the engine's action dtype, or None
        for actions sampled on the device (DeviceRollout.step_sampled; they are left in `self.actions`).  In order: the dynamics; the
        frame of every stepped state (the terminal one for finished envs) becomes the newest slot; the stacks of finished envs go to
        `final_pixels` and their observations to `final_obs` (other rows untouched); finished envs are reset and their stacks filled
        with the reset frame.  `pixels` is the other of two stack buffers every step: valid until the step after next."""
        e = self.engine
        if actions is None:
            e.step_sampled(want_final=False)
        else:
            e.step(actions, want_final=False)
        cur, new = self._stacks[self._cur], self._stacks[1 - self._cur]
        n = self.num_envs
        with torch.cuda.stream(self.stream):
            if self.stack > 1:
                new[:, :-1].copy_(cur[:, 1:])
            self._push(new, 1, None)
            done = torch.logical_or(e.terminated, e.truncated, out=self._done)
            torch.where(done.view((n,) + (1,) * (new.dim() - 1)), new, self.final_pixels, out=self.final_pixels)
            torch.where(done.view(n, 1), e.obs, e.final_obs, out=e.final_obs)
            mask = done.view(torch.uint8)
            e.handle.reset(e.obs, mask_dev=mask)
            self._push(new, self.stack, mask)
        self._cur ^= 1
        return new, e.reward, e.terminated, e.truncated

    def ready(self):
        """The caller's current stream waits (on the GPU) for everything launched so far on the engine's stream."""
        self.engine.ready()

    def synchronize(self):
        """Host wait for the engine's stream; raises on an error a launch latched."""
        self.engine.synchronize()

    def state_dict(self) -> dict:
        """The engine's snapshot plus the current stacks and the final stacks / observations (NumPy, picklable): load_state_dict()
        continues bit-identically, rows of `final_pixels` / `final_obs` that no later step rewrites included."""
        snap = self.engine.state_dict()
        return {"engine": snap, "pixels": self.pixels.cpu().numpy(), "final_pixels": self.final_pixels.cpu().numpy(),
                "final_obs": self.final_obs.cpu().numpy(), "layout": (self.height, self.width, self.grayscale, self.stack)}

    def load_state_dict(self, snap: dict):
        if tuple(snap["layout"]) != (self.height, self.width, self.grayscale, self.stack):
            raise ValueError(f"snapshot of (height, width, grayscale, stack) = {tuple(snap['layout'])}, this rollout has "
                             f"{(self.height, self.width, self.grayscale, self.stack)}")
        self.engine.load_state_dict(snap["engine"])
        with torch.cuda.stream(self.stream):
            for dst, key in ((self.pixels, "pixels"), (self.final_pixels, "final_pixels"), (self.final_obs, "final_obs")):
                dst.copy_(torch.from_numpy(np.ascontiguousarray(snap[key])).to(self.device))
        self.stream.synchronize()

    def close(self):
        self.engine.close()
