"""What the device-resident front ends share (DeviceRollout, TabularRollout, BlackjackRollout): the device check, the engine's
stream, the ordering calls and the allocation of trajectory tensors.  torch is imported when a rollout is constructed, not with this
module: gym_amd.toy_text stays importable without it."""
from __future__ import annotations

from . import _native


class _RolloutBase:
    # what synchronize() raises for an out-of-range action latched by a step: None lets the engine's MxvError through
    invalid_action_error = None

    def __init__(self, num_envs: int, device: int):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a HIP device (torch.cuda.is_available() is False); "
                               "gym_amd has no CPU fallback")
        self._torch = torch
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", device)
        self.last_placement = None      # the report of the last sorted / placed trajectory_buffers()

    def _adopt(self, handle, stream=None):
        """One torch-visible stream carries every launch of `handle`: the caller's (`stream`) or one of its own."""
        self.handle = handle
        self.stream = stream if stream is not None else self._torch.cuda.Stream(device=self.device)
        handle.set_stream(self.stream.cuda_stream)

    def _allocate(self, specs, layout: str, classes: dict, auto_bytes: int, sorted_min_bytes: int, budget_bytes=None):
        """The tensors of `specs` — (name, shape, dtype, zero-filled) each — as a dict.  layout="sorted": ordinary allocations sorted by HBM
        class (gym_amd/placement.py), `classes` naming the class of every write stream, the report left in self.last_placement;
        "separate": one torch allocation per tensor; "auto": sorted once `auto_bytes` reaches `sorted_min_bytes`."""
        t = self._torch
        if layout == "auto":
            from . import placement

            layout = "sorted" if auto_bytes >= sorted_min_bytes and placement.enabled() else "separate"   # MXV_PLACEMENT=off: never sort
        if layout == "sorted":
            from .placement import sorted_tensors

            out, self.last_placement = sorted_tensors(specs, classes, self.device, self.stream, budget_bytes)
            return out
        if layout != "separate":
            raise ValueError(f"layout must be 'auto', 'sorted' or 'separate', got {layout!r}")
        with t.cuda.stream(self.stream):
            return {name: (t.zeros if zero else t.empty)(shape, dtype=dt, device=self.device) for name, shape, dt, zero in specs}

    def ready(self):
        """GPU-side ordering of the outputs: the caller's current torch stream waits for everything launched so far on the
        engine's stream (no host synchronisation).  Use before touching output tensors outside `with torch.cuda.stream(r.stream)`."""
        self._torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def advantages(self, traj, values, last_value=None, *, gamma: float = 0.99, lam: float = 0.95, final_values=None, out=None):
        """GAE(lambda) over the chunk in `traj` (the dict of rollout_per_step / rollout_tape) -> (advantages, returns), float32 [K, N]:
        gym_amd.returns.gae on traj["reward"], traj["terminated"], traj["truncated"], launched on the caller's current stream after
        ready(), so that it waits for the rollout on the GPU.

        `values` [K, N]: the learner's V of the observation the action of step t was taken FROM.  That is NOT V(traj["obs"]):
        traj["obs"][t] is the observation AFTER step t, and after an autoreset the next episode's first one.  With `first_obs` the
        observation the chunk started from (reset()'s, or traj["obs"][K-1] of the previous chunk),
            values = V(gym_amd.returns.pre_step_observations(first_obs, traj["obs"]))    # cat(first_obs[None], traj["obs"][:-1])
            last_value = V(traj["obs"][K-1])                                             # [N]
        `final_values` [K, N]: V(traj["final_obs"]) (trajectory_buffers(want_final=True)), which a truncated step bootstraps from."""
        from .returns import gae

        self.ready()
        return gae(traj["reward"], traj["terminated"], traj["truncated"], values, last_value, gamma=gamma, lam=lam,
                   final_values=final_values, out=out)

    def vtrace(self, traj, values, log_prob, old_log_prob, last_value=None, *, gamma: float = 0.99, lam: float = 1.0, rho_bar: float = 1.0,
               c_bar: float = 1.0, pg_rho_bar=None, final_values=None, out=None):
        """V-trace targets of the chunk in `traj` -> (vs, pg_advantages), float32 [K, N]: gym_amd.vtrace.vtrace on traj["reward"],
        traj["terminated"], traj["truncated"] after ready().  For a chunk whose actions were drawn by older weights than the ones being
        updated: `old_log_prob` [K, N] is what the sampler recorded, `log_prob` [K, N] the learner's log pi of the stored actions
        (evaluate_categorical / evaluate_gaussian); `values`, `last_value` and `final_values` as in advantages()."""
        from .vtrace import vtrace

        self.ready()
        return vtrace(log_prob, old_log_prob, traj["reward"], traj["terminated"], traj["truncated"], values, last_value, gamma=gamma,
                      lam=lam, rho_bar=rho_bar, c_bar=c_bar, pg_rho_bar=pg_rho_bar, final_values=final_values, out=out)

    def returns_to_go(self, traj, *, gamma: float = 0.99, last_value=None, final_values=None, out=None):
        """Discounted returns-to-go of the chunk in `traj` -> float32 [K, N]: gym_amd.returns.discounted_returns after ready()."""
        from .returns import discounted_returns

        self.ready()
        return discounted_returns(traj["reward"], traj["terminated"], traj["truncated"], gamma=gamma, last_value=last_value,
                                  final_values=final_values, out=out)

    def policy_sampler(self, seed=None):
        """A gym_amd.policy.PolicySampler for this rollout's actions: its action count and dtype, its env_offset (so that shards of one
        logical vector env draw what the whole would), on its device; `seed` defaults to the rollout's action_seed.
        sampler.sample(logits)[0] is what step() takes (DeviceRollout), and with [None] in front the K = 1 tape of rollout_tape()."""
        from .policy import PolicySampler

        n, dtype = self._policy_head
        if n < 1:
            raise ValueError(f"{type(self).__name__}: policy_sampler() draws Discrete actions; this env takes Box actions: "
                             "use gaussian_sampler() for a Gaussian head (DESIGN.md §13)")
        return PolicySampler(n, seed=self.handle._action_seed if seed is None else seed, env_offset=self.env_offset, action_dtype=dtype,
                             device=self.device)

    def gaussian_sampler(self, seed=None):
        """A gym_amd.policy.GaussianSampler for this rollout's Box actions (one dim): its env_offset (so that shards of one logical vector
        env draw what the whole would), on its device; `seed` defaults to the rollout's action_seed.
        sampler.sample(mean, log_std)[0] is what step() takes."""
        from .policy import GaussianSampler

        n, _ = self._policy_head
        if n >= 1:
            raise ValueError(f"{type(self).__name__}: gaussian_sampler() draws Box actions; this env takes Discrete({n}) actions: "
                             "use policy_sampler()")
        return GaussianSampler(1, seed=self.handle._action_seed if seed is None else seed, env_offset=self.env_offset, device=self.device)

    def squashed_gaussian_sampler(self, seed=None):
        """A gym_amd.squashed.SquashedGaussianSampler for this rollout's Box actions (one dim): the bounds of the env's action space
        (Pendulum-v1 +-2, MountainCarContinuous-v0 +-1), its env_offset (so that shards of one logical vector env draw what the whole
        would), on its device; `seed` defaults to the rollout's action_seed.  sampler.sample(mean, log_std)[0] is what step() takes,
        sampler.rsample(mean, log_std) the differentiable draw of an off-policy update."""
        from .registration import single_spaces
        from .squashed import SquashedGaussianSampler

        n, _ = self._policy_head
        if n >= 1:
            raise ValueError(f"{type(self).__name__}: squashed_gaussian_sampler() draws Box actions; this env takes Discrete({n}) "
                             "actions: use policy_sampler()")
        box = single_spaces(self.spec.kind)[1]
        return SquashedGaussianSampler(int(box.shape[0]), low=box.low, high=box.high, seed=self.handle._action_seed if seed is None else seed,
                                       env_offset=self.env_offset, device=self.device)

    def replay_buffer(self, capacity, seed=None):
        """A gym_amd.replay.ReplayBuffer for this rollout's transitions: its observation shape and dtype, its action dtype, on its
        device; `seed` defaults to the rollout's action_seed.  buf.add_chunk(first_obs, traj) stores what rollout_per_step /
        rollout_tape leave in `traj`."""
        from .replay import ReplayBuffer

        layout = getattr(self, "_replay_obs", None)
        if layout is None:
            raise ValueError(f"{type(self).__name__}: replay_buffer() needs trajectories of [K, N, ...] observation rows; build a "
                             "gym_amd.ReplayBuffer with the shape and dtype of the rows you record")
        shape, dtype = layout
        return ReplayBuffer(capacity, shape, obs_dtype=dtype, action_dtype=self._policy_head[1],
                            seed=self.handle._action_seed if seed is None else seed, device=self.device)

    def prioritized_replay_buffer(self, capacity, alpha=0.6, eps=1e-6, seed=None):
        """A gym_amd.prioritized.PrioritizedReplayBuffer for this rollout's transitions: replay_buffer() with proportional draws, importance
        weights and update_priorities."""
        from .prioritized import PrioritizedReplayBuffer

        layout = getattr(self, "_replay_obs", None)
        if layout is None:
            raise ValueError(f"{type(self).__name__}: prioritized_replay_buffer() needs trajectories of [K, N, ...] observation rows; build a "
                             "gym_amd.PrioritizedReplayBuffer with the shape and dtype of the rows you record")
        shape, dtype = layout
        return PrioritizedReplayBuffer(capacity, shape, obs_dtype=dtype, action_dtype=self._policy_head[1],
                                       seed=self.handle._action_seed if seed is None else seed, device=self.device, alpha=alpha, eps=eps)

    def nstep_replay_buffer(self, capacity, n_step, gamma, prioritized=False, alpha=0.6, eps=1e-6, seed=None):
        """A gym_amd.nstep.NStepReplayBuffer — or, with prioritized=True, an NStepPrioritizedReplayBuffer with `alpha` and `eps` — for this
        rollout's transitions: replay_buffer() whose rows are n-step returns with a per-row discount."""
        from .nstep import NStepPrioritizedReplayBuffer, NStepReplayBuffer

        layout = getattr(self, "_replay_obs", None)
        if layout is None:
            raise ValueError(f"{type(self).__name__}: nstep_replay_buffer() needs trajectories of [K, N, ...] observation rows; build a "
                             "gym_amd.NStepReplayBuffer with the shape and dtype of the rows you record")
        shape, dtype = layout
        kw = dict(obs_dtype=dtype, action_dtype=self._policy_head[1], seed=self.handle._action_seed if seed is None else seed, device=self.device)
        if prioritized:
            return NStepPrioritizedReplayBuffer(capacity, shape, n_step, gamma, alpha=alpha, eps=eps, **kw)
        return NStepReplayBuffer(capacity, shape, n_step, gamma, **kw)

    def synchronize(self):
        """Wait for the engine's stream; raises if a step saw an out-of-range action."""
        try:
            self.handle.sync()
        except _native.MxvError as e:
            if e.code == _native.ERR_INVALID_ACTION and self.invalid_action_error is not None:
                raise self.invalid_action_error(e.message) from None
            raise

    def close(self):
        self.handle.close()
