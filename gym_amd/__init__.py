"""gym_amd — MI355X-native vectorised classic-control environment engine.

A drop-in for the `gym.vector.SyncVectorEnv` hot path of openai/gym 0.26.2 on CartPole-v0/v1,
Pendulum-v1, Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0: hand-written gfx950 HIP
kernels behind the C ABI of include/mxv.h, bound with ctypes (gym_amd._native) and wrapped by
`HipVectorEnv` (NumPy contract of the reference) and `DeviceRollout` (device-resident tensors).
There is no CPU fallback: without the built extension / without a HIP device the engine raises.
"""
__version__ = "0.6.0"

_LAZY = {
    "HipVectorEnv": ("gym_amd.vector_env", "HipVectorEnv"),
    "VectorEnv": ("gym_amd.vector_env", "VectorEnv"),
    "VectorEnvWrapper": ("gym_amd.vector_env", "VectorEnvWrapper"),
    "make": ("gym_amd.vector_env", "make"),
    "HipEnv": ("gym_amd.single_env", "HipEnv"),
    "DeviceRollout": ("gym_amd.rollout", "DeviceRollout"),
    "PixelRollout": ("gym_amd.pixels", "PixelRollout"),
    "pendulum_arrow_image": ("gym_amd.arrow", "pendulum_arrow_image"),
    "ShardedRollout": ("gym_amd.distributed", "ShardedRollout"),
    "MixedRollout": ("gym_amd.mixed", "MixedRollout"),
    "RecordEpisodeStatistics": ("gym_amd.wrappers", "RecordEpisodeStatistics"),
    "VectorListInfo": ("gym_amd.wrappers", "VectorListInfo"),
    "NormalizeObservation": ("gym_amd.wrappers", "NormalizeObservation"),
    "NormalizeReward": ("gym_amd.wrappers", "NormalizeReward"),
    "RunningNormalizer": ("gym_amd.normalize", "RunningNormalizer"),
    "HipTabularVectorEnv": ("gym_amd.toy_text", "HipTabularVectorEnv"),
    "TabularRollout": ("gym_amd.toy_text", "TabularRollout"),
    "HipBlackjackVectorEnv": ("gym_amd.toy_text", "HipBlackjackVectorEnv"),
    "BlackjackRollout": ("gym_amd.toy_text", "BlackjackRollout"),
    "gae": ("gym_amd.returns", "gae"),
    "discounted_returns": ("gym_amd.returns", "discounted_returns"),
    "sample_categorical": ("gym_amd.policy", "sample_categorical"),
    "PolicySampler": ("gym_amd.policy", "PolicySampler"),
    "sample_gaussian": ("gym_amd.policy", "sample_gaussian"),
    "GaussianSampler": ("gym_amd.policy", "GaussianSampler"),
    "evaluate_categorical": ("gym_amd.policy_eval", "evaluate_categorical"),
    "evaluate_gaussian": ("gym_amd.policy_eval", "evaluate_gaussian"),
    "advantage_moments": ("gym_amd.ppo", "advantage_moments"),
    "ppo_clip_loss": ("gym_amd.ppo", "ppo_clip_loss"),
    "dqn_loss": ("gym_amd.dqn", "dqn_loss"),
    "ReplayBuffer": ("gym_amd.replay", "ReplayBuffer"),
    "PrioritizedReplayBuffer": ("gym_amd.prioritized", "PrioritizedReplayBuffer"),
    "categorical_dqn_loss": ("gym_amd.c51", "categorical_dqn_loss"),
    "categorical_q_values": ("gym_amd.c51", "categorical_q_values"),
    "rsample_squashed_gaussian": ("gym_amd.squashed", "rsample_squashed_gaussian"),
    "SquashedGaussianSampler": ("gym_amd.squashed", "SquashedGaussianSampler"),
    "NStepReplayBuffer": ("gym_amd.nstep", "NStepReplayBuffer"),
    "NStepPrioritizedReplayBuffer": ("gym_amd.nstep", "NStepPrioritizedReplayBuffer"),
    "quantile_dqn_loss": ("gym_amd.qr", "quantile_dqn_loss"),
    "quantile_q_values": ("gym_amd.qr", "quantile_q_values"),
    "dqn_targets": ("gym_amd.targets", "dqn_targets"),
    "categorical_targets": ("gym_amd.targets", "categorical_targets"),
    "quantile_targets": ("gym_amd.targets", "quantile_targets"),
    "soft_q_targets": ("gym_amd.sac", "soft_q_targets"),
    "twin_q_loss": ("gym_amd.sac", "twin_q_loss"),
    "soft_policy_loss": ("gym_amd.sac", "soft_policy_loss"),
}

def __getattr__(name):
    if name in ("vector", "wrappers", "spaces", "error", "plugin", "toy_text"):  # sub-modules, gym-shaped
        import importlib

        return importlib.import_module(f"gym_amd.{name}")
    if name == "vtrace":
        # the function shares its sub-module's name, and importing a sub-module binds it as the package's attribute: the module is
        # callable (gym_amd/vtrace.py), so gym_amd.vtrace(...) is the function before and after that import
        import importlib

        return importlib.import_module("gym_amd.vtrace")
    if name in _LAZY:
        import importlib

        mod, attr = _LAZY[name]
        return getattr(importlib.import_module(mod), attr)
    raise AttributeError(f"module 'gym_amd' has no attribute {name!r}")
