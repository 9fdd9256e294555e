#!/usr/bin/env python3
"""PPO with the clipped surrogate on CartPole-v1, the update fused: examples/ppo_clip.py with its torch sequence of the loss replaced by
`gym_amd.advantage_moments` and `gym_amd.ppo_clip_loss`.

Everything up to the advantages is that example's: the sampler, the graphed chunk of K steps, `env.advantages`.  An update is then
head -> `gym_amd.evaluate_categorical` -> `gym_amd.ppo_clip_loss` -> `backward()`: three launches of this engine forwards and two
backwards, where the torch sequence (normalisation, exp, clamp, two products, minimum, three means, the scalar arithmetic) took about
twenty each way.  The diagnostics — policy and value loss, entropy, both KL estimates, the clipped fraction and the extreme ratios — are
one device vector written by the forward; it is read once per epoch, where the torch example synchronised five times.

The loss is a fixed tree of float64 additions, so it is a function of the batch and of nothing else; and the evaluation follows the
sampler's arithmetic bit for bit, so in the first epoch of every iteration the ratio is exactly 1.0 on every row, both KL estimates are
exactly 0 and nothing is clipped.

    python examples/ppo_clip_fused.py [--envs 4096] [--iterations 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def linear(obs, W):
    """obs [..., 4] times W [4, J] -> [..., J], in one fixed order of float32 operations whatever the leading shape."""
    return ((obs[..., 0:1] * W[0] + obs[..., 1:2] * W[1]) + obs[..., 2:3] * W[2]) + obs[..., 3:4] * W[3]


def train(num_envs: int = 4096, iterations: int = 20, K: int = 64, epochs: int = 4, lr: float = 0.02, clip: float = 0.2,
          value_coef: float = 0.5, entropy_coef: float = 0.01, gamma: float = 0.99, lam: float = 0.95, seed: int = 0, verbose: bool = True):
    import torch

    import gym_amd
    from gym_amd.ppo import STAT_NAMES
    from gym_amd.rollout import DeviceRollout

    env = DeviceRollout("CartPole-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.enable_episode_stats()
    env.reset(seed=seed)
    sampler = env.policy_sampler()                  # Discrete(2), the engine's action dtype, env_offset and action_seed
    dev = env.device
    W = torch.zeros((4, 2), device=dev, requires_grad=True)        # policy: pi(. | obs) = softmax(linear(obs, W))
    wv = torch.zeros((4, 1), device=dev, requires_grad=True)       # critic: V(obs) = linear(obs, wv) + bv
    bv = torch.zeros(1, device=dev, requires_grad=True)
    optimizer = torch.optim.Adam([W, wv, bv], lr=lr)
    f32 = dict(dtype=torch.float32, device=dev)
    traj = {"obs": torch.empty((K, num_envs, 4), **f32), "actions": torch.empty((K, num_envs), dtype=env.action_dtype, device=dev),
            "reward": torch.empty((K, num_envs), dtype=env.reward_dtype, device=dev),
            "terminated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev),
            "truncated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev),
            "log_prob": torch.empty((K, num_envs), **f32), "entropy": torch.empty((K, num_envs), **f32)}
    ep_len = torch.zeros((K, num_envs), **f32)
    step_out = (torch.empty(num_envs, dtype=env.action_dtype, device=dev), torch.empty(num_envs, **f32), torch.empty(num_envs, **f32))
    chosen_on = torch.empty((num_envs, 4), **f32)

    def value(obs):
        return linear(obs, wv).squeeze(-1) + bv

    def policy(obs):
        chosen_on.copy_(obs)                                                      # the observation the action is chosen on
        with torch.no_grad():
            return sampler.sample(linear(obs, W), out=step_out)[0]                # actions, log pi and entropy: one launch

    def record(k):
        traj["obs"][k].copy_(chosen_on)
        traj["actions"][k].copy_(step_out[0])
        traj["log_prob"][k].copy_(step_out[1])
        traj["entropy"][k].copy_(step_out[2])
        traj["reward"][k].copy_(env.reward)
        traj["terminated"][k].copy_(env.terminated)
        traj["truncated"][k].copy_(env.truncated)
        ep_len[k].copy_(env.ep_length * (env.terminated | env.truncated))

    graph = env.graphed_loop(policy, K, on_step=record)
    history = []
    with torch.cuda.stream(env.stream):
        for it in range(iterations):
            graph.replay()                                                        # K policy steps and K env steps, one host call
            with torch.no_grad():
                adv, ret = env.advantages(traj, value(traj["obs"]), value(env.obs), gamma=gamma, lam=lam)
                moments = gym_amd.advantage_moments(adv)                          # (mean, 1 / (std + 1e-8)) stays on the device
            old_log_prob = traj["log_prob"]
            stats = []
            for _ in range(epochs):
                # the stored actions under the current head: one launch; the loss and its diagnostics: two more
                log_prob, entropy = gym_amd.evaluate_categorical(linear(traj["obs"], W), traj["actions"])
                loss, diag = gym_amd.ppo_clip_loss(log_prob, old_log_prob, adv, clip=clip, moments=moments, entropy=entropy,
                                                   entropy_coef=entropy_coef, values=value(traj["obs"]), returns=ret, value_coef=value_coef)
                optimizer.zero_grad(set_to_none=True)
                loss.backward()
                optimizer.step()
                e = dict(zip(STAT_NAMES, diag.tolist()))                          # the one read of the epoch; the loss from its parts
                e.update(loss=e["policy_loss"] + value_coef * e["value_loss"] - entropy_coef * e["entropy"], clipped=e["clip_fraction"])
                stats.append(e)
            ended = (ep_len > 0).sum().clamp(min=1)
            row = {"iteration": it, "mean_episode_length": float(ep_len.sum() / ended), "episodes": int(ended),
                   "mean_entropy": float(traj["entropy"].mean()), "epochs": stats}
            history.append(row)
            if verbose:
                first, last = stats[0], stats[-1]
                print(f"iteration {it:3d}: {row['episodes']:6d} episodes ended, mean length {row['mean_episode_length']:7.1f}, "
                      f"entropy {row['mean_entropy']:7.5f}, first epoch ratio [{first['ratio_min']:.9f}, {first['ratio_max']:.9f}] "
                      f"kl {first['approx_kl']:.3e}, last epoch loss {last['loss']:9.5f} kl {last['approx_kl']:.3e} clipped {last['clipped']:.3f}")
    policy_steps = sampler.step_index()
    env.close()
    if verbose:
        print(f"{policy_steps} policy steps drawn")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=20)
    a = ap.parse_args()
    h = train(a.envs, a.iterations)
    print(f"mean episode length {h[0]['mean_episode_length']:.1f} -> {h[-1]['mean_episode_length']:.1f}")
