#!/usr/bin/env python3
"""Actor-critic with GAE(lambda) on CartPole-v1, 4 096 envs x 64 steps per iteration, every tensor resident on the device.

A linear-logistic policy and a linear value head.  The chunk's tensors come from `trajectory_buffers(K, want_final=True)`: `final_obs`
holds the last observation of every episode that ended inside the chunk, so a TRUNCATED episode (CartPole-v1's 500-step limit) bootstraps
from the critic's value of the observation it was cut at — `final_values` — and a terminated one from 0; the observation after an
autoreset belongs to the next episode and is never anybody's bootstrap.  `env.advantages(traj, values, last_value, final_values=...)`
is one kernel launch (gym_amd.gae) ordered after the rollout on the GPU; the learner's own normalisation of the advantages
over the batch stays in torch.

    python examples/actor_critic_gae.py [--envs 4096] [--iterations 40]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def train(num_envs: int = 4096, iterations: int = 40, K: int = 64, lr: float = 5.0, value_lr: float = 0.1, gamma: float = 0.99,
          lam: float = 0.95, seed: int = 0, verbose: bool = True):
    import torch

    from gym_amd.rollout import DeviceRollout

    torch.manual_seed(seed)
    env = DeviceRollout("CartPole-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.enable_episode_stats()
    env.reset(seed=seed)
    dev = env.device
    w = torch.zeros(4, device=dev)                  # policy: P(action = 1) = sigmoid(obs @ w)
    wv = torch.zeros(5, device=dev)                 # critic: V(obs) = obs @ wv[:4] + wv[4]
    traj = env.trajectory_buffers(K, want_final=True, layout="separate")
    ep_len = torch.zeros((K, num_envs), device=dev)

    def value(obs):
        return obs @ wv[:4] + wv[4]

    history = []
    with torch.cuda.stream(env.stream):
        for it in range(iterations):
            for k in range(K):
                traj["obs"][k].copy_(env.obs)                                     # the observation the action is chosen on
                a = (torch.rand(num_envs, device=dev) < torch.sigmoid(env.obs @ w)).to(env.action_dtype)
                env.step(a, want_final=True)
                traj["actions"][k].copy_(a)
                traj["reward"][k].copy_(env.reward)
                traj["terminated"][k].copy_(env.terminated)
                traj["truncated"][k].copy_(env.truncated)
                traj["final_obs"][k].copy_(env.final_obs)                         # meaningful where the step ended an episode
                ep_len[k].copy_(env.ep_length * (env.terminated | env.truncated))
            values = value(traj["obs"])                                           # [K, N]
            final_values = value(traj["final_obs"])                               # read only where truncated and not terminated
            adv, ret = env.advantages(traj, values, value(env.obs), gamma=gamma, lam=lam, final_values=final_values)
            norm = (adv - adv.mean()) / (adv.std() + 1e-8)
            act = traj["actions"].to(torch.float32)
            p = torch.sigmoid(traj["obs"] @ w)
            w.add_(lr * ((norm * (act - p)).unsqueeze(-1) * traj["obs"]).mean(dim=(0, 1)))
            err = values - ret                                                    # critic: one gradient step on 1/2 (V - returns)^2
            wv[:4].sub_(value_lr * (err.unsqueeze(-1) * traj["obs"]).mean(dim=(0, 1)))
            wv[4].sub_(value_lr * err.mean())
            ended = (ep_len > 0).sum().clamp(min=1)
            row = {"iteration": it, "mean_episode_length": float(ep_len.sum() / ended), "episodes": int(ended),
                   "truncated": int(traj["truncated"].sum()), "value_mse": float((err * err).mean())}
            history.append(row)
            if verbose:
                print(f"iteration {it:3d}: {row['episodes']:6d} episodes ended ({row['truncated']} truncated), mean length "
                      f"{row['mean_episode_length']:7.1f}, critic mse {row['value_mse']:9.3f}")
    env.close()
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=40)
    a = ap.parse_args()
    h = train(a.envs, a.iterations)
    print(f"mean episode length {h[0]['mean_episode_length']:.1f} -> {h[-1]['mean_episode_length']:.1f}")
