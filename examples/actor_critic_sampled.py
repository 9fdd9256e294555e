#!/usr/bin/env python3
"""Actor-critic with GAE(lambda) on CartPole-v1 whose sampling loop is one hipGraph replay per chunk: 4 096 envs x 64 steps per iteration.

examples/actor_critic_gae.py with three changes.  The policy is a two-logit softmax head, `logits = obs @ W`.  Its actions come from
`env.policy_sampler()` (gym_amd.policy): one launch per policy step that also writes log pi(action) and the entropy of
every row, so neither costs the loop a torch kernel.  And the K steps of a chunk are recorded once with `env.graphed_loop` and replayed.
The sampler draws from the engine's Philox streams — the action of env G at policy step t depends on (seed, G, t) alone — so no torch
generator is involved: two runs print identical histories, on one GPU or sharded over several.

A graphed step does not write `final_obs`, so here a truncated episode bootstraps from 0 like a terminated one (the GAE example shows
`final_values`).

    python examples/actor_critic_sampled.py [--envs 4096] [--iterations 40]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def train(num_envs: int = 4096, iterations: int = 40, K: int = 64, lr: float = 5.0, value_lr: float = 0.1, gamma: float = 0.99,
          lam: float = 0.95, seed: int = 0, verbose: bool = True):
    import torch

    from gym_amd.rollout import DeviceRollout

    env = DeviceRollout("CartPole-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.enable_episode_stats()
    env.reset(seed=seed)
    sampler = env.policy_sampler()                  # Discrete(2), the engine's action dtype, env_offset and action_seed
    dev = env.device
    W = torch.zeros((4, 2), device=dev)             # policy: pi(. | obs) = softmax(obs @ W); static, updated in place
    wv = torch.zeros(5, device=dev)                 # critic: V(obs) = obs @ wv[:4] + wv[4]
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
        return obs @ wv[:4] + wv[4]

    def policy(obs):
        chosen_on.copy_(obs)                                                      # the observation the action is chosen on
        return sampler.sample(obs @ W, out=step_out)[0]                           # actions, log pi and entropy: one launch

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
            values = value(traj["obs"])                                           # [K, N]
            adv, ret = env.advantages(traj, values, value(env.obs), gamma=gamma, lam=lam)
            norm = (adv - adv.mean()) / (adv.std() + 1e-8)
            # d log pi(a) / d logits = onehot(a) - softmax = onehot(a) - exp(log-probabilities of both actions)
            p = torch.softmax(traj["obs"] @ W, dim=-1)
            onehot = torch.nn.functional.one_hot(traj["actions"].long(), 2).to(torch.float32)
            W.add_(lr * torch.einsum("kn,knj,kni->ij", norm, onehot - p, traj["obs"]) / (K * num_envs))
            err = values - ret                                                    # critic: one gradient step on 1/2 (V - returns)^2
            wv[:4].sub_(value_lr * (err.unsqueeze(-1) * traj["obs"]).mean(dim=(0, 1)))
            wv[4].sub_(value_lr * err.mean())
            ended = (ep_len > 0).sum().clamp(min=1)
            row = {"iteration": it, "mean_episode_length": float(ep_len.sum() / ended), "episodes": int(ended),
                   "mean_log_prob": float(traj["log_prob"].mean()), "mean_entropy": float(traj["entropy"].mean()),
                   "value_mse": float((err * err).mean())}
            history.append(row)
            if verbose:
                print(f"iteration {it:3d}: {row['episodes']:6d} episodes ended, mean length {row['mean_episode_length']:7.1f}, "
                      f"log pi {row['mean_log_prob']:8.5f}, entropy {row['mean_entropy']:7.5f}, critic mse {row['value_mse']:9.3f}")
    policy_steps = sampler.step_index()
    env.close()
    if verbose:
        print(f"{policy_steps} policy steps drawn")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=40)
    a = ap.parse_args()
    h = train(a.envs, a.iterations)
    print(f"mean episode length {h[0]['mean_episode_length']:.1f} -> {h[-1]['mean_episode_length']:.1f}")
