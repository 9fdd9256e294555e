#!/usr/bin/env python3
"""Actor-critic with GAE(lambda) on Pendulum-v1 with a Gaussian policy whose sampling loop is one hipGraph replay per chunk: 4 096 envs x
64 steps per iteration.

examples/actor_critic_sampled.py for a Box action space.  The policy is a linear mean head, `mean = obs @ W`, with a state-independent
`log_std`.  Its actions come from `env.gaussian_sampler()` (gym_amd.policy): one launch per policy step that draws
`mean + exp(log_std) * z`, and also writes log pi(action) and the entropy of every row, so neither costs the loop a torch kernel.  The
K steps of a chunk are recorded once with `env.graphed_loop` and replayed.  The normals come from the engine's Philox streams — the
action of env G at policy step t depends on (seed, G, t) alone — so no torch generator is involved: two runs print identical histories,
on one GPU or sharded over several.

A graphed step does not write `final_obs`, so here a truncated episode bootstraps from 0 (the GAE example shows `final_values`).

    python examples/actor_critic_gaussian.py [--envs 4096] [--iterations 40]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def train(num_envs: int = 4096, iterations: int = 40, K: int = 64, lr: float = 0.05, value_lr: float = 0.01, gamma: float = 0.99,
          lam: float = 0.95, seed: int = 0, verbose: bool = True):
    import torch

    from gym_amd.rollout import DeviceRollout

    env = DeviceRollout("Pendulum-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.reset(seed=seed)
    sampler = env.gaussian_sampler()                # one action dim, the engine's env_offset and action_seed
    dev = env.device
    O = env.O
    W = torch.zeros((O, 1), device=dev)             # policy: a ~ N(obs @ W, exp(log_std)^2); static, updated in place
    log_std = torch.full((1,), -0.5, device=dev)    # state-independent, shared by all envs
    wv = torch.zeros(O + 1, device=dev)             # critic: V(obs) = obs @ wv[:O] + wv[O]
    f32 = dict(dtype=torch.float32, device=dev)
    traj = {"obs": torch.empty((K, num_envs, O), **f32), "actions": torch.empty((K, num_envs, 1), **f32),
            "reward": torch.empty((K, num_envs), dtype=env.reward_dtype, device=dev),
            "terminated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev),
            "truncated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev),
            "log_prob": torch.empty((K, num_envs), **f32), "entropy": torch.empty((K, num_envs), **f32)}
    step_out = (torch.empty((num_envs, 1), **f32), torch.empty(num_envs, **f32), torch.empty(num_envs, **f32))
    chosen_on = torch.empty((num_envs, O), **f32)

    def value(obs):
        return obs @ wv[:O] + wv[O]

    def policy(obs):
        chosen_on.copy_(obs)                                                      # the observation the action is chosen on
        return sampler.sample(obs @ W, log_std, out=step_out)[0]                  # actions, log pi and entropy: one launch

    def record(k):
        traj["obs"][k].copy_(chosen_on)
        traj["actions"][k].copy_(step_out[0])
        traj["log_prob"][k].copy_(step_out[1])
        traj["entropy"][k].copy_(step_out[2])
        traj["reward"][k].copy_(env.reward)
        traj["terminated"][k].copy_(env.terminated)
        traj["truncated"][k].copy_(env.truncated)

    graph = env.graphed_loop(policy, K, on_step=record)
    history = []
    with torch.cuda.stream(env.stream):
        for it in range(iterations):
            graph.replay()                                                        # K policy steps and K env steps, one host call
            values = value(traj["obs"])                                           # [K, N]
            adv, ret = env.advantages(traj, values, value(env.obs), gamma=gamma, lam=lam)
            norm = (adv - adv.mean()) / (adv.std() + 1e-8)
            # d log pi / d mean = (a - mean) / sigma^2,  d log pi / d log_std = ((a - mean) / sigma)^2 - 1
            row = {"iteration": it, "mean_reward": float(traj["reward"].mean()), "mean_log_prob": float(traj["log_prob"].mean()),
                   "mean_entropy": float(traj["entropy"].mean()), "log_std": float(log_std)}
            sigma = log_std.exp()
            zq = (traj["actions"].squeeze(-1) - (traj["obs"] @ W).squeeze(-1)) / sigma
            W.add_(lr * torch.einsum("kn,kni->i", norm * zq / sigma, traj["obs"]).unsqueeze(-1) / (K * num_envs))
            log_std.add_(lr * (norm * (zq * zq - 1.0)).mean()).clamp_(-2.0, 0.5)
            err = values - ret                                                    # critic: one gradient step on 1/2 (V - returns)^2
            wv[:O].sub_(value_lr * (err.unsqueeze(-1) * traj["obs"]).mean(dim=(0, 1)))
            wv[O].sub_(value_lr * err.mean())
            row["value_mse"] = float((err * err).mean())
            history.append(row)
            if verbose:
                print(f"iteration {it:3d}: mean reward {row['mean_reward']:8.4f}, log pi {row['mean_log_prob']:8.5f}, "
                      f"entropy {row['mean_entropy']:7.5f}, log_std {row['log_std']:7.4f}, critic mse {row['value_mse']:9.3f}")
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
    print(f"mean reward {h[0]['mean_reward']:.3f} -> {h[-1]['mean_reward']:.3f}")
