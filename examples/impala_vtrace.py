#!/usr/bin/env python3
"""IMPALA-style actor-critic with V-trace on CartPole-v1: the learner of examples/ppo_clip.py with rollouts ONE UPDATE BEHIND the
weights — chunk i + 1 is drawn by the weights the learner held before its update on chunk i, the way an actor that rolls out while the
learner updates would draw it.

The behaviour log-probabilities `old_log_prob` are what the sampler recorded (`env.policy_sampler()`, one launch per policy step); the
learner's `log_prob` of the stored actions under its CURRENT head comes from `gym_amd.evaluate_categorical(...)`, detached for the
targets; the value targets `vs` and the policy-gradient advantages come from `env.vtrace(...)`: one launch, truncated
importance weights min(rho_bar, pi / mu) and min(c_bar, pi / mu).

The first chunk is still on-policy: the evaluation follows the sampler's arithmetic bit for bit, so log_prob IS old_log_prob there, every
weight is exactly 1.0, and `vs` has the bits of the returns of `env.advantages(...)` (GAE at the same gamma and lam) — printed below.

    python examples/impala_vtrace.py [--envs 4096] [--iterations 30]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def linear(obs, W):
    """obs [..., 4] times W [4, J] -> [..., J], in one fixed order of float32 operations whatever the leading shape."""
    return ((obs[..., 0:1] * W[0] + obs[..., 1:2] * W[1]) + obs[..., 2:3] * W[2]) + obs[..., 3:4] * W[3]


def train(num_envs: int = 4096, iterations: int = 30, K: int = 64, lr: float = 0.02, value_coef: float = 0.5, entropy_coef: float = 0.01,
          gamma: float = 0.99, lam: float = 1.0, rho_bar: float = 1.0, c_bar: float = 1.0, seed: int = 0, verbose: bool = True):
    import torch

    import gym_amd
    from gym_amd.rollout import DeviceRollout

    env = DeviceRollout("CartPole-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.enable_episode_stats()
    env.reset(seed=seed)
    sampler = env.policy_sampler()
    dev = env.device
    W = torch.zeros((4, 2), device=dev, requires_grad=True)        # the learner's policy: pi(. | obs) = softmax(linear(obs, W))
    W_behaviour = torch.zeros((4, 2), device=dev)                  # the actor's copy: one update behind from the second chunk on
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
            return sampler.sample(linear(obs, W_behaviour), out=step_out)[0]      # actions, log mu and entropy: one launch

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
            old_log_prob = traj["log_prob"]                                       # log mu(a): the behaviour policy's, from the sampler
            log_prob, entropy = gym_amd.evaluate_categorical(linear(traj["obs"], W), traj["actions"])      # log pi(a): the learner's
            values = value(traj["obs"])
            with torch.no_grad():
                last_value = value(env.obs)
                vs, pg_adv = env.vtrace(traj, values, log_prob.detach(), old_log_prob, last_value, gamma=gamma, lam=lam, rho_bar=rho_bar,
                                        c_bar=c_bar)
                log_ratio = log_prob.detach() - old_log_prob
                row = {"iteration": it, "log_ratio_min": float(log_ratio.min()), "log_ratio_max": float(log_ratio.max())}
                if it == 0:
                    ret = env.advantages(traj, values.detach(), last_value, gamma=gamma, lam=lam)[1]
                    row["vs_equals_gae_returns"] = bool(torch.equal(vs.view(torch.int32), ret.view(torch.int32)))
                    if verbose:
                        print(f"first chunk (on-policy): log pi - log mu in [{row['log_ratio_min']}, {row['log_ratio_max']}], "
                              f"vs equals the GAE returns bit for bit: {row['vs_equals_gae_returns']}")
                before = W.detach().clone()
            err = values - vs
            loss = -(pg_adv * log_prob).mean() + value_coef * 0.5 * (err * err).mean() - entropy_coef * entropy.mean()
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            optimizer.step()
            W_behaviour.copy_(before)              # the next chunk is drawn by the weights from before this update
            ended = (ep_len > 0).sum().clamp(min=1)
            row.update(mean_episode_length=float(ep_len.sum() / ended), episodes=int(ended), loss=float(loss.detach()))
            history.append(row)
            if verbose:
                print(f"iteration {it:3d}: {row['episodes']:6d} episodes ended, mean length {row['mean_episode_length']:7.1f}, "
                      f"loss {row['loss']:9.5f}, log pi - log mu in [{row['log_ratio_min']:+.4f}, {row['log_ratio_max']:+.4f}]")
    env.close()
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=30)
    a = ap.parse_args()
    h = train(a.envs, a.iterations)
    print(f"mean episode length {h[0]['mean_episode_length']:.1f} -> {h[-1]['mean_episode_length']:.1f}")
