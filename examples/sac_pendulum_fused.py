#!/usr/bin/env python3
"""Soft actor-critic (Haarnoja et al. 2018) on Pendulum-v1 with the fused losses of gym_amd.sac: the learner of examples/sac_pendulum.py —
4 096 envs x 8 steps per iteration into a device ring, several sampled updates per chunk, no torch generator anywhere — with
everything between the draw and the optimizer on the engine's kernels.

  * acting: `sampler = env.squashed_gaussian_sampler()` — the env's bounds (+-2), the rollout's env_offset, device and action seed —
    and `sampler.sample(mean, log_std)`: ONE launch from the actor's head to the bounded action, no graph;
  * `buf = env.replay_buffer(capacity)` stores float32 actions; `buf.add_chunk(first_obs, traj)` one chunk in ONE launch, with the
    final observation where a step was truncated; `buf.sample(batch)` ONE launch under Philox stream tag 9;
  * the critics' target draws the next action with `sampler.sample` too; `gym_amd.soft_q_targets` makes
    y = r + gamma (1 - term) (min(Q1', Q2') - alpha log pi') of the target critics' outputs as one [M, 2] tensor in ONE launch, the
    temperature read from device memory (`log_alpha.detach().exp()` goes straight in);
  * the twin critics regress on it through `gym_amd.twin_q_loss(q12, targets=y)`: the critics' outputs as one [M, 2] tensor, the sum of
    the two half squared errors, its diagnostics and the dense gradient — 2 launches forwards, ONE behind `loss.backward()`;
  * the actor's update is `sampler.rsample(mean, log_std)` and `gym_amd.soft_policy_loss(log_prob, q12_pi, alpha=alpha)`:
    alpha log pi - min(Q1, Q2), its diagnostics, and ONE backward launch for both gradients (on a tie the first critic takes the whole
    gradient, where torch.minimum splits it);
  * the temperature alpha is learned against the target entropy -1 (minus the action dim): three scalar torch ops on the device
    scalar stats[1] (log_prob_mean) of the actor's loss;
  * the diagnostics of both losses are read ONCE per iteration.
Every draw is a function of (seed, row, step) under the Philox contract (tag 11 for the actions), so two runs print identical histories.

Actor (3-H-2) and critics (4-H-1) are tanh networks with a fixed, generator-free initialisation and Adam.

    python examples/sac_pendulum_fused.py [--envs 4096] [--iterations 150] [--updates 8] [--batch 4096]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOG_STD_MIN, LOG_STD_MAX = -5.0, 2.0


def _init(torch, rows, cols, phase, gain, **f32):
    """A fixed initialisation without a torch generator: a lattice of signs and magnitudes."""
    idx = torch.arange(rows * cols, **f32).view(rows, cols)
    return (torch.sin(idx * 1.7 + phase) * gain).requires_grad_()


def _mlp(torch, n_in, hidden, n_out, phase, **f32):
    return [_init(torch, n_in, hidden, phase, 0.5, **f32), torch.zeros(hidden, **f32, requires_grad=True),
            _init(torch, hidden, n_out, phase + 0.9, 0.1, **f32), torch.zeros(n_out, **f32, requires_grad=True)]


def _net(torch, x, p):
    """The tanh network p = (W1 [I, H], b1 [H], W2 [H, J], b2 [J]) on x [M, I] as broadcast multiplies and sums in one fixed order of
    float32 operations (no BLAS call, whose order of additions may differ between two runs)."""
    W1, b1, W2, b2 = p
    pre = x[:, 0:1] * W1[0]
    for j in range(1, x.shape[1]):
        pre = pre + x[:, j:j + 1] * W1[j]
    return (torch.tanh(pre + b1).unsqueeze(-1) * W2).sum(-2) + b2


def _actor(torch, obs, p):
    """-> (mean [M, 1], log_std [M, 1]), log_std squashed into [LOG_STD_MIN, LOG_STD_MAX]."""
    out = _net(torch, obs, p)
    ls = LOG_STD_MIN + 0.5 * (LOG_STD_MAX - LOG_STD_MIN) * (torch.tanh(out[:, 1:2]) + 1.0)
    return out[:, 0:1].contiguous(), ls.contiguous()


def _critic(torch, obs, act, p, bound):
    """Q(obs, action) [M, 1]; the action enters in units of its bound."""
    return _net(torch, torch.cat((obs, act.view(-1, 1) / bound), dim=1), p)


def _critics(torch, obs, act, pair, bound):
    """Both critics as one [M, 2] tensor: column c is critic c."""
    return torch.cat((_critic(torch, obs, act, pair[0], bound), _critic(torch, obs, act, pair[1], bound)), dim=1)


def train(num_envs: int = 4096, iterations: int = 150, K: int = 8, updates: int = 8, batch: int = 4096, capacity: int = 1 << 20,
          lr: float = 3e-3, gamma: float = 0.99, tau: float = 0.02, hidden: int = 64, reward_scale: float = 0.1, seed: int = 0,
          verbose: bool = True):
    import torch

    import gym_amd
    from gym_amd.rollout import DeviceRollout

    env = DeviceRollout("Pendulum-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.reset(seed=seed)
    sampler = env.squashed_gaussian_sampler()       # Box(-2, 2): scale 2, bias 0; the engine's env_offset and action_seed
    bound = sampler.scale[0]
    buf = env.replay_buffer(max(capacity, K * num_envs))      # float32 [3] rows, float32 actions
    dev = env.device
    f32 = dict(dtype=torch.float32, device=dev)
    O = env.O
    actor = _mlp(torch, O, hidden, 2, 0.3, **f32)
    critics = [_mlp(torch, O + 1, hidden, 1, 0.7, **f32), _mlp(torch, O + 1, hidden, 1, 1.9, **f32)]
    targets = [[p.detach().clone() for p in c] for c in critics]
    log_alpha = torch.zeros((), **f32, requires_grad=True)
    target_entropy = -1.0
    opt_actor = torch.optim.Adam(actor, lr=lr)
    opt_critic = torch.optim.Adam(critics[0] + critics[1], lr=lr)
    opt_alpha = torch.optim.Adam([log_alpha], lr=lr)
    first_obs = torch.empty((num_envs, O), **f32)
    traj = {"obs": torch.empty((K, num_envs, O), **f32), "final_obs": torch.zeros((K, num_envs, O), **f32),
            "actions": torch.empty((K, num_envs), **f32), "reward": torch.empty((K, num_envs), dtype=env.reward_dtype, device=dev),
            "terminated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev),
            "truncated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev)}
    drawn = buf.sample_buffers(batch)
    history = []
    with torch.cuda.stream(env.stream):
        for it in range(iterations):
            first_obs.copy_(env.obs)
            with torch.no_grad():
                for k in range(K):
                    mean, log_std = _actor(torch, env.obs, actor)
                    actions, _ = sampler.sample(mean, log_std)                    # ONE launch: the bounded action of every env
                    env.step(actions)                                             # writes final_obs where the episode was truncated
                    traj["actions"][k].copy_(actions.view(-1))
                    traj["obs"][k].copy_(env.obs)
                    traj["final_obs"][k].copy_(env.final_obs)
                    traj["reward"][k].copy_(env.reward * reward_scale)
                    traj["terminated"][k].copy_(env.terminated)
                    traj["truncated"][k].copy_(env.truncated)
            buf.add_chunk(first_obs, traj)                                        # K * N transitions, one launch
            for _ in range(updates):
                b = buf.sample(batch, out=drawn)                                  # one launch, no allocation
                alpha = log_alpha.detach().exp()
                with torch.no_grad():                                             # the soft target: a fresh action at the next observation
                    a2, lp2 = sampler.sample(*_actor(torch, b["next_obs"], actor))
                    y = gym_amd.soft_q_targets(_critics(torch, b["next_obs"], a2, targets, bound), b["reward"], b["terminated"],
                                               next_log_prob=lp2.view(-1), alpha=alpha, gamma=gamma)      # ONE launch; alpha read on the device
                # twin critics: the sum of the two half squared errors against y, fused; q_stats stays on the device
                critic_loss, q_stats = gym_amd.twin_q_loss(_critics(torch, b["obs"], b["actions"], critics, bound), targets=y)
                opt_critic.zero_grad(set_to_none=True)
                critic_loss.backward()
                opt_critic.step()
                a1, lp1 = sampler.rsample(*_actor(torch, b["obs"], actor))        # differentiable in mean and log_std: one launch each way
                actor_loss, pi_stats = gym_amd.soft_policy_loss(lp1.view(-1), _critics(torch, b["obs"], a1, critics, bound), alpha=alpha)
                opt_actor.zero_grad(set_to_none=True)
                actor_loss.backward()
                opt_actor.step()
                alpha_loss = -(log_alpha * (pi_stats[1] + target_entropy))        # log_prob_mean: a device scalar, no graph
                opt_alpha.zero_grad(set_to_none=True)
                alpha_loss.backward()
                opt_alpha.step()
                with torch.no_grad():
                    for tc, c in zip(targets, critics):
                        for tp, p in zip(tc, c):
                            tp.mul_(1.0 - tau).add_(p, alpha=tau)
            qs, ps = q_stats.tolist(), pi_stats.tolist()                          # the diagnostics of the last update, read once per iteration
            row = {"iteration": it, "mean_reward": float(traj["reward"].mean()) / reward_scale, "alpha": float(log_alpha.detach().exp()),
                   "mean_log_prob": ps[1], "critic_loss": qs[0], "actor_loss": ps[0], "q_mean": qs[2], "td_abs_mean": qs[1], "td_abs_max": qs[5],
                   "target_mean": qs[3], "critic_gap": qs[4], "q_min": qs[6], "q_max": qs[7], "later_critic_fraction": ps[4], "stored": len(buf)}
            history.append(row)
            if verbose:
                print(f"iteration {it:3d}: mean reward per step {row['mean_reward']:8.4f}, alpha {row['alpha']:7.4f}, "
                      f"log_prob {row['mean_log_prob']:8.4f}, critic loss {row['critic_loss']:10.5f}, actor loss {row['actor_loss']:9.4f}, "
                      f"Q mean {row['q_mean']:9.4f}, critic gap {row['critic_gap']:8.4f}, later critic {row['later_critic_fraction']:5.3f}, "
                      f"{row['stored']:8d} stored")
    drawn_steps = sampler.step_index()
    env.close()
    if verbose:
        print(f"{drawn_steps} action draws made")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--updates", type=int, default=8, help="sampled SAC updates per chunk")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--lr", type=float, default=3e-3)
    a = ap.parse_args()
    h = train(a.envs, a.iterations, updates=a.updates, batch=a.batch, lr=a.lr)
    print("mean reward per step by iteration: " + " ".join(f"{r['mean_reward']:.2f}" for r in h[::10]))
    print(f"mean reward per step {h[0]['mean_reward']:.3f} -> {h[-1]['mean_reward']:.3f}")
