#!/usr/bin/env python3
"""Replay-free parallel Q-learning (PQN-style) on CartPole-v1: 4 096 envs x 32 steps per iteration, no buffer, no torch generator.

Every piece of the update but the network itself runs in the engine's kernels:
  * exploration is Boltzmann: actions from `env.policy_sampler()` with logits = Q / temperature — one launch per policy step under the
    Philox contract, so two runs print identical histories; the temperature falls geometrically from 8 to 0.25 over the iterations
    (a head that starts at Q = 0 far below the returns must keep trying the action it has trained less);
  * the K steps of a chunk are recorded once into a graph and replayed.  The recording is the one `enable_graph_capture()` documents —
    `env.step(actions)` inside the caller's torch.cuda.graph — and not `env.graphed_loop`, whose steps do not write `final_obs`: the
    bootstrap of a truncated step needs it;
  * the targets are Peng's Q(lambda): `env.advantages(traj, values=max_a Q, ...)[1]`, the `returns` (= advantages + values) of the GAE
    kernel, bootstrapped from `last_value = max_a Q(obs after the chunk)` and, where a step was truncated, from
    `final_values = max_a Q(final_obs)`;
  * the loss is `gym_amd.dqn_loss(q, actions, targets=...)` — two launches forwards, one behind `loss.backward()` — and its eight
    diagnostics are read once per update with `stats.tolist()`.
`--double` switches to one-step double-DQN targets in the bootstrap mode: `next_q` from a target head that is copied from the online
one every few iterations, `next_q_online` from the online head, both on the next observation (the final observation where the step
was truncated), `terminated` from the rollout.

The Q head is a 4-32-2 tanh network written as broadcast multiplies and sums in a fixed order (no matrix product: a GEMM may reduce in
an order of its own), with Adam.

Measured on an MI355X with the defaults (mean length of the episodes that ended in the iteration, iteration 0 -> 59): 17.1 -> 197.6,
passing 43 at iteration 20 and 93 at iteration 40 (--iterations 120: 431.0); with --double: 17.1 -> 30.7, at most 40.8 (iteration 48) —
one-step targets carry a return back one step per update, which is what the lambda-returns are for.

    python examples/pqn_cartpole.py [--envs 4096] [--iterations 60] [--double]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def linear(obs, W):
    """obs [..., 4] times W [4, J] -> [..., J], in one fixed order of float32 operations whatever the leading shape."""
    return ((obs[..., 0:1] * W[0] + obs[..., 1:2] * W[1]) + obs[..., 2:3] * W[2]) + obs[..., 3:4] * W[3]


def q_head(obs, params):
    """Q(obs, .) [..., A] of the 4-H-A tanh network `params` = (W1 [4, H], b1 [H], W2 [H, A], b2 [A])."""
    import torch

    W1, b1, W2, b2 = params
    hidden = torch.tanh(linear(obs, W1) + b1)
    return (hidden.unsqueeze(-1) * W2).sum(-2) + b2


def train(num_envs: int = 4096, iterations: int = 60, K: int = 32, epochs: int = 8, lr: float = 1e-2, gamma: float = 0.99, lam: float = 0.65,
          temperature=(8.0, 0.25), delta: float = 1.0, hidden: int = 32, double: bool = False, target_every: int = 2, seed: int = 0,
          verbose: bool = True):
    import torch

    import gym_amd
    from gym_amd.dqn import STAT_NAMES
    from gym_amd.rollout import DeviceRollout

    env = DeviceRollout("CartPole-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.enable_episode_stats()
    env.reset(seed=seed)
    sampler = env.policy_sampler()                  # Discrete(2), the engine's action dtype, env_offset and action_seed
    dev = env.device
    f32 = dict(dtype=torch.float32, device=dev)
    # a fixed initialisation without a torch generator: a lattice of signs and magnitudes
    idx = torch.arange(4 * hidden, **f32).view(4, hidden)
    W1 = (torch.sin(idx * 1.7 + 0.3) * 0.5).requires_grad_()
    b1 = torch.zeros(hidden, **f32, requires_grad=True)
    W2 = (torch.cos(torch.arange(hidden * 2, **f32).view(hidden, 2) * 2.3) * 0.1).requires_grad_()
    b2 = torch.zeros(2, **f32, requires_grad=True)
    params = [W1, b1, W2, b2]
    target = [p.detach().clone() for p in params]
    optimizer = torch.optim.Adam(params, lr=lr)
    traj = {"obs": torch.empty((K, num_envs, 4), **f32), "next_obs": torch.empty((K, num_envs, 4), **f32),
            "final_obs": torch.zeros((K, num_envs, 4), **f32), "actions": torch.empty((K, num_envs), dtype=env.action_dtype, device=dev),
            "reward": torch.empty((K, num_envs), dtype=env.reward_dtype, device=dev),
            "terminated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev),
            "truncated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev)}
    ep_len = torch.zeros((K, num_envs), **f32)
    step_out = (torch.empty(num_envs, dtype=env.action_dtype, device=dev), torch.empty(num_envs, **f32), torch.empty(num_envs, **f32))
    # 1 / temperature in device memory: the recorded steps read it, so a replay follows the schedule (geometric, first to last iteration)
    inv_temperature = torch.full((), 1.0 / temperature[0], **f32)

    def one_step(k):
        traj["obs"][k].copy_(env.obs)                                             # the observation the action is chosen on
        with torch.no_grad():
            actions = sampler.sample(q_head(env.obs, params) * inv_temperature, out=step_out)[0]      # Boltzmann exploration: one launch
        env.step(actions)                                                         # writes final_obs where the episode ended
        traj["actions"][k].copy_(actions)
        traj["next_obs"][k].copy_(env.obs)
        traj["final_obs"][k].copy_(env.final_obs)
        traj["reward"][k].copy_(env.reward)
        traj["terminated"][k].copy_(env.terminated)
        traj["truncated"][k].copy_(env.truncated)
        ep_len[k].copy_(env.ep_length * (env.terminated | env.truncated))

    env.enable_graph_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(env.stream):
        for k in range(3):                                                        # lazy initialisation stays outside the recording
            one_step(k)
        env.stream.synchronize()
        with torch.cuda.graph(graph, stream=env.stream):
            for k in range(K):
                one_step(k)
    history = []
    with torch.cuda.stream(env.stream):
        for it in range(iterations):
            tau = temperature[0] * (temperature[1] / temperature[0]) ** (it / max(iterations - 1, 1))
            inv_temperature.fill_(1.0 / tau)
            graph.replay()                                                        # K policy steps and K env steps, one host call
            with torch.no_grad():
                truncated = (traj["truncated"] != 0) & (traj["terminated"] == 0)
                if double:
                    if it % target_every == 0:
                        for t, p in zip(target, params):
                            t.copy_(p)
                    # the observation the bootstrap looks at: the next one, and the final one where the step was truncated
                    next_obs = torch.where(truncated.unsqueeze(-1), traj["final_obs"], traj["next_obs"])
                    next_q, next_q_online = q_head(next_obs, target), q_head(next_obs, params)
                    reward = traj["reward"].float()                               # the engine's rewards are float64
                else:
                    values = q_head(traj["obs"], params).max(-1).values
                    last_value = q_head(env.obs, params).max(-1).values
                    final_values = q_head(traj["final_obs"], params).max(-1).values
                    targets = env.advantages(traj, values, last_value, gamma=gamma, lam=lam, final_values=final_values)[1]
            for _ in range(epochs):
                q = q_head(traj["obs"], params)
                if double:
                    loss, stats = gym_amd.dqn_loss(q, traj["actions"], reward=reward, terminated=traj["terminated"], next_q=next_q,
                                                   next_q_online=next_q_online, gamma=gamma, delta=delta)
                else:
                    loss, stats = gym_amd.dqn_loss(q, traj["actions"], targets=targets, delta=delta)
                optimizer.zero_grad(set_to_none=True)
                loss.backward()
                optimizer.step()
                diagnostics = dict(zip(STAT_NAMES, stats.tolist()))               # the one host read of the update
            ended = (ep_len > 0).sum().clamp(min=1)
            row = {"iteration": it, "temperature": tau, "mean_episode_length": float(ep_len.sum() / ended), "episodes": int(ended), **diagnostics}
            history.append(row)
            if verbose:
                print(f"iteration {it:3d}: temperature {tau:5.2f}, {row['episodes']:6d} episodes ended, mean length {row['mean_episode_length']:7.1f}, "
                      f"loss {row['loss_term']:9.5f}, |td| mean {row['td_abs_mean']:8.5f} max {row['td_abs_max']:8.4f}, "
                      f"Q taken mean {row['q_taken_mean']:8.4f} max {row['q_taken_max']:8.4f}, target mean {row['target_mean']:8.4f}, "
                      f"linear {row['linear_fraction']:.3f}")
    policy_steps = sampler.step_index()
    env.close()
    if verbose:
        print(f"{policy_steps} policy steps drawn")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=8, help="full-batch Adam steps per chunk")
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--temperature", type=float, nargs=2, default=(8.0, 0.25), metavar=("FIRST", "LAST"),
                    help="Boltzmann temperature of the first and of the last iteration (geometric in between)")
    ap.add_argument("--double", action="store_true", help="one-step double-DQN targets with a periodically copied target head")
    a = ap.parse_args()
    h = train(a.envs, a.iterations, epochs=a.epochs, lr=a.lr, temperature=tuple(a.temperature), double=a.double)
    print(f"mean episode length {h[0]['mean_episode_length']:.1f} -> {h[-1]['mean_episode_length']:.1f}")
