#!/usr/bin/env python3
"""Rainbow's core on CartPole-v1: categorical (C51) double DQN with a dueling head, 3-step returns and prioritised experience replay —
the graphed sampling loop of `c51_cartpole.py`, the n-step prioritised buffer of `dqn_nstep_cartpole.py`, and between them the one call
that joins the two: `gym_amd.categorical_targets`, which projects `reward + discount * z` with the per-row discount of the n-step
batch.  No torch generator anywhere.

What differs from `c51_cartpole.py`:
  * the buffer is `env.nstep_replay_buffer(capacity, n_step, gamma, prioritized=True)`: `sample` returns the n-step return as `reward`,
    the window's last observation as `next_obs` and `discount` = gamma^(steps taken) per row;
  * the head is dueling (Wang et al. 2016), in torch: a value stream [..., 1, Z] and an advantage stream [..., A, Z] over one hidden
    layer, logits = value + advantage - mean_a advantage;
  * each update builds the target distribution in one launch and hands it to the loss's given mode:
        m = gym_amd.categorical_targets(target_net(next_obs), b["reward"], b["terminated"], v_min=, v_max=, discount=b["discount"],
                                        next_logits_online=online_net(next_obs))
        loss, stats = gym_amd.categorical_dqn_loss(logits, b["actions"], v_min=, v_max=, target_probs=m, weights=b["weights"],
                                                   row_loss=row_loss)
    the fused bootstrap of the loss reads one scalar gamma and cannot take this batch; the backward reads `m` and does not repeat the
    selecting pass; `row_loss` (the cross-entropy of each row) goes to `buf.update_priorities`.
Noisy nets (Fortunato et al. 2018), Rainbow's sixth component, are not part of this: they are layers of the network, and they draw
from a generator; exploration here is the Boltzmann draw of `c51_cartpole.py`.
Priorities are exact integers, the draws Philox-keyed and every sum of the loss a fixed tree, so two runs draw the same batches and
print identical histories.

    python examples/rainbow_cartpole.py [--envs 256] [--iterations 60] [--n-step 3] [--atoms 51] [--support 0 100] [--updates 32] [--batch 2048]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pqn_cartpole import linear  # noqa: E402  (the first layer, in the same fixed order of operations)

ACTIONS = 2


def train(num_envs: int = 256, iterations: int = 60, K: int = 32, updates: int = 32, batch: int = 2048, capacity: int = 1 << 17, lr: float = 3e-3,
          gamma: float = 0.99, temperature=(4.0, 0.1), atoms: int = 51, support=(0.0, 100.0), hidden: int = 32, target_every: int = 2, seed: int = 0,
          alpha: float = 0.6, beta=(0.4, 1.0), eps: float = 1e-6, n_step: int = 3, verbose: bool = True):
    import torch

    import gym_amd
    from gym_amd.c51 import STAT_NAMES
    from gym_amd.rollout import DeviceRollout

    v_min, v_max = support
    env = DeviceRollout("CartPole-v1", num_envs, seed=seed, action_seed=seed + 1)
    env.enable_episode_stats()
    env.reset(seed=seed)
    sampler = env.policy_sampler()                  # Discrete(2), the engine's action dtype, env_offset and action_seed
    buf = env.nstep_replay_buffer(capacity, n_step, gamma, prioritized=True, alpha=alpha, eps=eps)      # float32 [4] rows, seed = the rollout's action_seed
    dev = env.device
    f32 = dict(dtype=torch.float32, device=dev)
    width = (ACTIONS + 1) * atoms                   # the advantage stream's A * Z columns, then the value stream's Z
    # a fixed initialisation without a torch generator: a lattice of signs and magnitudes
    idx = torch.arange(4 * hidden, **f32).view(4, hidden)
    W1 = (torch.sin(idx * 1.7 + 0.3) * 0.5).requires_grad_()
    b1 = torch.zeros(hidden, **f32, requires_grad=True)
    W2 = (torch.cos(torch.arange(hidden * width, **f32).view(hidden, width) * 2.3) * 0.1).requires_grad_()
    b2 = torch.zeros(width, **f32, requires_grad=True)
    params = [W1, b1, W2, b2]
    target = [p.detach().clone() for p in params]
    optimizer = torch.optim.Adam(params, lr=lr)

    def head(obs, weights):
        """dueling logits [..., 2, atoms] = value [..., 1, atoms] + advantage [..., 2, atoms] - its mean over the actions"""
        w1, c1, w2, c2 = weights
        h = torch.tanh(linear(obs, w1) + c1)
        out = (h.unsqueeze(-1) * w2).sum(-2) + c2
        adv = out[..., :ACTIONS * atoms].unflatten(-1, (ACTIONS, atoms))
        value = out[..., ACTIONS * atoms:].unsqueeze(-2)
        return (value + (adv - (adv[..., 0, :] + adv[..., 1, :]).unsqueeze(-2) * 0.5)).contiguous()

    first_obs = torch.empty((num_envs, 4), **f32)
    # traj["obs"][k] is the observation AFTER step k, as rollout_per_step leaves it
    traj = {"obs": torch.empty((K, num_envs, 4), **f32), "final_obs": torch.zeros((K, num_envs, 4), **f32),
            "actions": torch.empty((K, num_envs), dtype=env.action_dtype, device=dev),
            "reward": torch.empty((K, num_envs), dtype=env.reward_dtype, device=dev),
            "terminated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev),
            "truncated": torch.empty((K, num_envs), dtype=torch.uint8, device=dev)}
    ep_len = torch.zeros((K, num_envs), **f32)
    step_out = (torch.empty(num_envs, dtype=env.action_dtype, device=dev), torch.empty(num_envs, **f32), torch.empty(num_envs, **f32))
    q_act = torch.empty((num_envs, ACTIONS), **f32)
    inv_temperature = torch.full((), 1.0 / temperature[0], **f32)      # in device memory: the recorded steps read it
    drawn = buf.sample_buffers(batch)
    row_loss = torch.empty(batch, **f32)
    target_probs = torch.empty((batch, atoms), **f32)
    clipped = torch.empty(batch, **f32)

    def one_step(k):
        with torch.no_grad():
            q = gym_amd.categorical_q_values(head(env.obs, params), v_min=v_min, v_max=v_max, out=q_act)      # one launch
            actions = sampler.sample(q * inv_temperature, out=step_out)[0]            # Boltzmann exploration over the expected values
        env.step(actions)                                                         # writes final_obs where the episode ended
        traj["actions"][k].copy_(actions)
        traj["obs"][k].copy_(env.obs)
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
            first_obs.copy_(env.obs)                                              # the observation the chunk starts from
            for k in range(K):
                one_step(k)
    history = []
    with torch.cuda.stream(env.stream):
        for it in range(iterations):
            tau = temperature[0] * (temperature[1] / temperature[0]) ** (it / max(iterations - 1, 1))
            inv_temperature.fill_(1.0 / tau)
            b_it = beta[0] + (beta[1] - beta[0]) * it / max(iterations - 1, 1)      # annealed towards the unbiased estimate
            graph.replay()                                                        # K policy steps and K env steps, one host call
            buf.add_chunk(first_obs, traj)                                        # K * N n-step transitions at the largest priority seen
            if it % target_every == 0:
                with torch.no_grad():
                    for t, p in zip(target, params):
                        t.copy_(p)
            for _ in range(updates):
                b = buf.sample(batch, beta=b_it, out=drawn)                       # three launches, no allocation
                with torch.no_grad():
                    online_next, target_next = head(b["next_obs"], params), head(b["next_obs"], target)
                m = gym_amd.categorical_targets(target_next, b["reward"], b["terminated"], v_min=v_min, v_max=v_max, discount=b["discount"],
                                                next_logits_online=online_next, clipped_mass=clipped, out=target_probs)      # one launch
                loss, stats = gym_amd.categorical_dqn_loss(head(b["obs"], params), b["actions"], v_min=v_min, v_max=v_max, target_probs=m,
                                                           weights=b["weights"], row_loss=row_loss)
                optimizer.zero_grad(set_to_none=True)
                loss.backward()
                optimizer.step()
                buf.update_priorities(b["indices"], row_loss)                      # two launches
            diagnostics = dict(zip(STAT_NAMES, stats.tolist()))                   # the one host read of the iteration
            diagnostics["clipped_mass_mean"] = float(clipped.double().mean())     # the given mode of the loss reports 0: the targets call has it
            ended = (ep_len > 0).sum().clamp(min=1)
            row = {"iteration": it, "temperature": tau, "beta": b_it, "mean_episode_length": float(ep_len.sum() / ended), "episodes": int((ep_len > 0).sum()),
                   "stored": len(buf), "discount_mean": float(b["discount"].mean()), "discount_min": float(b["discount"].min()), **diagnostics}
            history.append(row)
            if verbose:
                print(f"iteration {it:3d}: temperature {tau:5.2f}, {row['episodes']:5d} episodes ended, mean length {row['mean_episode_length']:7.1f}, "
                      f"{row['stored']:7d} stored, loss {row['loss_term']:9.5f} (row max {row['row_loss_max']:8.4f}), "
                      f"Q taken mean {row['q_taken_mean']:8.4f} max {row['q_taken_max']:8.4f}, target mean {row['target_mean']:8.4f}, "
                      f"entropy {row['entropy_mean']:6.4f}, clipped mass {row['clipped_mass_mean']:8.6f}")
    sample_steps = buf.sample_step
    env.close()
    if verbose:
        print(f"{sample_steps} sample steps drawn from {n_step}-step transitions ({atoms} atoms on [{v_min}, {v_max}], gamma {gamma}, dueling head)")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--updates", type=int, default=32, help="sampled Adam steps per chunk")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--capacity", type=int, default=1 << 17)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--target-every", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--n-step", type=int, default=3, help="steps of a window at most")
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--support", type=float, nargs=2, default=(0.0, 100.0), metavar=("V_MIN", "V_MAX"))
    ap.add_argument("--beta", type=float, nargs=2, default=(0.4, 1.0), metavar=("FIRST", "LAST"))
    ap.add_argument("--temperature", type=float, nargs=2, default=(4.0, 0.1), metavar=("FIRST", "LAST"),
                    help="Boltzmann temperature of the first and of the last iteration (geometric in between)")
    a = ap.parse_args()
    h = train(a.envs, a.iterations, updates=a.updates, batch=a.batch, capacity=a.capacity, lr=a.lr, temperature=tuple(a.temperature),
              atoms=a.atoms, support=tuple(a.support), target_every=a.target_every, alpha=a.alpha, beta=tuple(a.beta), n_step=a.n_step)
    print("mean episode length by iteration: " + " ".join(f"{r['mean_episode_length']:.1f}" for r in h))
    print(f"mean episode length {h[0]['mean_episode_length']:.1f} -> {h[-1]['mean_episode_length']:.1f}")
