#!/usr/bin/env python3
"""Vectorised (SAFE)MADDPG training on the HIP environment — BASELINE.json configs 3-5.

    python examples/train_maddpg.py --alg maddpg --envs 4096 --episodes 3
    python examples/train_maddpg.py --alg safemaddpg --envs 8192 --episodes 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_maddpg.py ...

One "episode" is 95 vector steps.  Env shards are independent; with more than one rank the
only collective is the flat gradient bucket all-reduce per optimiser step (RCCL over xGMI).
Prints one JSON line with whole-job env-steps/s including policy inference, replay writes and the
11 gradient steps per 60 vector steps of model.py:40-71.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_ALG_ARGS = dict(  # madrl/args/default.yaml merged with alg_args/maddpg.yaml
    gumbel_softmax=False, epsilon_softmax=False, softmax_eps=None, episodic=False, cuda=True, grad_clip_eps=1.0,
    save_model_freq=40, replay_warmup=0, policy_lrate=1.0e-4, value_lrate=1.0e-4, mixer_lrate=None, target=True,
    target_lr=0.1, entr=1.0e-3, max_steps=240, batch_size=32, replay=True, replay_buffer_size=5.0e3, agent_type="rnn",
    agent_id=True, shared_params=True, layernorm=True, mixer=False, gaussian_policy=False, LOG_STD_MIN=0.0,
    LOG_STD_MAX=0.5, fixed_policy_std=1.0, hid_activation="relu", init_type="normal", init_std=0.1,
    action_enforcebound=True, double_q=True, clip_c=1.0, gamma=0.99, hid_size=64, continuous=True,
    normalize_advantages=False, train_episodes_num=400, behaviour_update_freq=60, target_update_freq=120,
    policy_update_epochs=1, value_update_epochs=10, mixer_update_epochs=None, reward_normalisation=True, eval_freq=20,
    num_eval_episodes=10, action_low=0, action_high=1.0, action_bias=0.0, action_scale=1.0,
)

# alg_args/facmaddpg.yaml over the defaults above (kept apart: DEFAULT_ALG_ARGS is the MADDPG configuration)
FACMADDPG_ALG_ARGS = dict(
    policy_lrate=1.0e-3, value_lrate=1.0e-3, mixer_lrate=1.0e-3, gaussian_policy=False, action_enforcebound=True,
    policy_update_epochs=1, value_update_epochs=1, mixer_update_epochs=1, grad_clip_eps=1.0, fixed_policy_std=1.0,
    double_q=True, target_lr=0.01, hypernet_layers=2, hypernet_embed=64, mixing_embed_dim=64,
    hyper_initialization_nonzeros=False, gated=False, skip_connections=False, mixer=True, behaviour_update_freq=60,
    target_update_freq=4800,
)

# alg_args/sqddpg.yaml over the defaults above
SQDDPG_ALG_ARGS = dict(policy_lrate=1.0e-4, value_lrate=1.0e-4, sample_size=10, gaussian_policy=False,
                       action_enforcebound=True)

# alg_args/ippo.yaml and mappo.yaml (the same settings) over the defaults above: on-policy, an update event every 240
# vector steps of ten value and ten policy sub-updates on pooled windows of 32 steps of every environment
PPO_ALG_ARGS = dict(policy_lrate=1.0e-4, value_lrate=1.0e-4, value_update_epochs=10, policy_update_epochs=10, lambda_=0.95,
                    eps_clip=0.6, value_loss_coef=2.0, reward_normalisation=True, normalize_advantages=True,
                    gaussian_policy=False, action_enforcebound=True, behaviour_update_freq=240, target_update_freq=480)

# alg_args/coma.yaml over the defaults above: on-policy, an update event every 60 vector steps of ten value sub-updates and
# one policy sub-update on pooled windows of 32 steps of every environment; ten draws per agent for the baseline
COMA_ALG_ARGS = dict(policy_lrate=1.0e-4, value_lrate=1.0e-4, sample_size=10, gaussian_policy=False,
                     action_enforcebound=True)

# alg_args/maac.yaml over the defaults above: soft actor-critic with ONE attention critic for all agents (csrc/attn_critic.hip);
# off-policy with transition replay, an update event every 60 vector steps like MADDPG
MAAC_ALG_ARGS = dict(policy_lrate=1.0e-4, value_lrate=1.0e-4, attend_heads=1, norm_in=False, soft=True, reward_scale=100,
                     gaussian_policy=True, action_enforcebound=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alg", choices=["maddpg", "safemaddpg", "matd3", "iddpg", "facmaddpg", "sqddpg", "ippo", "mappo", "coma", "maac"],
                    default="maddpg")
    ap.add_argument("--envs", type=int, default=4096, help="envs per GPU")
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--agents", type=int, default=5, choices=[3, 5])
    ap.add_argument("--batch-scale", type=int, default=None)
    ap.add_argument("--gaussian-policy", action="store_true",
                    help="learned log-std heads (gaussian_policy: True, LOG_STD_MIN 0.0 / LOG_STD_MAX 0.5 of default.yaml)")
    ap.add_argument("--gauss-burst", action="store_true",
                    help="with --gaussian-policy and an agent-summed --alg: the rollout as one persistent launch per run of "
                         "steps, log-std head included (FLEX_GAUSS_BURST=1, flexenv_rollout_burst_summed_gauss; with --agent-type mlp "
                         "flexenv_rollout_burst_summed_mlp)")
    ap.add_argument("--agent-type", choices=["rnn", "mlp"], default="rnn",
                    help="agent_type of default.yaml: the recurrent agent, or the MLP agent on the stacked history "
                         "(csrc/actor_mlp.hip; its rollout is the one-launch burst with the MLP policy phase: "
                         "flexenv_rollout_burst_mlp under maddpg / safemaddpg, flexenv_rollout_burst_summed_mlp under the "
                         "agent-summed algorithms; FLEX_MLP_BURST=0 switches both off)")
    ap.add_argument("--unshared", action="store_true",
                    help="shared_params: False of default.yaml — one actor and one critic per agent (csrc/actor_unshared.hip)")
    ap.add_argument("--unshared-twins", action="store_true",
                    help="shared_params: False under --alg matd3 — one actor and one twin-flag critic per agent "
                         "(csrc/critic_unshared_twin.hip: both heads from one first layer)")
    ap.add_argument("--unshared-critics", action="store_true",
                    help="with --unshared and --alg sqddpg | facmaddpg: the per-agent critics through the HIP kernels "
                         "(FLEX_UNSHARED_CRITICS=1: csrc/sqddpg_unshared.hip, csrc/critic_unshared.hip) instead of the tensor "
                         "composition / the per-agent loop")
    ap.add_argument("--episodic", action="store_true",
                    help="episodic: True of default.yaml — one update event per block of 95 vector steps, on batches of whole "
                         "episodes gathered by csrc/episodes.hip (ippo / mappo / coma: the on-policy triple batch_size = "
                         "replay_buffer_size = behaviour_update_freq, in blocks)")
    ap.add_argument("--intended-actions", action="store_true",
                    help="with --alg safemaddpg: SAFEMADDPG.intended_actions — every building's adjusted controls reach the env "
                         "as they are, agent-major (not the reference's routing; the form that learns)")
    ap.add_argument("--intended-launch", action="store_true",
                    help="with --intended-actions: that routing inside the one-launch rollout burst (FLEX_INTENDED_LAUNCH=1, "
                         "flexenv_rollout_burst_routed) instead of a policy, a projection, a transpose and an env launch per step")
    a = ap.parse_args()
    if a.intended_actions and a.alg != "safemaddpg":
        ap.error("--intended-actions: needs --alg safemaddpg")
    if a.intended_launch:
        if not a.intended_actions:
            ap.error("--intended-launch: needs --intended-actions")
        os.environ["FLEX_INTENDED_LAUNCH"] = "1"         # (read when the trainer builds its RolloutGraph)
    if a.gauss_burst:
        if not a.gaussian_policy or a.alg not in ("matd3", "iddpg", "facmaddpg", "sqddpg", "ippo", "mappo", "coma"):
            ap.error("--gauss-burst: needs --gaussian-policy and an agent-summed --alg "
                     "(matd3, iddpg, facmaddpg, sqddpg, ippo, mappo, coma)")
        os.environ["FLEX_GAUSS_BURST"] = "1"             # (read when the trainer builds its RolloutGraph)
    if a.unshared and a.alg == "matd3":
        ap.error("--unshared: MATD3 is built for shared_params (default.yaml:26); its per-agent twin critics are "
                 "asked for with --unshared-twins")
    if a.unshared_twins and a.alg != "matd3":
        ap.error("--unshared-twins: needs --alg matd3 (the other algorithms take --unshared)")
    if a.unshared_critics:
        if not a.unshared or a.alg not in ("sqddpg", "facmaddpg"):
            ap.error("--unshared-critics: needs --unshared and --alg sqddpg or facmaddpg")
        os.environ["FLEX_UNSHARED_CRITICS"] = "1"        # (read at every call of the critics)

    import torch
    import safe_marl_amd  # noqa: F401
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import COMA, FACMADDPG, IDDPG, IPPO, MAAC, MADDPG, MAPPO, MATD3, SAFEMADDPG, SQDDPG
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS, convert

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    blds = [5, 10, 15, 20, 25] if a.agents == 5 else [5, 15, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    if a.alg == "safemaddpg":
        env_args["alg"] = "safemaddpg"
    net = create_network(env_args)
    series = make_synthetic_series(net, n_days=365)
    env = VecFlexProvisionEnv(env_args, a.envs, device=f"cuda:{local}", net=net, series=series,
                              seed=1234 + 1000 * rank, warm_start=True)
    alg = dict(DEFAULT_ALG_ARGS)
    if a.alg == "facmaddpg":
        alg.update(FACMADDPG_ALG_ARGS)
    if a.alg == "sqddpg":
        alg.update(SQDDPG_ALG_ARGS)
    if a.alg in ("ippo", "mappo"):
        alg.update(PPO_ALG_ARGS)
    if a.alg == "coma":
        alg.update(COMA_ALG_ARGS)
    if a.alg == "maac":
        alg.update(MAAC_ALG_ARGS)
    if a.gaussian_policy:
        alg.update(gaussian_policy=True)
    if a.agent_type != "rnn":
        alg.update(agent_type=a.agent_type)
    if a.unshared or a.unshared_twins:
        alg.update(shared_params=False)
    if a.episodic:
        # capacity and cadence count BLOCKS of 95 vector steps of every environment (replay_buffer.EpisodeReplayBuffer)
        if a.alg in ("ippo", "mappo", "coma"):
            alg.update(episodic=True, batch_size=2, replay_buffer_size=2, behaviour_update_freq=2)      # default.yaml:1
        else:
            alg.update(episodic=True, replay_buffer_size=2, behaviour_update_freq=1)
    alg.update(alg=a.alg, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size,
               action_dim=4, v_min=0.9, v_max=1.1)
    args = convert(alg)
    torch.manual_seed(0)
    trainer = PGTrainer(args, {"maddpg": MADDPG, "safemaddpg": SAFEMADDPG, "matd3": MATD3, "iddpg": IDDPG,
                                 "facmaddpg": FACMADDPG, "sqddpg": SQDDPG, "ippo": IPPO, "mappo": MAPPO,
                                 "coma": COMA, "maac": MAAC}[a.alg], env, None,
                        batch_scale=a.batch_scale,
                        # (on-policy: the trainer's default holds what is collected between two update events)
                        replay_capacity=None if a.alg in ("ippo", "mappo", "coma") else a.envs * 96 * 2)
    if a.intended_actions:
        trainer.behaviour_net.intended_actions = True           # (before the first episode builds the RolloutGraph)
    stat = {}
    trainer.behaviour_net.train_process(stat, trainer)          # warm-up episode (allocations, rocBLAS plans)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for ep in range(a.episodes):
        trainer.behaviour_net.train_process(stat, trainer)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    steps = a.episodes * 95
    if rank == 0:
        out = {"metric": "training env-steps/s (rollout + replay + MADDPG updates)", "alg": a.alg,
               "value": a.envs * world * steps / dt, "unit": "env-steps/s", "n_gpus": world, "envs_per_gpu": a.envs,
               "gaussian_policy": bool(args.gaussian_policy), "n_agents": env.n_agents, "vector_steps": steps, "ms_per_vector_step": dt / steps * 1e3,
               "batch": trainer.effective_batch_size(),
               "grad_steps": int((a.episodes if a.episodic else steps) // args.behaviour_update_freq) * (args.value_update_epochs + args.policy_update_epochs
                                                                         + (args.mixer_update_epochs if args.mixer else 0)),
               "stat": {k: (float(v) if not isinstance(v, float) else v) for k, v in stat.items()},
               # fused paths that declined a call and ran their PyTorch composition instead (util.note_fallback): none expected
               "fallbacks": dict(FALLBACKS)}
        if a.gauss_burst:                   # asked for: the run must have rolled out through it
            rg = getattr(trainer.behaviour_net, "_rollout_graph", None)
            out["gauss_burst"] = bool(rg is not None and rg.fused_burst
                                      and (rg.gauss_burst or (rg.gaussian and getattr(rg, "mlp_burst", False))))
            if not out["gauss_burst"]:
                raise SystemExit("--gauss-burst: this configuration did not roll out through the one-launch burst "
                                 "(learner.RolloutGraph.gauss_burst, or mlp_burst with --agent-type mlp)")
        if a.agent_type != "rnn":
            out["agent_type"] = a.agent_type
            rg = getattr(trainer.behaviour_net, "_rollout_graph", None)
            if rg is not None and getattr(rg, "mlp_burst", False) and trainer.graph_rollout:
                out["rollout"] = "flexenv_rollout_burst_summed_mlp"      # (the one-launch burst with the MLP policy phase)
            if rg is not None and getattr(rg, "mlp_plain_burst", False) and trainer.graph_rollout:
                out["rollout"] = "flexenv_rollout_burst_mlp"             # (the same under MADDPG / SAFEMADDPG: in-kernel noise)
        if a.intended_actions:
            rg = getattr(trainer.behaviour_net, "_rollout_graph", None)
            out["intended_actions"] = True
            out["rollout_burst_launch"] = bool(rg is not None and rg.fused_burst and trainer.graph_rollout)
            if out["rollout_burst_launch"]:
                out["rollout"] = "flexenv_rollout_burst_routed"          # (the burst with the intended routing in the launch)
            if a.intended_launch and not out["rollout_burst_launch"]:     # asked for: the run must have rolled out through it
                raise SystemExit("--intended-launch: this configuration did not roll out through the one-launch burst "
                                 "(learner.RolloutGraph.fused_burst)")
        if a.unshared or a.unshared_twins:
            out["shared_params"] = False
        if a.unshared_critics:
            out["unshared_critics"] = True
        if a.episodic:
            out["episodic"] = True
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
