"""GPU: what csrc/flex_agent_tile.h claims.  The per-agent RNN actor (csrc/actor_unshared.hip), the per-agent critic
(csrc/critic_unshared.hip) and the per-agent MLP actor (csrc/actor_mlp.hip) run ONE first stage — the first layer's block product
over the observation columns, + bias + the agent's own id column, LayerNorm, ReLU — so on the same inputs and the same per-agent
fc1 / LayerNorm parameters their saves hold the same bits: ``save_x`` of all three, ``save_z1`` of the critic and the MLP actor
(the RNN actor saves z1 before the bias).  No tolerance: a pair that differs is a finding, not noise."""
import pytest
import torch as th

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
ACT = 4

# (b, n, obs_dim, layernorm, agent_id)
CASES = [(1, 1, 6, True, False),        # one partial tile; width below one k-group
         (33, 3, 30, True, True),       # a second tile with one live row; width no multiple of 8: the clamped loads run
         (129, 5, 144, False, True),    # a second work-group of an agent; no LayerNorm
         (31, 8, 30, True, True)]       # FLEXNET_MAX_AGENTS


def _table(args, name, tensors):
    for i, t in enumerate(tensors):
        getattr(args, name)[i] = t.data_ptr()


@pytest.mark.parametrize("b,n,obs_dim,layernorm,agent_id", CASES)
def test_the_three_forwards_share_their_first_stage(b, n, obs_dim, layernorm, agent_id):
    from safe_marl_amd import _lib
    g = th.Generator(device="cuda").manual_seed(1000 * b + n)
    rnd = lambda *shape, scale=1.0: scale * th.randn(*shape, device="cuda", generator=g)      # noqa: E731
    per_agent = lambda *shape, scale=1.0: [rnd(*shape, scale=scale) for _ in range(n)]      # noqa: E731
    new = lambda *shape: th.full(shape, SENTINEL, dtype=th.float32, device="cuda")            # noqa: E731
    rows, ld1, eps = b * n, obs_dim + (n if agent_id else 0), 1e-5
    obs = rnd(b, n, obs_dim, scale=0.5)
    first = {"fc1_w": per_agent(64, ld1, scale=0.3), "fc1_b": per_agent(64, scale=0.3),      # the shared stage: distinct per agent
             "ln_w": [1.0 + t for t in per_agent(64, scale=0.3)], "ln_b": per_agent(64, scale=0.3)}

    def fill(a, later):
        for name, tensors in list(first.items()) + list(later.items()):
            _table(a, name, tensors)
        a.rows, a.n_agents, a.agent_id, a.layernorm, a.ln_eps = rows, n, int(agent_id), int(layernorm), eps
        return later                                           # (kept alive by the caller until the launch is done)

    # the RNN actor, its six saves
    au = _lib.FlexActorUnsharedArgs()
    hid = rnd(b, n, 64, scale=0.5)
    keep = [fill(au, {"w_ih": per_agent(192, 64, scale=0.2), "w_hh": per_agent(192, 64, scale=0.2), "b_ih": per_agent(192, scale=0.2),
                      "b_hh": per_agent(192, scale=0.2), "fc2_w": per_agent(ACT, 64, scale=0.2), "fc2_b": per_agent(ACT, scale=0.2)})]
    au.obs_dim, au.act_dim, au.obs, au.hidden_in = obs_dim, ACT, obs.data_ptr(), hid.data_ptr()
    out_au = {k: new(rows, w) for k, w in (("means", ACT), ("hidden_out", 64), ("save_z1", 64), ("save_x", 64), ("save_r", 64),
                                           ("save_z", 64), ("save_n", 64), ("save_hn", 64))}
    # the critic on the observations alone: x1 = obs, agent a's block at a * obs_dim, no second block
    cu = _lib.FlexCriticUnsharedArgs()
    keep.append(fill(cu, {"fc2_w": per_agent(64, 64, scale=0.2), "fc2_b": per_agent(64, scale=0.2), "fc3_w": per_agent(64, scale=0.2),
                          "fc3_b": per_agent(1, scale=0.2)}))
    cu.w1, cu.w2, cu.x1, cu.x1_pitch, cu.x1_agent_off = obs_dim, 0, obs.data_ptr(), n * obs_dim, obs_dim
    out_cu = {"q": new(b, n), "save_z1": new(rows, 64), "save_x": new(rows, 64)}
    # the MLP actor
    am = _lib.FlexActorMlpUnsharedArgs()
    keep.append(fill(am, {"fc2_w": per_agent(64, 64, scale=0.2), "fc2_b": per_agent(64, scale=0.2), "fc3_w": per_agent(ACT, 64, scale=0.2),
                          "fc3_b": per_agent(ACT, scale=0.2)}))
    am.obs_dim, am.act_dim, am.hid, am.obs = obs_dim, ACT, 64, obs.data_ptr()
    out_am = {"means": new(rows, ACT), "h": new(rows, 64), "save_z1": new(rows, 64), "save_x": new(rows, 64)}

    for entry, a, outs in (("flexnet_actor_unshared_forward", au, out_au), ("flexnet_critic_unshared_forward", cu, out_cu),
                           ("flexnet_actor_mlp_unshared_forward", am, out_am)):
        for k, t in outs.items():
            setattr(a, k, t.data_ptr())
        _lib.launch(entry, a)
    th.cuda.synchronize()
    for outs in (out_au, out_cu, out_am):
        for k, t in outs.items():
            assert bool((t != SENTINEL).all()), k              # every row written

    def same(what, got, ref, pair):
        differ = int((got != ref).sum().item())
        print(f"b {b} n {n} o {obs_dim} ln {layernorm} id {agent_id} {what}, {pair}: {differ} of {ref.numel()} elements differ, "
              f"max |difference| {(got - ref).abs().max().item():.3e}")
        assert th.equal(got, ref), (what, pair)

    same("save_x", out_cu["save_x"], out_am["save_x"], "critic against MLP actor")
    same("save_x", out_au["save_x"], out_am["save_x"], "RNN actor against MLP actor")
    same("save_z1", out_cu["save_z1"], out_am["save_z1"], "critic against MLP actor")
