"""GPU: the two families of per-agent critic kernels agree, bit for bit, where they compute the same thing.  n plain critics on
maddpg.py's shared blocks (csrc/critic_unshared.hip, ``shared`` rows [o_1 .. o_n | onehot(i) | a_1 .. a_n]) and the twin critics
made of them by appending a non-zero flag column to every fc1.weight (csrc/critic_unshared_twin.hip): the first head's flag
input is 0, so a one-head twin launch is the plain launch — through the wide-load first layer (at_fc1_block_wide: "the bits are
at_fc1_block's") and through the stages of critic_unshared_stages.h under the head loop — and head 0 of a two-head launch is
that again ("its bits are a one-head launch's").  Every comparison is torch.equal.

Shapes, the smallest at which each path runs: one row; 33 rows of 3 agents with the blocks' row lengths 18 and 6 and fc1's 25,
so that no wide load is taken, and the same with the id columns (fc1's rows 28 long: 8-byte weight loads alone); 65 rows of 8
agents at obs 144 / act 8 with the id columns and LayerNorm (16-byte input loads; fc1's rows 1 225 long); 16 417 samples of
one agent, where the backward's grid is capped and a wavefront walks a second tile."""
import pytest
import torch as th

from .test_critic_unshared_gpu import SENTINEL, _critics

pytestmark = pytest.mark.gpu

# (b, n, obs_dim, act_dim, layernorm, agent_id)
CASES = [(1, 1, 6, 2, False, True), (33, 3, 6, 2, True, False), (33, 3, 6, 2, False, True), (65, 8, 144, 8, True, True),
         (16417, 1, 6, 2, True, True)]
SUMS = ("d_ln_w", "d_ln_b", "d_fc1_b", "d_fc2_b", "d_fc3_w")


def _filled(*shape):
    return th.full(shape, SENTINEL, dtype=th.float32, device="cuda")


def _launches(twin, heads, weights, obs, act, dq, layernorm, agent_id):
    """The forward with its saves, then the backward on them with the parameter sums and the own-action gradient, through the
    entry points of one family; every output pre-filled with a sentinel."""
    from safe_marl_amd import _lib
    b, n, o = obs.shape
    a = act.shape[2]
    rows = b * n
    stem = "flexnet_critic_unshared_twin" if twin else "flexnet_critic_unshared"
    fwd, bwd = ((_lib.FlexCriticUnsharedTwinArgs, _lib.FlexCriticUnsharedTwinBwdArgs) if twin else
                (_lib.FlexCriticUnsharedArgs, _lib.FlexCriticUnsharedBwdArgs))

    def head(s):
        s.rows, s.n_agents, s.w1, s.w2 = rows, n, n * o, n * a
        s.agent_id, s.layernorm, s.ln_eps = int(agent_id), int(layernorm), 1e-5
        if twin:
            s.heads = heads
        names = {f[0] for f in s._fields_}
        for i, w in enumerate(weights):
            for k, t in w.items():
                if k in names and t is not None:
                    getattr(s, k)[i] = t.data_ptr()
        return s

    out = {"q": _filled(heads, b, n), "z1": _filled(rows, 64), "x": _filled(heads, rows, 64), "dz1": _filled(rows, 64),
           "dz2": _filled(heads, rows, 64), "d_x2_own": _filled(rows, a), "d_fc3_b": _filled(n)}
    out.update({k: _filled(n, 64) for k in SUMS + (("d_flag",) if twin else ())})
    f = head(fwd())
    f.x1, f.x1_pitch, f.x1_agent_off = obs.data_ptr(), n * o, 0
    f.x2, f.x2_pitch, f.x2_agent_off = act.data_ptr(), n * a, 0
    f.q, f.save_z1, f.save_x = out["q"].data_ptr(), out["z1"].data_ptr(), out["x"].data_ptr()
    _lib.launch(stem + "_forward", f)
    g = head(bwd())
    g.param_grads = 1
    g.dq, g.z1, g.x = dq.data_ptr(), out["z1"].data_ptr(), out["x"].data_ptr()
    setattr(g, "dz1_sum" if twin else "dz1", out["dz1"].data_ptr())
    for k in ("dz2", "d_fc3_b") + SUMS + (("d_flag",) if twin else ()):
        setattr(g, k, out[k].data_ptr())
    g.d_x2_own, g.own_first, g.own_step, g.own_w = out["d_x2_own"].data_ptr(), 0, a, a
    ws = _filled(_lib.FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS if twin else _lib.FLEXNET_CRITIC_UNSHARED_WS_FLOATS)
    g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
    _lib.launch(stem + "_backward", g)
    th.cuda.synchronize()
    return out


@pytest.mark.parametrize("b,n,obs_dim,act_dim,layernorm,agent_id", CASES)
def test_a_twin_launch_is_the_plain_launch_on_the_first_head(b, n, obs_dim, act_dim, layernorm, agent_id):
    from safe_marl_amd.nets import _CRITIC_UNSHARED_TABLES, _critic_unshared_params
    critics = _critics(n, "maddpg", obs_dim, act_dim, layernorm, agent_id, seed=b + n)
    plain_w = [dict(zip(_CRITIC_UNSHARED_TABLES, (None if p is None else p.detach() for p in _critic_unshared_params(c))))
               for c in critics]
    g = th.Generator(device="cuda").manual_seed(100 * b + n)
    obs = 0.5 * th.randn(b, n, obs_dim, device="cuda", generator=g)
    act = 0.5 * th.randn(b, n, act_dim, device="cuda", generator=g)
    dq = th.randn(2, b, n, device="cuda", generator=g) / (b * n)
    twin_w = []
    for w in plain_w:                                          # the flag column: as large as the other columns, never zero
        flag = 0.3 + th.rand(64, 1, device="cuda", generator=g)
        twin_w.append(dict(w, fc1_w=th.cat([w["fc1_w"], flag], 1).contiguous()))
        assert twin_w[-1]["fc1_w"].shape[1] == w["fc1_w"].shape[1] + 1 and bool((twin_w[-1]["fc1_w"][:, -1] != 0).all())

    plain = _launches(False, 1, plain_w, obs, act, dq[0].contiguous(), layernorm, agent_id)
    one = _launches(True, 1, twin_w, obs, act, dq[:1].contiguous(), layernorm, agent_id)
    two = _launches(True, 2, twin_w, obs, act, dq, layernorm, agent_id)
    assert bool((plain["q"] != SENTINEL).all()) and bool((plain["dz1"] != SENTINEL).all())

    same = {}
    for k in ("q", "z1", "x", "dz1", "dz2", "d_x2_own", "d_fc3_b") + SUMS:
        if k in ("d_ln_w", "d_ln_b") and not layernorm:        # not written without LayerNorm, by either family
            same[k] = bool((plain[k] == SENTINEL).all() and (one[k] == SENTINEL).all())
        else:
            same[k] = th.equal(one[k].view(plain[k].shape), plain[k])
    same["two heads: q of head 0"] = th.equal(two["q"][0], plain["q"][0])
    same["two heads: x of head 0"] = th.equal(two["x"][0], plain["x"][0])
    same["two heads: z1"] = th.equal(two["z1"], plain["z1"])
    for k, v in same.items():
        print(f"b {b} n {n} o {obs_dim} a {act_dim} ln {layernorm} id {agent_id} {k}: {'identical' if v else 'DIFFERS'}")
    assert all(same.values()), [k for k, v in same.items() if not v]
    # the flag column is in use: the second head differs, and a one-head launch leaves no gradient on it
    assert not th.equal(two["q"][1], two["q"][0]) and bool((one["d_flag"] == 0).all())
